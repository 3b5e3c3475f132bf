"""The surface buffers of the geometry render without a GPU: the two entry points (``mofa_depth_median``, ``mofa_point_normals``) are
exported, declared and bound; each refuses bad arguments before any launch, with a message that names what was wrong; their kernels are
in the code object and light; ``Renderer.render_geometry`` / ``render_path_geometry`` refuse what they cannot do.  The kernels themselves
are compared in tests/test_gpu_surface.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from mofanerf_amd import build, factory, lib, synth
from mofanerf_amd.rays import pose_spherical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mofa_depth_median", "mofa_point_normals")


def test_the_two_entry_points_are_exported_declared_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    hdr = open(os.path.join(ROOT, "include", "mofanerf_hip.h")).read()
    pragma_on, pragma_off = hdr.index("#pragma GCC visibility push(default)"), hdr.index("#pragma GCC visibility pop")
    for name in NEW:
        assert name in exported, name
        m = re.search(r"\bint " + name + r"\s*\(", re.sub(r"/\*.*?\*/", lambda c: " " * len(c.group()), hdr, flags=re.S))
        assert m and pragma_on < m.start() < pragma_off, name
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert lib.load().mofa_abi_version() == 5 == lib.ABI_VERSION and lib.PROF_KINDS == 12
    assert int(re.search(r"#define MOFA_PROF_KINDS (\d+)", hdr).group(1)) == 12


def test_the_new_kernels_are_in_the_library_and_light():
    """k_depth_median<1|2|4>, k_depth_median_long and k_point_normals: at most 128 vector registers and no scratch, like every ray-side
    kernel (many rays per CU); the compositing kernels they stand next to are still there."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rs = {r["kernel"]: r for r in kernel_resources.resources(build.build())}
    want = [f"mofa::k_depth_median<{n}>" for n in (1, 2, 4)] + ["mofa::k_depth_median_long", "mofa::k_point_normals"]
    for k in want:
        assert k in rs, (k, sorted(rs))
        assert rs[k]["vgpr"] <= 128 and rs[k]["scratch"] == 0, (k, rs[k])
    for k in [f"mofa::k_composite_sigma<{n}>" for n in (1, 2, 4)] + ["mofa::k_composite_sigma_long", "mofa::k_ray_points"]:
        assert k in rs, k


def test_each_argument_error_returns_einval_with_its_message():
    L = lib.load()
    p = 256       # never dereferenced: every call below is refused before a launch
    err = L.mofa_last_error
    inf, nan = float("inf"), float("nan")
    # mofa_depth_median(weights, z, z_row_stride, n_rays, S, threshold, depth_med, index, stream)
    for k in (0, 1, 6, 7):
        args = [p, p, 0, 4, 8, 0.5, p, p, None]
        args[k] = None
        assert L.mofa_depth_median(*args) == -1 and b"depth_median: null pointer" in err(), k
    assert L.mofa_depth_median(p, p, 0, 0, 8, 0.5, p, p, None) == -1 and b"depth_median" in err() and b"0 rays" in err()
    assert L.mofa_depth_median(p, p, 0, -3, 8, 0.5, p, p, None) == -1 and b"-3 rays" in err()
    assert L.mofa_depth_median(p, p, 0, 4, 0, 0.5, p, p, None) == -1 and b"0 samples" in err()
    assert L.mofa_depth_median(p, p, 0, 2 ** 25, 64, 0.5, p, p, None) == -1 and b"2^31" in err()           # exactly 2^31 samples
    assert L.mofa_depth_median(p, p, 0, 2 ** 31, 1, 0.5, p, p, None) == -1 and b"2^31" in err()
    assert L.mofa_depth_median(p, p, 9, 4, 8, 0.5, p, p, None) == -1 and b"depth_median: z_row_stride = 9" in err()
    assert L.mofa_depth_median(p, p, 1, 4, 8, 0.5, p, p, None) == -1 and b"z_row_stride = 1" in err()
    for t, word in ((0.0, b"threshold = 0"), (-0.5, b"threshold = -0.5"), (inf, b"threshold = inf"), (-inf, b"threshold = -inf"), (nan, b"threshold = ")):
        assert L.mofa_depth_median(p, p, 0, 4, 8, t, p, p, None) == -1 and b"depth_median" in err() and word in err() and b"finite and > 0" in err(), t
    # mofa_point_normals(points, acc, rays_d, H, W, acc_min, normals, valid, stream)
    for k in (0, 1, 2, 6, 7):
        args = [p, p, p, 4, 4, 0.5, p, p, None]
        args[k] = None
        assert L.mofa_point_normals(*args) == -1 and b"point_normals: null pointer" in err(), k
    assert L.mofa_point_normals(p, p, p, 0, 4, 0.5, p, p, None) == -1 and b"point_normals: a 0 x 4 map" in err()
    assert L.mofa_point_normals(p, p, p, 4, 0, 0.5, p, p, None) == -1 and b"a 4 x 0 map" in err()
    assert L.mofa_point_normals(p, p, p, -1, 4, 0.5, p, p, None) == -1 and b"a -1 x 4 map" in err()
    assert L.mofa_point_normals(p, p, p, 2 ** 16, 2 ** 15, 0.5, p, p, None) == -1 and b"2^31" in err()      # exactly 2^31 pixels
    for a in (inf, -inf, nan):
        assert L.mofa_point_normals(p, p, p, 4, 4, a, p, p, None) == -1 and b"point_normals: acc_min = " in err() and b"finite" in err(), a


def _cpu_product():
    args = factory.default_args(netdepth=8, netwidth=64, netdepth_fine=8, netwidth_fine=64, no_reload=True, device="cpu", basedir="/nonexistent")
    _, kw, _, _, _, _, render = factory.create_nerf(args)
    return render.eval(), dict(kw, near=8.0, far=26.0)


def test_render_geometry_refuses_flat_rays_for_normals_an_unknown_surface_and_a_bad_threshold():
    render, kw = _cpu_product()
    bm, _, exp = synth.codes(0)
    K = synth.intrinsics(4, 4)
    flat = torch.zeros(2, 16, 3)
    flat[1, :, 2] = -1.0
    grid = flat.reshape(2, 4, 4, 3)
    call = lambda rays, **more: render.render_geometry(4, 4, K, rays=rays, shapeCodes=bm, expType=20, expCodes=exp, **dict(kw, **more))
    with pytest.raises(lib.MofaError, match=r"normals=True needs a 2-D grid of rays.*\[2, 16, 3\]"):
        call(flat, normals=True)
    for rays in (flat, grid):
        with pytest.raises(lib.MofaError, match="surface = 'mean'"):
            call(rays, surface="mean")
        for t in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(lib.MofaError, match="median_threshold"):
                call(rays, median=True, median_threshold=t)
        with pytest.raises(lib.MofaError, match="acc_min"):
            call(rays, normals=True, acc_min=float("nan"))
    for more in (dict(points=True), dict(normals=True)):              # NDC rays: a point on them is no scene position
        with pytest.raises(lib.MofaError, match="ndc=True"):
            call(grid, ndc=True, **more)
    with pytest.raises(lib.MofaError, match="GPU"):                   # a grid of rays, a median under NDC and flat rays without normals are
        call(grid, normals=True)                                      # all accepted: the device check is reached
    with pytest.raises(lib.MofaError, match="GPU"):
        call(grid, median=True, ndc=True)
    with pytest.raises(lib.MofaError, match="GPU"):
        call(flat, median=True, points=True, surface="expected")


def test_render_path_geometry_refuses_the_same_and_unknown_options(tmp_path):
    render, kw = _cpu_product()
    bm, _, exp = synth.codes(0)
    K = synth.intrinsics(4, 4)
    poses = [pose_spherical(10.0, 0.0, 16.0)]
    assert hasattr(render, "render_path_geometry")
    call = lambda **more: render.render_path_geometry(poses, (4, 4, float(K[0][0])), K, 1024, kw, expCodes=exp, shapeCodes=bm,
                                                      savedir=str(tmp_path), **more)
    with pytest.raises(lib.MofaError, match="surface = 'mean'"):
        call(surface="mean")
    with pytest.raises(lib.MofaError, match="median_threshold"):
        call(median_threshold=0.0)
    with pytest.raises(lib.MofaError, match="unknown argument 'normal'"):
        call(normal=True)
    with pytest.raises(lib.MofaError, match="far > near"):
        call(near=26.0, far=8.0)
    with pytest.raises(lib.MofaError, match="near and far are required"):
        render.render_path_geometry(poses, (4, 4, float(K[0][0])), K, 1024, {k: v for k, v in kw.items() if k not in ("near", "far")},
                                    expCodes=exp, shapeCodes=bm)
    with pytest.raises(lib.MofaError, match="GPU"):
        call()
    no_ndc = {k: v for k, v in kw.items() if k != "ndc"}              # a dictionary that never mentions NDC renders world-space rays
    with pytest.raises(lib.MofaError, match="GPU"):
        render.render_path_geometry(poses, (4, 4, float(K[0][0])), K, 1024, no_ndc, expCodes=exp, shapeCodes=bm)
    with pytest.raises(lib.MofaError, match="ndc=True"):              # one that asks for NDC rays is refused by name
        render.render_path_geometry(poses, (4, 4, float(K[0][0])), K, 1024, dict(kw, ndc=True), expCodes=exp, shapeCodes=bm)
    assert os.listdir(tmp_path) == []                                # nothing was written on the way to a refusal

"""The geometry-only render without a GPU: the three entry points (``mofa_ray_points``, ``mofa_composite_sigma``,
``mofa_occ_scatter_sigma``) are exported, declared and bound; each refuses bad arguments before any launch, with a message that names
what was wrong; ``Renderer.render_geometry`` refuses what it cannot do.  The kernels themselves are compared bit for bit in
tests/test_gpu_geometry.py."""
import os
import re
import subprocess

import pytest
import torch

from mofanerf_amd import build, factory, lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mofa_ray_points", "mofa_composite_sigma", "mofa_occ_scatter_sigma")


def test_the_three_entry_points_are_exported_declared_and_bound():
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    hdr = open(os.path.join(ROOT, "include", "mofanerf_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert name in exported, name
        assert re.search(r"\bint " + name + r"\s*\(", hdr), name
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert lib.load().mofa_abi_version() == 5 == lib.ABI_VERSION and lib.PROF_KINDS == 12
    assert int(re.search(r"#define MOFA_PROF_KINDS (\d+)", hdr).group(1)) == 12


def test_the_new_kernels_are_in_the_library_and_light():
    """k_composite_sigma<1|2|4> and k_composite_sigma_long next to the untouched k_composite<1|2|4> / k_composite_long: at most 128
    vector registers and no scratch, like every ray-side kernel (many rays per CU)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rs = {r["kernel"]: r for r in kernel_resources.resources(build.build())}
    want = [f"mofa::k_composite_sigma<{n}>" for n in (1, 2, 4)] + ["mofa::k_composite_sigma_long", "mofa::k_ray_points", "mofa::k_occ_scatter_sigma"]
    for k in want:
        assert k in rs, (k, sorted(rs))
        assert rs[k]["vgpr"] <= 128 and rs[k]["scratch"] == 0, (k, rs[k])
    for k in [f"mofa::k_composite<{n}>" for n in (1, 2, 4)] + ["mofa::k_composite_long"]:
        assert k in rs, k


def test_each_argument_error_returns_einval_with_its_message():
    L = lib.load()
    p = 256       # never dereferenced: every call below is refused before a launch
    err = L.mofa_last_error
    # mofa_ray_points(rays_o, rays_d, z, z_row_stride, n_rays, S, pts, stream)
    for k in (0, 1, 2, 6):
        args = [p, p, p, 0, 4, 8, p, None]
        args[k] = None
        assert L.mofa_ray_points(*args) == -1 and b"ray_points: null pointer" in err(), k
    assert L.mofa_ray_points(p, p, p, 0, 0, 8, p, None) == -1 and b"ray_points" in err() and b"0 rays" in err()
    assert L.mofa_ray_points(p, p, p, 0, 4, 0, p, None) == -1 and b"0 samples" in err()
    assert L.mofa_ray_points(p, p, p, 9, 4, 8, p, None) == -1 and b"z_row_stride = 9" in err()
    assert L.mofa_ray_points(p, p, p, 7, 4, 8, p, None) == -1 and b"z_row_stride = 7" in err()
    assert L.mofa_ray_points(p, p, p, 0, 2 ** 25, 64, p, None) == -1 and b"2^31" in err()          # exactly 2^31 samples
    assert L.mofa_ray_points(p, p, p, 0, 2 ** 31, 1, p, None) == -1 and b"2^31" in err()
    # mofa_composite_sigma(sigma, z, z_row_stride, rays_d, noise, n_rays, S, disp, acc, depth, weights, stream)
    for k in (0, 1, 3, 7, 8, 9, 10):                                                             # noise (4) may be NULL; weights may not
        args = [p, p, 0, p, None, 4, 8, p, p, p, p, None]
        args[k] = None
        assert L.mofa_composite_sigma(*args) == -1 and b"composite_sigma: null pointer" in err(), k
    assert L.mofa_composite_sigma(p, p, 0, p, None, 4, 1, p, p, p, p, None) == -1 and b"need S >= 2 (got 1)" in err()
    assert L.mofa_composite_forward(p, p, 0, p, None, 4, 1, 0, p, p, p, p, p, None) == -1 and b"need S >= 2 (got 1)" in err()   # the same words
    assert L.mofa_composite_sigma(p, p, 0, p, None, 0, 8, p, p, p, p, None) == -1
    assert L.mofa_composite_sigma(p, p, 5, p, None, 4, 8, p, p, p, p, None) == -1 and b"z_row_stride = 5" in err()
    assert L.mofa_composite_sigma(p, p, 0, p, None, 2 ** 25, 64, p, p, p, p, None) == -1 and b"2^31" in err()
    # mofa_occ_scatter_sigma(sigma_kept, flags, workspace, n_samples, n_kept, sigma, stream)
    for k in (1, 2, 5):
        args = [p, p, p, 32, 4, p, None]
        args[k] = None
        assert L.mofa_occ_scatter_sigma(*args) == -1 and b"occ_scatter_sigma: null pointer" in err(), k
    assert L.mofa_occ_scatter_sigma(None, p, p, 32, 1, p, None) == -1 and b"sigma_kept NULL" in err()
    assert L.mofa_occ_scatter_sigma(p, p, p, 32, 33, p, None) == -1 and b"n_kept = 33" in err()
    assert L.mofa_occ_scatter_sigma(p, p, p, 0, 0, p, None) == -1 and b"0 samples" in err()
    assert L.mofa_occ_scatter_sigma(p, p, p, 2 ** 31, 0, p, None) == -1


def _cpu_product():
    args = factory.default_args(netdepth=8, netwidth=64, netdepth_fine=8, netwidth_fine=64, no_reload=True, device="cpu", basedir="/nonexistent")
    _, kw, _, _, _, _, render = factory.create_nerf(args)
    return render.eval(), kw


def test_render_geometry_refuses_a_cpu_renderer_noise_and_unknown_keys():
    render, kw = _cpu_product()
    bm, _, exp = synth.codes(0)
    K = synth.intrinsics(4, 4)
    rays = torch.zeros(2, 16, 3)
    rays[1, :, 2] = -1.0
    call = lambda **more: render.render_geometry(4, 4, K, rays=rays, shapeCodes=bm, expType=20, expCodes=exp, **dict(kw, near=8.0, far=26.0, **more))
    assert hasattr(render, "render_geometry")
    with pytest.raises(lib.MofaError, match="GPU"):
        call()                                                   # the whole render_kwargs_test dictionary is accepted; the device is not
    with pytest.raises(lib.MofaError, match="raw_noise_std = 0.5"):
        call(raw_noise_std=0.5)
    with pytest.raises(lib.MofaError, match="unknown argument 'uvCodes'"):
        call(uvCodes=torch.zeros(256))                            # no texture argument exists
    with pytest.raises(lib.MofaError, match="unknown argument 'N_sample'"):
        call(N_sample=64)
    for k in ("white_bkgd", "use_viewdirs", "retraw", "network_query_fn", "verbose"):      # accepted and ignored: the device check is reached
        with pytest.raises(lib.MofaError, match="GPU"):
            call(**{k: True})

"""Mesh ray casting on the GPU (``mofa_ray_query``, ``mesh.ray_cast`` / ``ray_bounds``, ``Renderer.mesh_bounds``) against the NumPy
restatement (tests/ray_reference.py):

* ``ray_cast`` is brute force's bit for bit, and integer for integer on ``face`` (``ray_reference.mismatches``;
  tests/test_ray_reference_cpu.py shows what it catches), on the whole catalogue of ray sets, on every grid, for first and last hits
  and all three ``cull``; at one grid the walk's own counters are the restated walk's;
* the same input gives the same bytes, also on another stream;
* ``ray_bounds`` is its restatement; ``Renderer.mesh_bounds`` is the restatement on the rays the renderer generates, and
  ``render_geometry`` takes its columns as they are;
* bad input raises ``MofaError``, a bad index before any other kernel runs.
"""
import numpy as np
import pytest
import torch

import ray_reference as rr
import wind_reference as wr
from harness import make_product
from mofanerf_amd import lib, mesh, synth
from mofanerf_amd.rays import pose_spherical

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRIDS = (1, 2, 7, 32, None, (5, 9, 3))
WALK_GRID = 7
NAMES = [c["name"] for c in rr.catalogue()]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items()}
    return x.cpu().numpy() if torch.is_tensor(x) else x


def case_of(name):
    (c,) = [c for c in rr.catalogue() if c["name"] == name]
    return c


def gpu_args(c):
    return dev(c["origins"]), dev(c["dirs"]), dev(c["verts"]), dev(c["faces"])


def window(c):
    return dict(t_min=c["t_min"], t_max=None if np.isinf(c["t_max"]) else c["t_max"])


@pytest.mark.parametrize("name", NAMES)
def test_ray_cast_equals_brute_force_on_every_grid(name):
    c = case_of(name)
    a, table = gpu_args(c), rr.table_of(c)
    cpu = (c["origins"], c["dirs"], c["verts"], c["faces"])
    seen = 0
    for which in rr.WHICH:
        for cull in rr.CULL:
            want = rr.brute_force(*cpu, c["t_min"], c["t_max"], which, cull, table=table)
            seen += int(want["hit"].sum())
            for g in GRIDS:
                got = host(mesh.ray_cast(*a, which=which, cull=cull, grid=g, **window(c)))
                assert rr.mismatches(got, want) == [], (name, which, cull, g, rr.mismatches(got, want))
                assert np.array_equal(got["hit"], got["face"] >= 0)
                if g is not None:
                    assert got["grid"] == tuple(np.broadcast_to(g, (3,)))
    assert seen > 0 or name in ("cube_window2", "cube_window5")


@pytest.mark.parametrize("name", NAMES)
def test_the_walks_counters_are_the_restated_walks(name):
    c = case_of(name)
    a, table = gpu_args(c), rr.table_of(c)
    for which in rr.WHICH:
        walk = rr.grid_walk(c["origins"], c["dirs"], c["verts"], c["faces"], WALK_GRID, c["t_min"], c["t_max"], which, None, table=table)
        got = host(mesh.ray_cast(*a, which=which, grid=WALK_GRID, **window(c)))
        assert rr.mismatches(got, walk, rr.WALK_COUNTERS) == [], (name, which, got["counts"], walk["counts"])
        assert got["grid"] == (WALK_GRID,) * 3


def test_the_same_input_gives_the_same_bytes_also_on_another_stream():
    c = case_of("aimed_two_spheres")
    a = gpu_args(c)
    first = host(mesh.ray_cast(*a, which="last"))
    again = host(mesh.ray_cast(*a, which="last"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = mesh.ray_cast(*a, which="last")
    side.synchronize()
    other = host(other)
    for got in (again, other):
        assert rr.mismatches(got, first) == [] and got["counts"] == first["counts"] and got["grid"] == first["grid"]
    assert first["hit"].any() and not first["hit"].all()


@pytest.mark.parametrize("name,near,far,margin", [("cube_axes", 0.5, 3.0625, 0.125), ("cube_axes", 0.5, 2.75, 0.125),
                                                  ("aimed_torus", 0.25, 40.0, 0.1), ("bad_rays", 0.0, 8.0, 0.3)])
def test_ray_bounds_equals_its_restatement(name, near, far, margin):
    c = case_of(name)
    want = rr.ray_bounds(c["origins"], c["dirs"], c["verts"], c["faces"], near, far, margin)
    for g in (None, 3):
        got = host(mesh.ray_bounds(*gpu_args(c), near, far, margin, grid=g))
        assert rr.bounds_mismatches(got, want) == [], (name, g, rr.bounds_mismatches(got, want))
    assert want["hit"].any() and not want["hit"].all()
    assert (want["near"] >= np.float32(near)).all() and (want["far"] <= np.float32(far)).all()


def test_mesh_bounds_on_the_renderers_own_rays_and_the_geometry_render_takes_them():
    render, kw, _ = make_product((8, 64, 8, 64), 0, 4096, DEV)
    H, W = 6, 9                                                       # small and not square
    K = synth.intrinsics(H, W)
    pose = pose_spherical(-20.0, 10.0, 16.0)[:3, :4]
    verts, faces, _, _ = wr.field_case("sphere")
    verts = (3.0 * verts).astype(np.float32)
    v, f = dev(verts), dev(faces)
    near, far, margin = 8.0, 26.0, 0.5
    n, fa, hit = render.mesh_bounds(H, W, K, pose, v, f, near, far, margin)
    assert n.shape == fa.shape == (H * W, 1) and hit.shape == (H, W) and n.dtype == fa.dtype == torch.float32 and hit.dtype == torch.bool
    ro, rd, _, _ = render._make_rays(H, W, K, pose, None, True, None, False)
    want = rr.ray_bounds(ro.cpu().numpy(), rd.cpu().numpy(), verts, faces, near, far, margin)
    got = {"near": n.cpu().numpy().reshape(-1), "far": fa.cpu().numpy().reshape(-1), "hit": hit.cpu().numpy().reshape(-1)}
    assert rr.bounds_mismatches(got, want) == []
    assert want["hit"].any() and not want["hit"].all()
    inside = want["hit"]
    assert (want["far"][inside] - want["near"][inside] < 0.5 * (far - near)).all()        # the bounds hug a head of radius 3 at distance 16
    bm, _, exp = (x.to(DEV) for x in synth.codes(0))
    depth, disp, acc, _ = render.render_geometry(H, W, K, c2w=pose, shapeCodes=bm, expType=20, expCodes=exp, **dict(kw, near=n, far=fa, ndc=False))
    render.check_launches(block=True)
    assert depth.shape == acc.shape == (H, W) and torch.isfinite(depth).all() and torch.isfinite(acc).all()
    with pytest.raises(lib.MofaError, match="ndc"):
        render.mesh_bounds(H, W, K, pose, v, f, near, far, margin, ndc=True)


def test_no_rays_no_mesh_and_only_degenerate_faces():
    c = case_of("bad_rays")
    o, d, v, f = gpu_args(c)
    empty = mesh.ray_cast(o[:0], d[:0], v, f)
    assert empty["t"].shape == (0,) and empty["bary"].shape == (0, 3) and empty["face"].dtype == torch.int32
    bad = rr.bad_rays(c["origins"].astype(np.float64), c["dirs"].astype(np.float64))
    flat = dev(np.array([(0, 0, 0), (1, 1, 1), (2, 2, 2)], dtype=np.float32)), dev(np.array([(0, 1, 2)], dtype=np.int32))
    for vv, ff in ((v[:0], f[:0]), (v, f[:0]), flat):
        got = host(mesh.ray_cast(o, d, vv, ff))
        assert (got["face"] == -1).all() and not got["hit"].any() and np.isnan(got["bary"]).all() and np.isnan(got["point"]).all()
        assert np.isnan(got["t"][bad]).all() and np.isinf(got["t"][~bad]).all() and np.isnan(got["t64"][bad]).all()
        assert got["counts"]["bad_rays"] == int(bad.sum())
    assert got["counts"]["degenerate_faces"] == 1
    b = mesh.ray_bounds(o, d, v[:0], f[:0], 1.0, 2.0, 0.0)
    assert (b["near"] == 1.0).all() and (b["far"] == 2.0).all() and not b["hit"].any()


def test_refusals():
    c = case_of("cube_axes")
    o, d, v, f = gpu_args(c)
    L = lib.load()
    for bad, match in (((o.cpu(), d, v, f), "GPU"), ((o, d.cpu(), v, f), "GPU"), ((o, d, v.cpu(), f), "GPU"), ((o, d, v, f.cpu()), "GPU"),
                       ((o.double(), d, v, f), "float32"), ((o, d, v, f.long()), "int32"), ((o[:, :2].contiguous(), d, v, f), "points"),
                       ((o, d[:5], v, f), "directions"), ((o, d, v[:, :2].contiguous(), f), "verts")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.ray_cast(*bad)
    for kw in (dict(which="nearest"), dict(cull="both"), dict(grid=0), dict(grid=(2, 2)), dict(grid=mesh.DIST_GRID_CAP + 1), dict(grid=2.5),
               dict(t_min=2.0, t_max=1.0), dict(t_min=float("nan")), dict(t_max=float("nan"))):
        with pytest.raises(lib.MofaError, match="ray_cast"):
            mesh.ray_cast(o, d, v, f, **kw)
    for args in ((0.0, 1.0, -0.1), (1.0, 1.0, 0.1), (2.0, 1.0, 0.1), (0.0, float("nan"), 0.1), (0.0, 1.0, float("nan"))):
        with pytest.raises(lib.MofaError, match="ray_bounds"):
            mesh.ray_bounds(o, d, v, f, *args)
    # a bad index: refused after mofa_cc_validate, before any other kernel (a NaN vertex next to it is not reported)
    bad_f = f.clone()
    bad_f[3, 1] = 8
    bad_v = v.clone()
    bad_v[2, 0] = float("nan")
    with pytest.raises(lib.MofaError, match="face indices lie outside"):
        mesh.ray_cast(o, d, bad_v, bad_f)
    with pytest.raises(lib.MofaError, match="not finite"):
        mesh.ray_cast(o, d, bad_v, f)
    with pytest.raises(lib.MofaError, match="face indices lie outside"):
        mesh.ray_bounds(o, d, v, bad_f, 0.0, 1.0, 0.1)
    assert L.mofa_ray_query(None, None, 1, None, None, 1, None, 1, None, None, None, None, None, None, 0, 0.0, 1.0, 0, 0, None, None, None, None, None,
                            None, None, None) == -1 and b"null pointer" in L.mofa_last_error()

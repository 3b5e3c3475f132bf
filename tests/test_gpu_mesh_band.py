"""Narrow-band extraction on the GPU (``mesh.band_surface`` / ``mofa_band_*`` / ``Renderer.extract_mesh(brick=B)``).

* the band mesh equals ``mesh.iso_surface`` on the dense grid of the same function after renumbering by edge id (vertex bits equal,
  oriented triangles equal as a multiset), and equals the NumPy restatement (tests/band_reference.py) byte for byte in its own order;
* the GPU's active bricks equal the NumPy fixed point of seeding plus growth;
* the output bytes do not depend on the run or the chunk size;
* the documented limitation (a component inside bricks whose corners do not straddle the level is missed) holds as stated.
"""
import numpy as np
import pytest
import torch

import band_reference as br
import mt_reference as mt
from mofanerf_amd import lib, mesh, synth
from mofanerf_amd.model import NeRF
from mofanerf_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _shipped_launch_forms(monkeypatch):
    for k in ("MOFA_PIPE", "MOFA_CHAIN", "MOFA_FUSED", "MOFA_CHAIN_TRAIN"):
        monkeypatch.delenv(k, raising=False)
    lib.reload_env()
    lib.test_hooks()
    yield
    monkeypatch.undo()
    lib.reload_env()
    lib.test_hooks()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(*ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


# ---- fields: per point, exactly rounded float32 operations only (+ - * / sqrt, max), so every evaluation of a point gives its bits ---
def _norm(x, y, z):
    return torch.sqrt(x * x + y * y + z * z)


def sphere(p, r=0.6, c=(0.0, 0.0, 0.0)):
    return r - _norm(p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2])


def torus(p, R=0.55, r=0.2, zc=0.0):
    q = torch.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) - R
    z = p[:, 2] - zc
    return r - torch.sqrt(q * q + z * z)


def two_spheres(p):
    return torch.maximum(sphere(p, 0.3, (0.45, 0.0, 0.0)), sphere(p, 0.3, (-0.45, 0.0, 0.0)))


def ring_and_ball(p):
    """A thin ring off the brick-corner planes and one ball that holds a brick corner: the seeds sit at the ball only."""
    return torch.maximum(torus(p, 0.6, 0.06, 0.12), sphere(p, 0.15, (0.5, 0.25, 0.0)))


FIELDS = {"sphere": sphere, "torus": torus, "two_spheres": two_spheres, "ring_and_ball": ring_and_ball}
CHI = {"sphere": 2, "torus": 0, "two_spheres": 4}


def dense(fn, res, lo, step):
    """The dense grid of fn and its mesh (mesh.iso_surface)."""
    n = res[0] * res[1] * res[2]
    pts = torch.empty(n, 3, device=DEV)
    mesh.grid_points(res, lo, step, 0, n, pts)
    grid = fn(pts).reshape(res).contiguous()
    return grid


def check_equals_dense(v, f, ids, grid, level, lo, step):
    """band (v, f, ids) renumbered == mesh.iso_surface of the dense grid: vertex bits equal, oriented faces equal as a multiset."""
    dv, df = mesh.iso_surface(grid, level, lo, step)
    dv, df = host(dv, df)
    rv, rf, rids = br.renumber(v, f, ids)
    assert len(rv) == len(dv) and np.array_equal(bits(rv), bits(dv))
    assert np.array_equal(rf, br.canonical_faces(df))
    assert len(np.unique(ids)) == len(ids)
    return dv, df


def run_band(fn, res, lo, step, level, B, chunk=1 << 16):
    v, f, ids, stats = mesh.band_surface(fn, res, lo, step, level, B, chunk)
    v, f, ids = host(v, f, ids)
    return v, f, ids, stats


def active_set(stats, res, B):
    nb = br.bricks_per_axis(res, B)
    a = np.zeros(int(np.prod(nb)), bool)
    a[stats["active_bricks"]] = True
    return a.reshape(nb)


@pytest.mark.parametrize("name,res,B", [("sphere", (33, 41, 25), 4), ("torus", (49, 57, 41), 4), ("sphere", (57, 41, 49), 8),
                                        ("two_spheres", (41, 49, 33), 8), ("sphere", (65, 49, 81), 16), ("two_spheres", (65, 33, 65), 16),
                                        ("torus", (129, 97, 97), 16)])
def test_band_equals_dense_on_analytic_fields(name, res, B):
    lo, step = mt.cube_grid(res)
    fn = FIELDS[name]
    v, f, ids, stats = run_band(fn, res, lo, step, 0.0, B)
    grid = dense(fn, res, lo, step)
    check_equals_dense(v, f, ids, grid, 0.0, lo, step)
    g = grid.cpu().numpy()
    active, seeded, rounds = br.active_fixed_point(g, 0.0, B)
    assert np.array_equal(active_set(stats, res, B), active)
    assert stats["bricks_seeded"] == seeded.sum() and stats["rounds"] == rounds and stats["bricks_total"] == active.size
    assert np.array_equal(stats["active_bricks"], np.flatnonzero(active.reshape(-1)))
    assert stats["points_evaluated"] == np.prod([n // B + 1 for n in res]) + active.sum() * (B + 1) ** 3
    assert stats["points_dense"] == np.prod(res)
    # the GPU's own order: the NumPy restatement byte for byte
    rv, rf, rids = br.band_mesh(g, 0.0, lo, step, B, active)
    assert np.array_equal(ids, rids) and np.array_equal(f, rf) and np.array_equal(bits(v), bits(rv))
    assert len(f) > 500 and f.dtype == np.int32 and ids.dtype == np.int64
    assert mt.is_closed_oriented_manifold(f) and mt.euler_characteristic(v, f) == CHI[name] and mt.signed_volume(v, f) > 0
    # no atomics: the same bytes on a second run and at three chunk sizes (one not a multiple of a brick's points)
    for chunk in (1 << 16, 1000, 4097, (B + 1) ** 3 * 3):
        v2, f2, ids2, _ = run_band(fn, res, lo, step, 0.0, B, chunk)
        assert np.array_equal(bits(v2), bits(v)) and np.array_equal(f2, f) and np.array_equal(ids2, ids)


def test_band_growth_reaches_what_the_corners_miss():
    res, B = (65, 65, 33), 8
    lo, step = mt.cube_grid(res)
    v, f, ids, stats = run_band(ring_and_ball, res, lo, step, 0.0, B)
    assert stats["bricks_active"] > stats["bricks_seeded"] > 0 and stats["rounds"] >= 2, stats
    grid = dense(ring_and_ball, res, lo, step)
    check_equals_dense(v, f, ids, grid, 0.0, lo, step)
    active, _, rounds = br.active_fixed_point(grid.cpu().numpy(), 0.0, B)
    assert np.array_equal(active_set(stats, res, B), active) and stats["rounds"] == rounds
    assert mt.is_closed_oriented_manifold(f)


def test_band_misses_a_component_inside_one_brick():
    """The documented limitation: a small sphere strictly inside one brick with no brick corner inside — the band is empty, the dense
    mesh is not."""
    res, B = (33, 33, 33), 16
    lo, step = mt.cube_grid(res)
    fn = lambda p: sphere(p, 0.2, (0.5, 0.5, 0.5))          # noqa: E731
    v, f, ids, stats = run_band(fn, res, lo, step, 0.0, B)
    assert v.shape == (0, 3) and f.shape == (0, 3) and ids.shape == (0,)
    assert stats["bricks_seeded"] == stats["bricks_active"] == 0 and stats["rounds"] == 0
    dv, df = host(*mesh.iso_surface(dense(fn, res, lo, step), 0.0, lo, step))
    assert len(df) > 100


def test_band_ties_at_the_level_equal_dense():
    """An integer-valued field, round(8 sigma) of the sphere: a thick shell of samples equal to the level."""
    res, B = (49, 41, 57), 8
    lo, step = mt.cube_grid(res)
    fn = lambda p: torch.round(8.0 * sphere(p))                   # noqa: E731
    v, f, ids, stats = run_band(fn, res, lo, step, 2.0, B)
    grid = dense(fn, res, lo, step)
    assert (grid == 2.0).sum() > 1000 and len(f) > 1000
    check_equals_dense(v, f, ids, grid, 2.0, lo, step)
    assert mt.is_closed_oriented_manifold(f)


def test_band_ties_on_random_integers_equal_the_restatement():
    """A random integer grid looked up by the point's lattice index: many samples equal the level, many small components — the band
    output equals the NumPy restatement on the active bricks of its fixed point, byte for byte."""
    rng = np.random.default_rng(7)
    res, B = (29, 33, 21), 4
    table = torch.from_numpy(rng.integers(0, 5, res).astype(np.float32)).to(DEV)
    lo, step = mt.cube_grid(res, 2.0)
    lo_t, step_t = torch.from_numpy(lo).to(DEV), torch.from_numpy(step).to(DEV)

    def fn(p):
        ijk = torch.round((p - lo_t) / step_t).long()
        return table[ijk[:, 0], ijk[:, 1], ijk[:, 2]]

    v, f, ids, stats = run_band(fn, res, lo, step, 2.0, B)
    grid = dense(fn, res, lo, step)
    assert torch.equal(grid, table) and (grid == 2.0).sum() > 1000 and len(f) > 1000
    g = grid.cpu().numpy()
    active, _, _ = br.active_fixed_point(g, 2.0, B)
    assert np.array_equal(active_set(stats, res, B), active)
    rv, rf, rids = br.band_mesh(g, 2.0, lo, step, B, active)
    assert np.array_equal(ids, rids) and np.array_equal(f, rf) and np.array_equal(bits(v), bits(rv))


@pytest.mark.parametrize("value", [0.0, 2.0])
def test_band_uniform_field_is_empty(value):
    res = (17, 25, 9)
    lo, step = mt.cube_grid(res)
    v, f, ids, stats = run_band(lambda p: torch.full((p.shape[0],), value, device=DEV), res, lo, step, 1.0, 8)
    assert v.shape == (0, 3) and f.shape == (0, 3) and ids.shape == (0,)
    assert stats["bricks_active"] == 0 and stats["points_evaluated"] == 3 * 4 * 2


def test_band_non_finite_density_raises():
    res, B = (33, 33, 33), 8
    lo, step = mt.cube_grid(res)

    def fn(p):                                                    # NaN on a thin shell round the surface: inside the band, not at a corner
        s = sphere(p)
        return torch.where(s.abs() < 0.02, torch.full_like(s, float("nan")), s)

    with pytest.raises(lib.MofaError, match="non-finite"):
        mesh.band_surface(fn, res, lo, step, 0.0, B, 4096)
    with pytest.raises(lib.MofaError, match="non-finite"):
        mesh.band_surface(lambda p: sphere(p) / 0.0, res, lo, step, 0.0, B, 4096)


def test_band_large_grid_evaluates_a_small_fraction():
    """513^3 at B = 8: under 15 % of the dense points, and still the dense mesh."""
    res, B = (513, 513, 513), 8
    lo, step = mt.cube_grid(res)
    v, f, ids, stats = run_band(sphere, res, lo, step, 0.0, B, 1 << 20)
    frac = stats["points_evaluated"] / stats["points_dense"]
    print(f"513^3 sphere, B = 8: {stats['bricks_active']} of {stats['bricks_total']} bricks, {frac:.4f} of the dense points")
    assert frac < 0.15
    check_equals_dense(v, f, ids, dense(sphere, res, lo, step), 0.0, lo, step)


def test_band_rounds_span_several_launches():
    """513^3 at B = 4, a sphere of radius 0.8: the seeded round and the active set each hold more than three launches' worth of bricks
    (the per-brick kernels launch at most 2^14 workgroups at a time), so grow, count and emit run launches that start past brick 0 —
    and the mesh is still the dense one."""
    res, B = (513, 513, 513), 4
    lo, step = mt.cube_grid(res)
    fn = lambda p: sphere(p, 0.8)                                 # noqa: E731
    v, f, ids, stats = run_band(fn, res, lo, step, 0.0, B, 1 << 20)
    assert stats["bricks_seeded"] > 3 * (1 << 14) and stats["bricks_active"] > 3 * (1 << 14), stats["bricks_seeded"]
    check_equals_dense(v, f, ids, dense(fn, res, lo, step), 0.0, lo, step)


def test_band_abi_refuses_a_wrong_active_count():
    """mofa_band_count / mofa_band_emit read the workspace's active count back and refuse any other n_active (the mesh workspace, the brick
    list and the launches are sized by it).  Driven through the C ABI: seed, evaluate the seeded bricks, then count and emit."""
    L = lib.load()
    res, B = (33, 33, 33), 8
    nx, ny, nz = res
    lo, step = mt.cube_grid(res)
    lo3, st3 = mesh._f3(lo), mesh._f3(step)
    st = lib.stream()
    ws = torch.empty(L.mofa_band_workspace_bytes(nx, ny, nz, B), dtype=torch.uint8, device=DEV)
    counts = torch.empty(2, dtype=torch.int64, device=DEV)
    n_corners = 5 ** 3
    pts = torch.empty(n_corners, 3, device=DEV)
    lib.check(L.mofa_band_corner_points(nx, ny, nz, B, lo3, st3, 0, n_corners, lib.ptr(pts), st), "mofa_band_corner_points")
    corner_sigma = sphere(pts).contiguous()
    lib.check(L.mofa_band_seed(nx, ny, nz, B, lib.ptr(corner_sigma), 0.0, ws.data_ptr(), counts.data_ptr(), st), "mofa_band_seed")
    n_new, n_active = counts.tolist()
    assert n_new == n_active > 1
    P = (B + 1) ** 3
    bpts = torch.empty(n_active * P, 3, device=DEV)
    lib.check(L.mofa_band_points(nx, ny, nz, B, lo3, st3, ws.data_ptr(), n_new, 0, n_active * P, lib.ptr(bpts), st), "mofa_band_points")
    sigma = sphere(bpts).contiguous()
    mws = torch.empty(L.mofa_band_mesh_bytes(B, n_active + 1), dtype=torch.uint8, device=DEV)
    bricks = torch.full((n_active + 1,), -1, dtype=torch.int64, device=DEV)
    for wrong in (n_active - 1, n_active + 1):
        assert L.mofa_band_count(nx, ny, nz, B, lib.ptr(sigma), 0.0, ws.data_ptr(), wrong, mws.data_ptr(), counts.data_ptr(),
                                 bricks.data_ptr(), st) == -1
        assert b"active bricks" in L.mofa_last_error()
    assert (bricks == -1).all()                                   # refused before any launch
    lib.check(L.mofa_band_count(nx, ny, nz, B, lib.ptr(sigma), 0.0, ws.data_ptr(), n_active, mws.data_ptr(), counts.data_ptr(),
                                bricks.data_ptr(), st), "mofa_band_count")
    V, F = counts.tolist()
    assert V > 0 and F > 0 and int(bricks[-1]) == -1 and (bricks[:-1] >= 0).all()
    verts = torch.empty(V, 3, device=DEV)
    edge_ids = torch.empty(V, dtype=torch.int64, device=DEV)
    faces = torch.empty(F, 3, dtype=torch.int32, device=DEV)
    args = (lib.ptr(verts), edge_ids.data_ptr(), faces.data_ptr(), st)
    assert L.mofa_band_emit(nx, ny, nz, B, lo3, st3, lib.ptr(sigma), 0.0, ws.data_ptr(), n_active + 1, mws.data_ptr(), *args) == -1
    assert b"active bricks" in L.mofa_last_error()
    lib.check(L.mofa_band_emit(nx, ny, nz, B, lo3, st3, lib.ptr(sigma), 0.0, ws.data_ptr(), n_active, mws.data_ptr(), *args),
              "mofa_band_emit")
    torch.cuda.synchronize()
    assert torch.isfinite(verts).all() and len(torch.unique(edge_ids)) == V


# ---- the network ----------------------------------------------------------------------------------------------------------------------
def make(D, W, seed=1, netchunk=1024 * 64):
    render = Renderer(netchunk=netchunk, expCodesLen=30)
    render.idSpecificMod.load_state_dict(synth.style_state(0))
    for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(0)):
        dst.data[:] = src
    render = render.to(DEV).eval()
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, seed))
    return render, net.to(DEV)


@pytest.mark.parametrize("D,W,forms", [(8, 256, ()), (10, 1024, ()), (10, 1024, (("MOFA_CHAIN", "0"),))])
def test_extract_mesh_band_equals_dense_on_the_network(D, W, forms, knob):
    for k, val in forms:
        knob(k, val)
    render, net = make(D, W)
    bm, tex, e = [t.to(DEV) for t in synth.codes(3)]
    bounds, res, B = ((-1.0, -1.1, -0.9), (1.1, 0.9, 1.0)), (129, 129, 129), 8
    grid = render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm, expCodes=e)
    g = grid.cpu().numpy()
    # a level at which every component of the surface is seeded (the band's precondition for equality), from a fixed list of quantiles
    level = None
    for q in (0.5, 0.4, 0.6, 0.3, 0.7, 0.2, 0.8):
        lv = float(np.quantile(g, q))
        active, _, _ = br.active_fixed_point(g, lv, B)
        nb = br.bricks_per_axis(res, B)
        m = br.mixed_cells(g, lv).reshape(nb[0], B, nb[1], B, nb[2], B).any(axis=(1, 3, 5))
        if not (m & ~active).any():
            level = lv
            break
    assert level is not None, "no tested level has every surface component seeded"
    verts, faces = render.extract_mesh(net, bounds=bounds, resolution=res, level=level, shapeCodes=bm, expCodes=e, brick=B)
    stats = render.mesh_stats
    assert np.array_equal(active_set(stats, res, B), active)
    v, f, ids = host(verts, faces, stats["edge_ids"])
    dv, df = render.extract_mesh(net, bounds=bounds, resolution=res, level=level, shapeCodes=bm, expCodes=e)
    dv, df = host(dv, df)
    rv, rf, _ = br.renumber(v, f, ids)
    assert len(df) > 1000 and np.array_equal(bits(rv), bits(dv)) and np.array_equal(rf, br.canonical_faces(df))
    print(f"{D}x{W} {res}: level {level:.4f}, {stats['bricks_active']} of {stats['bricks_total']} bricks, "
          f"{stats['points_evaluated'] / stats['points_dense']:.3f} of the dense points, {stats['rounds']} growth rounds")
    # colours: the same vertices, normals summed in another order
    v2, f2, rgb = render.extract_mesh(net, bounds=bounds, resolution=res, level=level, shapeCodes=bm, expCodes=e, uvCodes=tex,
                                      colors=True, brick=B)
    assert torch.equal(v2, verts) and torch.equal(f2, faces)
    _, _, drgb = render.extract_mesh(net, bounds=bounds, resolution=res, level=level, shapeCodes=bm, expCodes=e, uvCodes=tex, colors=True)
    order = np.argsort(ids, kind="stable")
    c, dc = host(rgb, drgb)
    assert c.shape == v.shape and np.abs(c[order] - dc).max() <= 1e-5

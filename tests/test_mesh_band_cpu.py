"""Narrow-band extraction without a GPU: the argument checks of the mofa_band_* entry points and of mesh.band_surface (which refuse before
any launch), and the NumPy restatement (tests/band_reference.py): the active-brick fixed point of seeding plus growth, and the band mesh
built from it, which equals the dense marching tetrahedra after renumbering by edge_id whenever every component is seeded."""
import ctypes as C
import math

import numpy as np
import pytest

import band_reference as br
import mt_reference as mt
from mofanerf_amd import lib, mesh

EINVAL = -1


def _f3(*v):
    return (C.c_float * 3)(*v)


def test_band_entry_points_validate_before_launching():
    L = lib.load()
    ws, p, out = 1, 1, 1                                          # (never dereferenced: every call below is refused first)
    lo, step = _f3(-1, -1, -1), _f3(0.1, 0.1, 0.1)
    good = (17, 25, 33)
    assert L.mofa_band_workspace_bytes(*good, 8) > 0
    assert L.mofa_band_workspace_bytes(4097, 4097, 4097, 8) > 0  # >= 4097 samples per axis
    assert L.mofa_band_workspace_bytes(4097, 4097, 4097, 4) > 0
    assert L.mofa_band_mesh_bytes(8, 10) >= 10 * 7 * 9 ** 3 * 2
    for b in (0, 2, 3, 5, 7, 12, 32, -8):                         # B not in {4, 8, 16}
        assert L.mofa_band_workspace_bytes(*good, b) == 0
        assert L.mofa_band_mesh_bytes(b, 10) == 0
        assert L.mofa_band_seed(*good, b, p, 0.0, ws, out, None) == EINVAL
        assert b"brick size" in L.mofa_last_error()
    assert L.mofa_band_mesh_bytes(8, 0) == 0
    for shape in ((18, 25, 33), (17, 24, 33), (17, 25, 34), (1, 25, 33), (0, 25, 33), (5, 9, 13)):   # (n - 1) % B != 0, n < 2
        assert L.mofa_band_workspace_bytes(*shape, 8) == 0
        assert L.mofa_band_seed(*shape, 8, p, 0.0, ws, out, None) == EINVAL
        assert L.mofa_band_corner_points(*shape, 8, lo, step, 0, 1, out, None) == EINVAL
        assert L.mofa_band_points(*shape, 8, lo, step, ws, 1, 0, 1, out, None) == EINVAL
        assert L.mofa_band_grow(*shape, 8, p, 0.0, ws, 1, out, None) == EINVAL
        assert L.mofa_band_count(*shape, 8, p, 0.0, ws, 1, ws, out, None, None) == EINVAL
        assert L.mofa_band_emit(*shape, 8, lo, step, p, 0.0, ws, 1, ws, out, out, out, None) == EINVAL
    # oversized grids: an axis of 2^24 samples or more, 2^31 brick corners or more
    for shape, b in (((2 ** 24 + 1, 17, 17), 8), ((2 ** 40 + 1, 17, 17), 8), ((8193, 8193, 8193), 4), ((16385, 16385, 4097), 8)):
        assert L.mofa_band_workspace_bytes(*shape, b) == 0
        assert L.mofa_band_seed(*shape, b, p, 0.0, ws, out, None) == EINVAL
        assert b"too large" in L.mofa_last_error()
        assert L.mofa_band_emit(*shape, b, lo, step, p, 0.0, ws, 1, ws, out, out, out, None) == EINVAL
    # a non-finite level
    for level in (float("nan"), float("inf"), -float("inf")):
        assert L.mofa_band_seed(*good, 8, p, level, ws, out, None) == EINVAL
        assert b"level" in L.mofa_last_error()
        assert L.mofa_band_grow(*good, 8, p, level, ws, 1, out, None) == EINVAL
        assert L.mofa_band_count(*good, 8, p, level, ws, 1, ws, out, None, None) == EINVAL
        assert L.mofa_band_emit(*good, 8, lo, step, p, level, ws, 1, ws, out, out, out, None) == EINVAL
    # null pointers (the brick list of mofa_band_count is optional)
    for i in range(3):
        a = [p, ws, out]
        a[i] = None
        assert L.mofa_band_seed(*good, 8, a[0], 0.0, a[1], a[2], None) == EINVAL
        assert b"null pointer" in L.mofa_last_error()
        assert L.mofa_band_grow(*good, 8, a[0], 0.0, a[1], 1, a[2], None) == EINVAL
    for i in range(3):
        a = [lo, step, out]
        a[i] = None
        assert L.mofa_band_corner_points(*good, 8, a[0], a[1], 0, 1, a[2], None) == EINVAL
    for i in range(4):
        a = [lo, step, ws, out]
        a[i] = None
        assert L.mofa_band_points(*good, 8, a[0], a[1], a[2], 1, 0, 1, a[3], None) == EINVAL
    for i in range(4):
        a = [p, ws, ws, out]
        a[i] = None
        assert L.mofa_band_count(*good, 8, a[0], 0.0, a[1], 1, a[2], a[3], None, None) == EINVAL
    for i in range(8):
        a = [lo, step, p, ws, ws, out, out, out]
        a[i] = None
        assert L.mofa_band_emit(*good, 8, a[0], a[1], a[2], 0.0, a[3], 1, a[4], a[5], a[6], a[7], None) == EINVAL
        assert b"null pointer" in L.mofa_last_error()
    # ranges: corners / points past the end, brick counts outside the brick grid, bad geometry
    n_corners = 3 * 4 * 5
    assert L.mofa_band_corner_points(*good, 8, lo, step, 0, n_corners + 1, out, None) == EINVAL
    assert L.mofa_band_corner_points(*good, 8, lo, step, -1, 2, out, None) == EINVAL
    assert L.mofa_band_points(*good, 8, lo, step, ws, 2, 0, 2 * 729 + 1, out, None) == EINVAL
    assert L.mofa_band_points(*good, 8, lo, step, ws, 0, 0, 1, out, None) == EINVAL
    assert L.mofa_band_points(*good, 8, lo, step, ws, 2 * 3 * 4 + 1, 0, 1, out, None) == EINVAL
    assert L.mofa_band_grow(*good, 8, p, 0.0, ws, 0, out, None) == EINVAL
    assert L.mofa_band_count(*good, 8, p, 0.0, ws, 0, ws, out, None, None) == EINVAL
    assert L.mofa_band_emit(*good, 8, lo, _f3(0.1, 0.0, 0.1), p, 0.0, ws, 1, ws, out, out, out, None) == EINVAL
    assert L.mofa_band_emit(*good, 8, _f3(float("nan"), 0, 0), step, p, 0.0, ws, 1, ws, out, out, out, None) == EINVAL
    # every entry point that takes the grid geometry refuses a non-finite lo or a step <= 0
    for lo_, st_ in ((lo, _f3(0.1, 0.0, 0.1)), (lo, _f3(0.1, -0.1, 0.1)), (_f3(float("nan"), 0, 0), step), (_f3(0, float("inf"), 0), step)):
        assert L.mofa_band_corner_points(*good, 8, lo_, st_, 0, 1, out, None) == EINVAL
        assert b"step > 0" in L.mofa_last_error()
        assert L.mofa_band_points(*good, 8, lo_, st_, ws, 1, 0, 1, out, None) == EINVAL
        assert b"step > 0" in L.mofa_last_error()
        assert L.mofa_band_emit(*good, 8, lo_, st_, p, 0.0, ws, 1, ws, out, out, out, None) == EINVAL
    assert L.mofa_abi_version() == 5


def test_band_surface_refuses_before_touching_the_gpu():
    def never(pts):
        raise AssertionError("density_fn called")

    lo, step = np.full(3, -1, np.float32), np.full(3, 0.1, np.float32)
    for res, b in (((17, 17, 17), 5), ((17, 17, 17), 32), ((18, 17, 17), 8), ((8193, 8193, 8193), 4), ((17, 17, 1), 8)):
        with pytest.raises(lib.MofaError):
            mesh.band_surface(never, res, lo, step, 0.0, b, 1024)
    for level in (float("nan"), float("inf")):
        with pytest.raises(lib.MofaError, match="level"):
            mesh.band_surface(never, (17, 17, 17), lo, step, level, 8, 1024)
    with pytest.raises(lib.MofaError, match="step"):
        mesh.band_surface(never, (17, 17, 17), lo, np.float32([0.1, 0, 0.1]), 0.0, 8, 1024)
    with pytest.raises(lib.MofaError, match="chunk"):
        mesh.band_surface(never, (17, 17, 17), lo, step, 0.0, 8, 0)


# ---- the NumPy restatement ----------------------------------------------------------------------------------------------------------
def _check_band_equals_dense(g, level, lo, step, B):
    active, seeded, rounds = br.active_fixed_point(g, level, B)
    assert (active >= seeded).all()
    v, f, ids = br.band_mesh(g, level, lo, step, B, active)
    dv, df = mt.marching_tets(g, level, lo, step)
    rv, rf, rids = br.renumber(v, f, ids)
    assert np.array_equal(rids, br.dense_edge_ids(g, level))
    assert np.array_equal(rv.view(np.uint32), dv.view(np.uint32))
    assert np.array_equal(rf, br.canonical_faces(df))
    return active, seeded, rounds, v, f


@pytest.mark.parametrize("name,res,B", [("sphere", (33, 41, 25), 4), ("torus", (49, 57, 41), 4), ("sphere", (57, 41, 49), 8),
                                        ("two_spheres", (41, 49, 33), 8), ("sphere", (65, 49, 81), 16), ("two_spheres", (65, 33, 65), 16)])
def test_reference_band_equals_dense_on_analytic_fields(name, res, B):
    lo, step = mt.cube_grid(res)
    g = mt.field(name, res, lo, step)
    active, _, _, v, f = _check_band_equals_dense(g, 0.0, lo, step, B)
    assert len(f) > 200 and active.sum() < active.size
    assert mt.is_closed_oriented_manifold(f) and mt.signed_volume(v, f) > 0
    assert mt.euler_characteristic(v, f) == {"sphere": 2, "torus": 0, "two_spheres": 4}[name]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_band_equals_dense_on_random_blobs(seed):
    """A union of random spheres (radii of several bricks): every component spans brick corners of both signs."""
    rng = np.random.default_rng(seed)
    res, B = (41, 33, 49), 4
    lo, step = mt.cube_grid(res)
    p = mt.grid_points(res, lo, step).astype(np.float64)
    s = np.full(len(p), -np.inf)
    for _ in range(4):
        c, r = rng.uniform(-0.5, 0.5, 3), rng.uniform(0.25, 0.4)
        s = np.maximum(s, r - np.linalg.norm(p - c, axis=1))
    g = s.astype(np.float32).reshape(res)
    _check_band_equals_dense(g, 0.0, lo, step, B)


def test_reference_growth_reaches_what_the_corners_miss():
    """A thin ring off the corner planes with one ball that holds a brick corner: the seeds sit at the ball, growth walks round the ring
    in several rounds."""
    res, B = (65, 65, 33), 8
    lo, step = mt.cube_grid(res)
    p = mt.grid_points(res, lo, step).astype(np.float64)
    ring = 0.06 - np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - 0.6) ** 2 + (p[:, 2] - 0.12) ** 2)
    ball = 0.15 - np.linalg.norm(p - np.array([0.5, 0.25, 0.0]), axis=1)
    g = np.maximum(ring, ball).astype(np.float32).reshape(res)
    active, seeded, rounds, v, f = _check_band_equals_dense(g, 0.0, lo, step, B)
    assert active.sum() > seeded.sum() > 0 and rounds >= 2, (active.sum(), seeded.sum(), rounds)
    assert mt.is_closed_oriented_manifold(f) and mt.signed_volume(v, f) > 0


def test_reference_misses_a_component_inside_one_brick():
    """The documented limitation: a small sphere strictly inside one brick, no brick corner inside it — nothing is seeded."""
    res, B = (33, 33, 33), 16
    lo, step = mt.cube_grid(res)
    p = mt.grid_points(res, lo, step).astype(np.float64)
    g = (0.2 - np.linalg.norm(p - 0.5, axis=1)).astype(np.float32).reshape(res)
    active, seeded, rounds = br.active_fixed_point(g, 0.0, B)
    assert not active.any() and rounds == 0
    v, f, ids = br.band_mesh(g, 0.0, lo, step, B, active)
    assert v.shape == (0, 3) and f.shape == (0, 3) and len(ids) == 0
    assert len(mt.marching_tets(g, 0.0, lo, step)[1]) > 100


def test_renumber_is_a_canonical_form():
    rng = np.random.default_rng(0)
    res, B = (17, 17, 17), 4
    lo, step = mt.cube_grid(res)
    g = mt.field("sphere", res, lo, step)
    v, f, ids = br.band_mesh(g, 0.0, lo, step, B, np.ones(br.bricks_per_axis(res, B), bool))
    perm = rng.permutation(len(v))                                    # any vertex order, any face order, any rotation
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    f2 = inv[f][rng.permutation(len(f))]
    f2 = np.roll(f2, 1, axis=1)
    a, b = br.renumber(v, f, ids), br.renumber(v[perm], f2, ids[perm])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    flipped = br.renumber(v, f[:, [0, 2, 1]], ids)[1]                 # orientation is kept
    assert not np.array_equal(flipped, a[1])
    assert math.isclose(mt.signed_volume(v, f), -mt.signed_volume(v, f[:, [0, 2, 1]]))

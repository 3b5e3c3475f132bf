"""The NumPy restatement of the occupancy grid (tests/occ_reference.py) against brute force, and the properties the renderer relies on.
No GPU: the kernels are compared with the restatement in tests/test_gpu_occ.py."""
import os

import numpy as np
import pytest

import occ_reference as occ
from mofanerf_amd import build, lib, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_cells(grid, threshold):
    nx, ny, nz = grid.shape
    out = np.zeros((nx - 1, ny - 1, nz - 1), dtype=bool)
    for i in range(nx - 1):
        for j in range(ny - 1):
            for k in range(nz - 1):
                out[i, j, k] = bool((grid[i:i + 2, j:j + 2, k:k + 2] > np.float32(threshold)).any())
    return out


def brute_dilate(cells, d):
    cx, cy, cz = cells.shape
    out = np.zeros_like(cells)
    for i in range(cx):
        for j in range(cy):
            for k in range(cz):
                out[i, j, k] = cells[max(0, i - d):i + d + 1, max(0, j - d):j + d + 1, max(0, k - d):k + d + 1].any()
    return out


def test_cells_and_dilation_equal_brute_force():
    rng = np.random.default_rng(3)
    g = rng.normal(size=(9, 7, 11)).astype(np.float32)
    g[2, 3, 4] = np.nan                                             # NaN is never above the threshold
    for thr in (-0.5, 1.2, 2.5):
        cells = occ.cells_from_grid(g, thr)
        assert np.array_equal(cells, brute_cells(g, thr))
        for d in (0, 1, 2, 3):
            assert np.array_equal(occ.dilate_cells(cells, d), brute_dilate(cells, d))
    sparse = rng.uniform(size=(8, 6, 9)) > 0.97
    assert 0 < sparse.sum() < 40
    step = sparse
    for d in (1, 2, 3, 4):
        step = occ.dilate_cells(step, 1)                            # dilation by d = d dilations by 1
        assert np.array_equal(occ.dilate_cells(sparse, d), step) and np.array_equal(step, brute_dilate(sparse, d))
    assert np.array_equal(occ.dilate_cells(sparse, 0), sparse)
    assert occ.dilate_cells(sparse, 20).all()                       # a distance beyond the grid: clipped, everything
    a, b = rng.normal(size=(5, 5, 5)).astype(np.float32), rng.normal(size=(5, 5, 5)).astype(np.float32)
    assert np.array_equal(occ.occupancy([a, b], 1.0, 1), occ.dilate_cells(occ.cells_from_grid(a, 1.0) | occ.cells_from_grid(b, 1.0), 1))


def test_a_ball_centred_on_a_lattice_point_keeps_every_sample_inside_it():
    """The claim: for the field f(p) = r^2 - |p - c|^2 with c ON a lattice point, |p_a - c_a| is monotone along every cell edge, so f on
    a cell is largest at one of its corners; hence at dilate = 0 every sample inside the bounds with f(p) > 0 lies in a cell with a
    corner sample above the threshold 0 and is kept.  (Samples are taken with |p - c| < r (1 - 1e-5) in float64, so that the float32
    rounding of the grid values does not decide.)  A ball that lies inside one cell shows why the lattice point matters."""
    n = (33, 29, 37)
    res, lo, step = mesh.grid_spec(((-4.0, -3.5, -4.5), (4.0, 3.5, 4.5)), n)
    assert np.array_equal(step, np.float32([0.25, 0.25, 0.25]))
    r = 2.3
    g = occ.ball_grid(n, lo, step, (0.0, 0.0, 0.0), r)
    cells = occ.occupancy(g, 0.0, 0)
    assert 0.02 < cells.mean() < 0.5
    rng = np.random.default_rng(11)
    o = rng.uniform(-5, 5, (4000, 3)).astype(np.float32)
    d = rng.normal(size=(4000, 3)).astype(np.float32)
    z = rng.uniform(0, 3, (4000, 8)).astype(np.float32)
    k = occ.kept(o, d, z, lo, step, n, cells)
    p = occ.points(o, d, z).astype(np.float64)
    inside_ball = np.linalg.norm(p, axis=-1) < r * (1 - 1e-5)
    assert inside_ball.sum() > 300 and k[inside_ball].all()
    assert (~k).sum() > 1000 and not k[np.linalg.norm(p, axis=-1) > r + 0.25 * np.sqrt(3) + 1e-4].any()    # at most one cell diagonal beyond
    tiny = occ.ball_grid(n, lo, step, (0.125, 0.125, 0.125), 0.1)   # a ball strictly inside one cell: no corner sees it
    assert not occ.occupancy(tiny, 0.0, 0).any()


def test_faces_are_inside_one_ulp_beyond_is_outside_and_nan_is_outside():
    """With lo = 0 and step = 0.25 the subtraction and the division are exact, so t = n - 1 exactly on the hi face and one ulp beyond
    it is above; with lo = 1 the point one ulp below lo gives an exact negative difference.  (For bounds whose arithmetic rounds, the
    kept flag is what the formula gives — the GPU test compares it bit for bit.)"""
    n = (33, 33, 33)
    res, lo, step = mesh.grid_spec(((0.0, 0.0, 0.0), (8.0, 8.0, 8.0)), n)
    cells = np.ones((32, 32, 32), dtype=bool)
    f = np.float32
    zero = np.zeros((1, 3), np.float32)
    z1 = np.ones(1, np.float32)

    def one(p, lo_=lo):
        return bool(occ.kept(np.asarray([p], np.float32), zero, z1, lo_, step, n, cells)[0, 0])      # d = 0: p = o exactly

    assert one([0, 0, 0]) and one([8, 8, 8]) and one([0, 8, 3.3]) and one([8, 0, 0])
    up = np.nextafter(f(8), f(np.inf))
    for a in range(3):
        p = [4.0, 4.0, 4.0]
        p[a] = up
        assert not one(p)
        p[a] = np.nan
        assert not one(p)
        p[a] = np.inf
        assert not one(p)
        p[a] = -0.25
        assert not one(p)
    lo1 = np.float32([1, 1, 1])
    below = np.nextafter(f(1), f(0))
    assert one([1, 1, 1], lo1) and one([9, 9, 9], lo1)
    for a in range(3):
        p = [5.0, 5.0, 5.0]
        p[a] = below
        assert not one(p, lo1)
    # the last cell takes the hi face: c = min(int(t), n - 2)
    only_last = np.zeros((32, 32, 32), dtype=bool)
    only_last[31, 31, 31] = True
    assert bool(occ.kept(np.float32([[8, 8, 8]]), zero, z1, lo, step, n, only_last)[0, 0])
    assert not bool(occ.kept(np.float32([[7.7, 8, 8]]), zero, z1, lo, step, n, only_last)[0, 0])


def test_the_occupancy_kernels_are_part_of_the_library_and_refuse_bad_arguments():
    """Without a GPU: the entry points exist, validate their arguments before any launch, and state their workspace."""
    import ctypes as C
    assert "mofa_occ.hip" in build.SOURCES
    L = lib.load()
    assert L.mofa_occ_workspace_bytes(0) == 0 and L.mofa_occ_workspace_bytes(2 ** 31) == 0
    n = 1000
    assert L.mofa_occ_workspace_bytes(n) >= n * 8 + 8
    assert L.mofa_occ_workspace_bytes(5_000_000) >= 5_000_000 * 8 + (5_000_000 // 2048 + 1) * 8
    f3 = (C.c_float * 3)(0.0, 0.0, 0.0)
    s3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    bad = (C.c_float * 3)(1.0, 0.0, 1.0)
    p = 256       # never dereferenced: every call below is refused before a launch
    assert L.mofa_occ_cells(p, 1, 4, 4, 0.0, 0, p, None) == -1 and b"lattice" in L.mofa_last_error()
    assert L.mofa_occ_cells(p, 4, 4, 4, float("nan"), 0, p, None) == -1 and b"threshold" in L.mofa_last_error()
    assert L.mofa_occ_dilate(p, 4, 4, 4, 9, 2 * p, 3 * p, None) == -1 and b"dilate" in L.mofa_last_error()
    assert L.mofa_occ_dilate(p, 4, 4, 4, -1, 2 * p, 3 * p, None) == -1
    assert L.mofa_occ_dilate(p, 4, 4, 4, 1, p, 3 * p, None) == -1 and b"aliased" in L.mofa_last_error()
    assert L.mofa_occ_classify(p, p, p, 0, 0, 4, p, 4, 4, 4, f3, s3, p, p, p, None) == -1
    assert L.mofa_occ_classify(p, p, p, 3, 8, 4, p, 4, 4, 4, f3, s3, p, p, p, None) == -1 and b"z_row_stride" in L.mofa_last_error()
    assert L.mofa_occ_classify(p, p, p, 0, 8, 4, p, 4, 4, 4, f3, bad, p, p, p, None) == -1 and b"step" in L.mofa_last_error()
    assert L.mofa_occ_classify(p, p, p, 0, 2 ** 30, 4, p, 4, 4, 4, f3, s3, p, p, p, None) == -1
    assert L.mofa_occ_gather(p, p, p, p, 0, 8, 4, p, p, 0, p, p, p, None) == -1 and b"n_kept" in L.mofa_last_error()
    assert L.mofa_occ_gather(p, p, p, p, 0, 8, 4, p, p, 33, p, p, p, None) == -1
    assert L.mofa_occ_scatter(None, p, p, 32, 1, p, None) == -1
    assert L.mofa_occ_scatter(p, p, p, 32, 33, p, None) == -1
    assert L.mofa_occ_scatter(p, p, p, 32, 4, p + 4, None) == -1 and b"aligned" in L.mofa_last_error()


def test_occupancy_argument_checks_need_no_gpu():
    from mofanerf_amd import occupancy
    import torch
    for d in (-1, 9, 1.5):
        with pytest.raises(lib.MofaError, match="dilate"):
            occupancy.occupancy_from_grid(torch.zeros(4, 4, 4), 0.0, (0, 0, 0), (1, 1, 1), dilate=d)
    for thr in (float("nan"), float("inf"), None):
        with pytest.raises(lib.MofaError, match="threshold"):
            occupancy.occupancy_from_grid(torch.zeros(4, 4, 4), thr, (0, 0, 0), (1, 1, 1))
    with pytest.raises(lib.MofaError, match="CPU"):
        occupancy.occupancy_from_grid(torch.zeros(4, 4, 4), 0.0, (0, 0, 0), (1, 1, 1))

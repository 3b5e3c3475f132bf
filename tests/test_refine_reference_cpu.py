"""The NumPy restatement of the vertex refinement (tests/refine_reference.py) checked against what it must obey, without a GPU: it
reproduces marching tetrahedra at 0 iterations, obeys the derived radial bound on the sharp ball, tells every injected fault from the
right arithmetic on the inputs the GPU tests use, and gives radial normals.  Plus the PLY round trip with normals and the argument
checks of the new entry points (no launch)."""
import ctypes as C

import numpy as np
import pytest

import mt_reference as mt
import refine_reference as rr
from mofanerf_amd import lib, mesh

LEVEL = 0.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def balls():
    """Per grid: the field, its lattice, the unrefined mesh and its edge ids (computed once, never changed)."""
    out = {}
    for res in rr.BALL_GRIDS:
        grid, lo, step = rr.ball_grid(res)
        verts, faces = mt.marching_tets(grid, LEVEL, lo, step)
        out[res] = dict(grid=grid, lo=lo, step=step, verts=verts, faces=faces, edge_ids=rr.iso_edge_ids(grid, LEVEL))
    return out


@pytest.mark.parametrize("res", rr.BALL_GRIDS)
def test_zero_iterations_reproduce_marching_tets_bit_for_bit(balls, res):
    b = balls[res]
    assert len(b["verts"]) > 1000 and len(b["edge_ids"]) == len(b["verts"]) and (np.diff(b["edge_ids"]) > 0).all()
    verts, (t_lo, t_hi, s_lo, s_hi), counts = rr.refine(rr.ball_np, b["edge_ids"], res, b["lo"], b["step"], LEVEL, 0)
    assert not counts.any()
    assert np.array_equal(bits(verts), bits(b["verts"]))
    assert (t_lo == 0).all() and (t_hi == 1).all()
    a, e, _ = rr.edge_ends(b["edge_ids"], res)                    # the ends' densities are the grid's, bit for bit
    assert np.array_equal(bits(s_lo), bits(b["grid"][a[:, 0], a[:, 1], a[:, 2]]))
    assert np.array_equal(bits(s_hi), bits(b["grid"][e[:, 0], e[:, 1], e[:, 2]]))


@pytest.mark.parametrize("res", rr.BALL_GRIDS)
@pytest.mark.parametrize("k", (1, 6, 20))
def test_refined_vertices_obey_the_radial_bound(balls, res, k):
    b = balls[res]
    verts, (t_lo, t_hi, s_lo, s_hi), counts = rr.refine(rr.ball_np, b["edge_ids"], res, b["lo"], b["step"], LEVEL, k)
    assert not counts.any()
    err, bound = rr.radial_error(verts), rr.radial_bound(b["edge_ids"], res, b["lo"], b["step"], k)
    print(f"{res} k={k}: max radial error {err.max():.3e}, max bound {bound.max():.3e}, worst error / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(t_hi - t_lo, np.full(len(verts), 2.0 ** -k, dtype=np.float32))
    assert (rr.inside(s_lo, LEVEL) != rr.inside(s_hi, LEVEL)).all()


@pytest.mark.parametrize("res", rr.BALL_GRIDS)
def test_the_unrefined_ball_misses_the_k6_bound_by_a_factor_of_four(balls, res):
    """What makes the GPU end-to-end test fail without the feature: linear interpolation of (R / r)^8 - 1 across a cell sits far off
    the sphere (measured: 22.5 and 23.5 times the largest k = 6 bound on the two grids)."""
    b = balls[res]
    bound = rr.radial_bound(b["edge_ids"], res, b["lo"], b["step"], 6)
    worst = rr.radial_error(b["verts"]).max()
    print(f"{res}: unrefined max radial error {worst:.3e} = {worst / bound.max():.1f} x the largest k = 6 bound {bound.max():.3e}")
    assert worst >= 4 * bound.max()


def _kernel_outputs(fault):
    """Everything the GPU tests compare bit for bit, computed by the restatement on their inputs, with one fault injected (or none)."""
    out = {}
    lo, step = rr.kernel_grid()
    n = rr.KERNEL_SIZES[-1]
    edges = rr.kernel_edges(n, 0)
    t_lo, t_hi, s_lo, s_hi, s_m = rr.kernel_brackets(n, 0, 0.25)
    counts = np.zeros(4, dtype=np.int64)
    for mode in range(3):
        out[f"points{mode}"] = rr.edge_points(rr.KERNEL_RES, lo, step, edges, t_lo, t_hi, rr.KERNEL_FIRST, n, mode,
                                              np.zeros((n, 3), dtype=np.float32), counts, fault)
    out["update"] = np.stack(rr.bracket_update(s_m, 0.25, t_lo, t_hi, s_lo, s_hi, counts, fault))
    out["place"] = rr.edge_place(rr.KERNEL_RES, lo, step, edges, t_lo, t_hi, s_lo, s_hi, 0.25, np.zeros((len(edges), 3), dtype=np.float32),
                                 counts, fault)
    for res in rr.BALL_GRIDS:
        grid, blo, bstep = rr.ball_grid(res)
        e = rr.iso_edge_ids(grid, LEVEL)
        verts, br, _ = rr.refine(rr.ball_np, e, res, blo, bstep, LEVEL, 6, fault)
        right = verts if fault is None else rr.refine(rr.ball_np, e, res, blo, bstep, LEVEL, 6)[0]
        out[f"ball{res}"] = verts
        out[f"bound{res}"] = rr.radial_error(verts) <= rr.radial_bound(e, res, blo, bstep, 6)
        out[f"normals{res}"] = rr.density_normals(rr.ball_np, right, bstep, fault=fault)[0]
    return out


@pytest.fixture(scope="module")
def right_outputs():
    return _kernel_outputs(None)


@pytest.mark.parametrize("fault", rr.FAULTS)
def test_every_injected_fault_breaks_a_comparison(right_outputs, fault):
    """t_m taken as t_lo, the update's sides swapped, p_b interpolated at t = 1, u clamped to [0, 1/2], the normal's sign flipped, h not
    scaled per axis: each changes bits (or breaks the radial bound) somewhere in what the GPU tests compare."""
    wrong = _kernel_outputs(fault)
    broken = [k for k in right_outputs if not np.array_equal(wrong[k].view(np.uint8), right_outputs[k].view(np.uint8))]
    print(fault, "->", broken)
    assert broken
    assert all(right_outputs[k].all() for k in right_outputs if k.startswith("bound"))


@pytest.mark.parametrize("res", rr.BALL_GRIDS)
def test_ball_normals_point_radially(balls, res):
    """Central differences at h = step / 2 on (R / r)^8 - 1 are not exactly radial (the three axes truncate differently).  Measured on
    the k = 6 meshes, largest angle to the radial direction of the float64 central difference: 0.05718 rad (17^3), 0.08697 rad
    (17 x 21 x 13) -> rr.FD_ANGLE_F64 = 0.0870; float32 restatement against that float64 direction: 1.30e-6, 1.48e-6 rad ->
    rr.FD_ANGLE_F32_SLACK = 1.5e-6.  The restatement (and the GPU) is allowed rr.NORMAL_TOL = 2 (0.0870 + 1.5e-6) rad."""
    b = balls[res]
    verts, _, _ = rr.refine(rr.ball_np, b["edge_ids"], res, b["lo"], b["step"], LEVEL, 6)
    c = np.array(rr.BALL_C, dtype=np.float64)
    radial = verts.astype(np.float64) - c
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    h = (np.float32(0.5) * b["step"]).astype(np.float32).astype(np.float64)
    p = np.repeat(verts.astype(np.float64)[:, None, :], 6, 1)
    for a in range(3):
        p[:, 2 * a, a] += h[a]
        p[:, 2 * a + 1, a] -= h[a]
    s = ((rr.BALL_R / np.linalg.norm(p.reshape(-1, 3) - c, axis=1)) ** 8 - 1).reshape(-1, 6)
    g = np.stack([(s[:, 2 * a] - s[:, 2 * a + 1]) / (2 * h[a]) for a in range(3)], 1)
    n64 = -g / np.linalg.norm(g, axis=1, keepdims=True)
    n32, counts = rr.density_normals(rr.ball_np, verts, b["step"])
    e64, slack, total = rr.angle(n64, radial).max(), rr.angle(n32, n64).max(), rr.angle(n32, radial).max()
    print(f"{res}: float64 central difference vs radial {e64:.5f} rad, float32 restatement vs float64 {slack:.3e} rad, vs radial {total:.5f} rad")
    assert not counts.any()
    assert e64 <= rr.FD_ANGLE_F64 and slack <= rr.FD_ANGLE_F32_SLACK and total <= rr.NORMAL_TOL
    assert np.abs(np.linalg.norm(n32.astype(np.float64), axis=1) - 1).max() <= 2 ** -23
    assert (np.einsum("ij,ij->i", n32, radial) > 0.99).all()         # outward: toward lower density


def test_zero_and_non_finite_gradients_give_zero_normals():
    s = np.array([[1, 1, 2, 2, 3, 3], [1, 0, np.nan, 0, 0, 0], [np.inf, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0]], dtype=np.float32)
    counts = np.zeros(4, dtype=np.int64)
    n = rr.fd_normals(s.reshape(-1), np.array([0.5, 0.25, 0.125], dtype=np.float32), counts)
    assert counts[rr.ZERO_NORMAL] == 3 and not n[:3].any() and np.array_equal(n[3], np.array([1, 0, 0], dtype=np.float32))


def test_ply_round_trips_with_and_without_normals(tmp_path):
    rng = np.random.default_rng(5)
    verts, normals, colors = rng.standard_normal((7, 3)).astype(np.float32), rng.standard_normal((7, 3)).astype(np.float32), rng.random((7, 3))
    faces = rng.integers(0, 7, (5, 3)).astype(np.int32)
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, verts, faces, colors, normals=normals)
    v, f, c, n = mesh.read_ply(path)
    assert np.array_equal(bits(v), bits(verts)) and np.array_equal(f, faces) and np.array_equal(c, mesh.to8b(colors))
    assert np.array_equal(bits(n), bits(normals))
    assert b"property float nx\nproperty float ny\nproperty float nz\n" in open(path, "rb").read(400)
    mesh.write_ply(path, verts, faces, normals=normals)
    v, f, c, n = mesh.read_ply(path)
    assert c is None and np.array_equal(bits(n), bits(normals)) and np.array_equal(bits(v), bits(verts))
    mesh.write_ply(path, verts, faces, colors)                        # a file without normals reads as before: three elements
    out = mesh.read_ply(path)
    assert len(out) == 3 and np.array_equal(bits(out[0]), bits(verts)) and np.array_equal(out[2], mesh.to8b(colors))
    assert len(mesh.read_ply(path)) == 3 and b"nx" not in open(path, "rb").read(300)
    with pytest.raises(ValueError, match="normals"):
        mesh.write_ply(path, verts, faces, normals=normals[:3])


def test_new_entry_points_refuse_bad_arguments_without_a_launch():
    L = lib.load()
    f3 = lambda *v: (C.c_float * 3)(*v)
    lo, step, one = f3(-1, -1, -1), f3(.1, .1, .1), 0x1000      # (a non-null address: every call below returns before it launches)
    assert L.mofa_edge_points(9, 9, 9, lo, step, one, None, None, 0, 4, 3, one, one, None) != 0
    assert b"mode" in L.mofa_last_error()
    assert L.mofa_edge_points(9, 9, 9, lo, step, one, None, None, 0, 4, 2, one, one, None) != 0      # the midpoint needs the bracket
    assert L.mofa_edge_points(9, 9, 9, lo, step, one, None, None, 0, 0, 0, one, one, None) != 0      # n = 0
    assert L.mofa_edge_points(9, 1, 9, lo, step, one, None, None, 0, 4, 0, one, one, None) != 0      # one sample on an axis
    assert L.mofa_edge_points(9, 9, 9, lo, f3(.1, 0, .1), one, None, None, 0, 4, 0, one, one, None) != 0
    assert L.mofa_edge_points(9, 9, 9, lo, step, one, None, None, 0, 4, 0, one, None, None) != 0     # no counters
    assert L.mofa_edge_bracket_init(one, one, float("nan"), 4, one, one, one, one, one, None) != 0
    assert b"level" in L.mofa_last_error()
    assert L.mofa_edge_bracket_update(None, 0.0, 4, one, one, one, one, one, None) != 0
    assert L.mofa_edge_place(9, 9, 9, lo, step, one, one, one, one, one, float("inf"), 4, one, one, None) != 0
    assert L.mofa_fd_points(one, f3(.1, -.1, .1), 0, 4, one, None) != 0
    assert L.mofa_fd_normals(one, f3(.1, .1, 0), 4, one, one, None) != 0
    assert L.mofa_iso_edge_ids(1, 9, 9, one, one, None) != 0
    for bad in (-1, 21, 1.5):
        with pytest.raises(lib.MofaError, match="iterations"):
            mesh.refine_vertices(None, None, (9, 9, 9), (-1, -1, -1), (.1, .1, .1), 0.0, bad, 100)

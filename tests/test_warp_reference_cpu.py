"""The non-rigid registration's NumPy restatement (tests/warp_reference.py) checked against things that share nothing with it — hand
arithmetic, a dense solve, properties of the minimiser, the surface distance of the warped template — and mesh.warp / mesh.warp_to's
refusals, all without a GPU.  tests/test_gpu_warp.py compares the GPU with the restatement bit for bit."""
import numpy as np
import pytest

import dist_reference as dist
import icp_reference as icp
import warp_reference as wr

SMALL = [name for name, _ in wr.SOLVER_MESHES]            # every solver case here has V <= 300
_warps = {}


def warped(scene, **kw):
    """warp_reference.warp on a catalogue scene, computed once per setting."""
    key = (scene,) + tuple(sorted(kw.items()))
    if key not in _warps:
        _warps[key] = wr.warp(*wr.scene(scene), **kw)
    return _warps[key]


def dense(D, adj, alpha):
    """A = D + alpha L (x) I3 as a [3V,3V] matrix, from the blocks and the lists (no code shared with wr.matvec)."""
    V = len(D)
    A = np.zeros((3 * V, 3 * V))
    cols = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    for i in range(V):
        for k in range(3):
            for l in range(3):
                A[3 * i + k, 3 * i + l] = D[i, cols[min(k, l), max(k, l)]]
        lst = adj["neighbours"][adj["offsets"][i]:adj["offsets"][i + 1]]
        for k in range(3):
            A[3 * i + k, 3 * i + k] += alpha * len(lst)
            for j in lst:
                A[3 * i + k, 3 * int(j) + k] -= alpha
    return A


def edge_energy(d, adj):
    """sum over the undirected edges of |d_i - d_j|^2"""
    total = 0.0
    for i in range(len(d)):
        for j in adj["neighbours"][adj["offsets"][i]:adj["offsets"][i + 1]]:
            if i < j:
                total += float(((d[i] - d[int(j)]) ** 2).sum())
    return total


# ---- exact values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", SMALL)
def test_without_stiffness_one_step_lands_on_the_targets(mesh):
    """stiffness = 0, the point metric, unit weights: A = I, so the first step has a == 1.0 exactly and the warped vertices are the targets
    bit for bit (c - v and v + (c - v) are exact in fp64 for fp32 inputs this close)."""
    verts, faces, targets, _, _ = wr.solver_case(mesh)
    adj = wr.adjacency(faces, len(verts))
    D, b, minv, _ = wr.system(verts, verts, targets, np.ones(len(verts)), adj, "point", 0.0)
    _, rec = wr.cg(D, b, minv, adj, 0.0, np.zeros((len(verts), 3)), 1, 1e-8)
    assert rec["a"] == 1.0 and rec["steps"] == 1
    out, d, solve = wr.warp_to(verts, faces, targets, stiffness=0.0, cg_iterations=1)
    assert dist._same(out, targets) and solve["steps"] == 1 and solve["stop"] == "iterations"
    assert np.array_equal(d, dist.widen(targets) - dist.widen(verts))


def test_three_vertex_system_by_hand():
    """One triangle, the plane metric, a handle on vertex 2 and a rejected vertex 1: every number from the formulas, in plain Python."""
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    targets = np.array([[0.5, 0, 1], [1, 0.25, 2], [0, 1, -0.5]], dtype=np.float32)
    normals = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8]], dtype=np.float32)
    weight, alpha, pw, beta = np.array([2.0, 0.0, 0.5]), 0.25, 0.125, 4.0
    hweight, hpos = np.array([0.0, 0.0, beta]), np.array([[0, 0, 0], [0, 0, 0], [0.5, 1, 0]], dtype=np.float32)
    adj = wr.adjacency(faces, 3)
    assert adj["neighbours"].tolist() == [1, 2, 0, 2, 0, 1]
    D, b, minv, e = wr.system(verts, verts, targets, weight, adj, "plane", alpha, pw, normals=normals, hweight=hweight, hpos=hpos)
    # vertex 0: n = z, u = (0.5, 0, 1), w = 2
    assert D[0].tolist() == [2 * pw, 0, 0, 2 * pw, 0, 2 * (1 + pw)] and b[0].tolist() == [2 * (pw * 0.5), 0.0, 2 * (1.0 + pw * 1.0)]
    assert e[0] == 2 * (1.0 + pw * 1.25) and minv[0].tolist() == [1 / (2 * pw + 0.5), 1 / (2 * pw + 0.5), 1 / (2 * (1 + pw) + 0.5)]
    # vertex 1: rejected, no handle: only the stiffness is left
    assert not D[1].any() and not b[1].any() and e[1] == 0 and minv[1].tolist() == [2.0, 2.0, 2.0]
    # vertex 2: n = (0.6, 0, 0.8) in float32, u = (0, 0, -0.5), w = 0.5, the handle adds beta I and beta (p - v) = (2, 0, 0)
    n0, n2 = float(np.float32(0.6)), float(np.float32(0.8))
    nu = n2 * -0.5
    assert D[2].tolist() == [0.5 * (n0 * n0 + pw) + beta, 0.0, 0.5 * (n0 * n2), 0.5 * pw + beta, 0.0, 0.5 * (n2 * n2 + pw) + beta]
    assert b[2].tolist() == [0.5 * (n0 * nu) + beta * 0.5, 0.0, 0.5 * (n2 * nu + pw * -0.5)]
    p = np.array([[1.0, 2.0, 3.0], [-1.0, 0.5, 0.25], [4.0, -2.0, 1.0]])
    q = wr.matvec(D, p, adj, alpha)
    assert q[1].tolist() == [alpha * (2 * -1.0 - 5.0), alpha * (2 * 0.5 - 0.0), alpha * (2 * 0.25 - 4.0)]
    assert q[0, 2] == 2 * (1 + pw) * 3.0 + alpha * (2 * 3.0 - 1.25)
    assert np.allclose(dense(D, adj, alpha) @ p.reshape(-1), q.reshape(-1), rtol=1e-15, atol=0)
    x, rec = wr.cg(D, b, minv, adj, alpha, np.zeros((3, 3)), 50, 1e-14)
    assert rec["stop"] == "tolerance" and np.allclose(x.reshape(-1), np.linalg.solve(dense(D, adj, alpha), b.reshape(-1)), rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("V", [1, 255, 1025, 2049])
def test_the_inner_product_is_the_written_order(V):
    rng = np.random.default_rng(V)
    a, b = rng.standard_normal((V, 3)) * 10.0 ** rng.integers(-8, 8, (V, 1)), rng.standard_normal((V, 3))
    rows = [float((a[i, 0] * b[i, 0] + a[i, 1] * b[i, 1]) + a[i, 2] * b[i, 2]) for i in range(V)]
    while True:
        sums = []
        for c0 in range(0, len(rows), 1024):
            part = [0.0] * 256
            for k in range(4):
                for t in range(256):
                    if c0 + t + 256 * k < len(rows):
                        part[t] += rows[c0 + t + 256 * k]
            w = 128
            while w >= 1:
                for t in range(w):
                    part[t] += part[t + w]
                w //= 2
            sums.append(part[0])
        rows = sums
        if len(rows) == 1:
            break
    assert wr.dot(a, b) == rows[0]
    if V > 1024:
        assert wr.dot(a, b, faults=("flat_sum",)) != rows[0]          # the order matters on these numbers


# ---- the solve is a solve ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("mesh", SMALL)
def test_the_solve_is_a_solve(mesh, metric):
    """|x - x*| <= |b - A x| / lambda_min(A) for a symmetric positive definite A (x - x* = A^-1 (A x - b)), plus the dense solve's own
    rounding, bounded by cond(A) eps |x*| times a small factor for the dimension.  Unknowns without a data term, a handle or a neighbour
    (a zero row: the restatement leaves them at the start) are not part of the system."""
    verts, faces, targets, weight, normals = wr.solver_case(mesh)
    V, alpha = len(verts), 0.7
    adj = wr.adjacency(faces, V)
    D, b, minv, _ = wr.system(verts, verts, targets, weight, adj, metric, alpha, 1e-2, normals=normals)
    x, rec = wr.cg(D, b, minv, adj, alpha, np.zeros((V, 3)), 2000, 1e-13)
    assert rec["stop"] == "tolerance", rec
    A, bb, xx = dense(D, adj, alpha), b.reshape(-1), x.reshape(-1)
    free = A.diagonal() > 0
    assert not xx[~free].any() and not A[~free].any() and not A[:, ~free].any()
    A, bb, xx = A[np.ix_(free, free)], bb[free], xx[free]
    lam = np.linalg.eigvalsh(A)
    assert lam[0] > 0
    star = np.linalg.solve(A, bb)
    bound = np.linalg.norm(bb - A @ xx) / lam[0] + 8 * len(bb) * np.finfo(np.float64).eps * (lam[-1] / lam[0]) * np.linalg.norm(star)
    print(mesh, metric, "steps", rec["steps"], "|x - x*|", np.linalg.norm(xx - star), "bound", bound)
    assert np.linalg.norm(xx - star) <= bound


def test_stiffness_does_what_it_says():
    """For the minimisers of E_data + alpha E_edge at alpha_1 < alpha_2, adding the two optimality inequalities gives
    (alpha_2 - alpha_1) (E_edge(d_1) - E_edge(d_2)) >= 0: the edge energy does not grow with the stiffness (checked at converged CG,
    with the rounding of the converged solves allowed for: a relative 1e-9)."""
    for mesh, metric in (("strip257", "point"), ("odd_mesh", "plane"), ("tetrahedron", "plane")):
        verts, faces, targets, weight, normals = wr.solver_case(mesh)
        adj = wr.adjacency(faces, len(verts))
        energies = []
        for alpha in (0.1, 1.0, 10.0):
            _, d, solve = wr.warp_to(verts, faces, targets, weight, normals, metric, alpha, cg_iterations=3000, cg_tol=1e-13)
            assert solve["stop"] == "tolerance"
            energies.append(edge_energy(d, adj))
        print(mesh, metric, energies)
        assert energies[0] * (1 + 1e-9) >= energies[1] and energies[1] * (1 + 1e-9) >= energies[2] and energies[0] > energies[2]


# ---- it warps ---------------------------------------------------------------------------------------------------------------------------
def surface_rms(verts, faces):
    """The verts -> patch rms surface distance at spacing 0.05 (the template's own computed once)."""
    key = ("surface", np.asarray(verts).tobytes())
    if key not in _warps:
        _warps[key] = dist.surface_distance(verts, faces, *icp.patch(), 0.05)["a_to_b"]["rms"]
    return _warps[key]


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_it_warps(metric):
    """The template -> target rms surface distance after warp's defaults is at most half of what it was (the cap carries a factor of two
    over a NumPy prototype's 0.25 / 0.28; the restatement gives 0.318 with the plane metric and 0.320 with the point metric, from 0.1041
    to 0.0331 / 0.0333).  Recorded, not asserted: the residual rms that the first and the last iteration of every level started from."""
    tv, tf, _, _ = wr.scene("patch")
    out = warped("patch", metric=metric)
    before, after = surface_rms(tv, tf), surface_rms(out["verts"], tf)
    levels = sorted({h["stiffness"] for h in out["history"]}, reverse=True)
    print(metric, "rms", before, "->", after, "ratio", after / before,
          "residual per level", [(a, [h["rms"] for h in out["history"] if h["stiffness"] == a][::4]) for a in levels])
    assert out["status"] == "iterations" and out["iterations"] == 15 and len(out["history"]) == 15
    assert after <= 0.5 * before


def test_the_border_rule():
    """Against the cropped patch the template overhangs the target (x > 0.4).  Without the rule the overhanging vertices are pulled onto the
    rim; with it they follow their neighbours.  Stated: who is rejected, the residuals; asserted: the overhanging part ends no further from
    the FULL patch with the rule than without it."""
    tv, tf, cv, cf = wr.scene("crop")
    pv, pf = icp.patch()
    over = dist.widen(tv)[:, 0] > 0.4 + 0.125                  # past the crop's last column of faces
    far = {}
    for rule in (True, False):
        out = warped("crop", reject_border=rule)
        last = out["history"][-1]
        res = dist.brute_force(out["verts"][over], pv, pf)
        far[rule] = float(np.sqrt(res["d2"].mean()))
        print("reject_border", rule, "rejected", last["rejected"], "used", last["used"], "residual rms", last["rms"], "overhang -> patch rms", far[rule])
        assert (last["rejected"]["border"] > 0) == rule and last["used"] + last["rejected"]["border"] == len(tv)
    assert int(over.sum()) >= 26 and far[True] <= far[False]


# ---- statuses, handles, init ------------------------------------------------------------------------------------------------------------
def test_statuses():
    tv, tf, pv, pf = wr.scene("patch")
    assert wr.warp(tv[:0], tf[:0], pv, pf)["status"] == "empty"
    out = wr.warp(tv, tf, pv, pf[:0])
    assert out["status"] == "no_correspondences" and out["iterations"] == 0 and dist._same(out["verts"], tv)
    flat = dist.square(4)                                       # the template hangs beside a flat square: every closest point is on its rim
    side = (tv * np.float32(0.25) + np.array([3.0, 0.5, 0.0], dtype=np.float32)).astype(np.float32)
    out = wr.warp(side, tf, *flat)
    assert out["status"] == "no_correspondences" and out["iterations"] == 0 and len(out["history"]) == 1
    assert out["history"][0]["used"] == 0 and out["history"][0]["rejected"]["border"] == len(tv) and not out["displacement"].any()
    out = wr.warp(side, tf, *flat, max_distance=0.5)
    assert out["status"] == "no_correspondences" and out["history"][0]["rejected"] == {"non_finite": 0, "beyond": len(tv), "border": 0}
    out = wr.warp(tv, tf, pv, pf, stiffness=(1.0,), iterations=4, tol=1.0)
    assert out["status"] == "converged" and out["iterations"] == 1
    assert warped("patch", metric="plane")["status"] == "iterations"
    # "singular": a first step without positive curvature although the residual is not zero.  A positive semi-definite system cannot
    # produce it in exact arithmetic (p = M^-1 r with r in A's range), so the record is shown on an indefinite D made by hand
    verts, faces, targets, weight, _ = wr.solver_case("tetrahedron")
    adj = wr.adjacency(faces, 4)
    D, b, minv, _ = wr.system(verts, verts, targets, weight, adj, "point", 0.0)
    x, rec = wr.cg(-D, b, minv, adj, 0.0, np.zeros((4, 3)), 5, 1e-8)
    assert rec["stop"] == "breakdown" and rec["steps"] == 0 and rec["rho"][0] > 0 and not x.any() and (rec["rho"] == rec["rho"][0]).all()


def test_handles_pull_their_vertices():
    """Row l of the normal equations, beta (y_l - p_l) = (b_data - D_data d)_l - alpha sum_j (d_l - d_j) + res_l with res = b - A d the
    solve's residual, bounds a handle's miss: |y_l - p_l| <= (|(b_data - D_data d)_l| + alpha sum_j |d_l - d_j| + |res_l|) / beta, plus the
    rounding of y to float32."""
    tv, tf, pv, pf = wr.scene("patch")
    index = np.array([0, 84, 168])
    pos = (dist.widen(tv)[index] + np.array([[0.0, 0.0, 0.3], [0.1, 0.0, -0.3], [0.0, -0.1, 0.2]])).astype(np.float32)
    beta, alpha = 50.0, 1.0
    kw = dict(metric="plane", stiffness=(alpha,), handles=(index, pos, beta))
    first = wr.warp(tv, tf, pv, pf, iterations=3, **kw)
    out = wr.warp(tv, tf, pv, pf, iterations=1, init=first["displacement"], **kw)
    free = wr.warp(tv, tf, pv, pf, iterations=4, metric="plane", stiffness=(alpha,))
    d, V = out["displacement"], len(tv)
    adj = wr.adjacency(tf, V)
    y0 = wr.apply(tv, first["displacement"])
    res = dist.brute_force(y0, pv, pf)
    fb, vb = icp.border_flags(pf, len(pv))
    w = np.where((res["face"] >= 0) & (icp.reject(res["face"], res["bary"], pf, fb, vb) == 0), 1.0, 0.0)
    hweight, hpos = wr.handle_arrays((index, pos, beta), V)
    Dd, bd, _, _ = wr.system(tv, y0, res["closest"], w, adj, "plane", alpha, face=res["face"], tverts=pv, tfaces=pf)
    D, b, _, _ = wr.system(tv, y0, res["closest"], w, adj, "plane", alpha, face=res["face"], tverts=pv, tfaces=pf, hweight=hweight, hpos=hpos)
    resid = b - wr.matvec(D, d, adj, alpha)
    data = bd - wr.matvec(Dd, d, adj, 0.0)
    y = dist.widen(out["verts"])
    for k, l in enumerate(index):
        lst = adj["neighbours"][adj["offsets"][l]:adj["offsets"][l + 1]]
        bound = (np.linalg.norm(data[l]) + alpha * sum(np.linalg.norm(d[l] - d[int(j)]) for j in lst) + np.linalg.norm(resid[l])) / beta
        miss, loose = np.linalg.norm(y[l] - dist.widen(pos)[k]), np.linalg.norm(dist.widen(free["verts"])[l] - dist.widen(pos)[k])
        print("handle", l, "miss", miss, "bound", bound, "without the handle", loose)
        assert miss <= bound + 2.0 ** -23 * np.abs(y[l]).max() * 2 and miss < 0.25 * loose


def test_an_init_is_taken_up():
    tv, tf, pv, pf = wr.scene("patch")
    first = warped("patch", metric="plane")
    again = wr.warp(tv, tf, pv, pf, iterations=0, init=first["displacement"])
    assert dist._same(again["verts"], first["verts"]) and dist._same(again["displacement"], first["displacement"]) and again["iterations"] == 0
    verts, faces, targets, weight, _ = wr.solver_case("strip257")
    _, d, cold = wr.warp_to(verts, faces, targets, weight, cg_iterations=40, cg_tol=0.0)
    _, d2, warm = wr.warp_to(verts, faces, targets, weight, init=d, cg_iterations=40, cg_tol=0.0)
    assert warm["rho"][0] < 1e-6 * cold["rho"][0] and cold["stop"] == warm["stop"] == "iterations"
    assert np.abs(d2 - d).max() < 1e-3 * np.abs(d).max()


# ---- every fault shows ------------------------------------------------------------------------------------------------------------------
def test_every_fault_changes_a_catalogue_case():
    tv, tf, pv, pf = wr.scene("patch")
    index = np.array([0, 84, 168])
    pos = (dist.widen(tv)[index] + np.array([0.0, 0.0, 0.3])).astype(np.float32)
    short = dict(stiffness=(1.0, 0.1), iterations=2)
    verts, faces, targets, weight, normals = wr.solver_case("odd_mesh")
    wide = wr.solver_case((__import__("smooth_reference").wide_fan()))
    shown = {}
    for fault in wr.FAULTS:
        if fault == "keep_border":
            got, want = (wr.warp(*wr.scene("crop"), faults=f, **short) for f in ((fault,), ()))
            shown[fault] = wr.mismatches(got, want)
        elif fault == "handles_no_rhs":
            got, want = (wr.warp(tv, tf, pv, pf, handles=(index, pos, 5.0), faults=f, **short) for f in ((fault,), ()))
            shown[fault] = wr.mismatches(got, want)
        elif fault == "no_warm_start":
            got, want = (wr.warp(tv, tf, pv, pf, cg_iterations=10, cg_tol=0.0, faults=f, **short) for f in ((fault,), ()))
            shown[fault] = wr.mismatches(got, want)
        elif fault == "reversed_order":                         # the order of a list shows where its sum rounds: heights that span 2^40
            got, want = (wr.warp_to(wide[0], wide[1], wide[2], wide[3], stiffness=3.0, cg_iterations=4, faults=f) for f in ((fault,), ()))
            shown[fault] = [] if dist._same(got[1], want[1]) else ["displacement"]
        elif fault == "freeze_not_sticky":                      # x survives a freeze that is forgotten; the search direction does not
            adj = wr.adjacency(faces, len(verts))
            D, b, minv, _ = wr.system(verts, verts, targets, weight, adj, "point", 1.0)
            got, want = (wr.cg(D, b, minv, adj, 1.0, np.zeros((len(verts), 3)), 60, 1e-3, faults=f)[1] for f in ((fault,), ()))
            assert want["stop"] == "tolerance" and want["steps"] < 59
            shown[fault] = [] if dist._same(got["p"], want["p"]) else ["p"]
        else:
            metric = "plane" if fault in ("unsymmetric", "no_point_weight") else "point"
            got, want = (wr.warp_to(verts, faces, targets, weight, normals, metric, 1.0, cg_iterations=12, cg_tol=0.0, faults=f) for f in ((fault,), ()))
            shown[fault] = ([] if dist._same(got[1], want[1]) else ["displacement"]) + wr.solve_mismatches(got[2], want[2])
    print(shown)
    assert all(shown[f] for f in wr.FAULTS), [f for f in wr.FAULTS if not shown[f]]


# ---- refusals without a GPU -------------------------------------------------------------------------------------------------------------
def test_the_library_validates_its_arguments_before_any_launch():
    from mofanerf_amd import lib
    L = lib.load()
    assert L.mofa_warp_apply(None, None, 1, None, None) == -1 and b"null pointer" in L.mofa_last_error()
    assert L.mofa_warp_apply(1, 1, 2 ** 31, 1, None) == -1 and b"V = 2147483648" in L.mofa_last_error()
    assert L.mofa_warp_dot(1, 1, 0, 1, None) == -1 and b"V = 0" in L.mofa_last_error()
    assert L.mofa_warp_matvec(1, 2, 1, 1, 1, 1, -1.0, 3, 1, 1, None) == -1 and b"alpha" in L.mofa_last_error()
    assert L.mofa_warp_matvec(1, 2, 1, 1, 1, 1, 1.0, 2, 1, 1, None) == -1 and b"in place" in L.mofa_last_error()
    assert L.mofa_warp_matvec(1, 2, 1, None, 1, 1, 1.0, 3, 1, 1, None) == -1 and b"null neighbours" in L.mofa_last_error()
    assert L.mofa_warp_solve(1, 1, 1, 1, 1, 1, 1, 1.0, 0, 1e-8, 1, 1, 1, 1, None) == -1 and b"cg_iterations" in L.mofa_last_error()
    assert L.mofa_warp_solve(1, 1, 1, 1, 1, 1, 1, 1.0, 10001, 1e-8, 1, 1, 1, 1, None) == -1 and b"cg_iterations" in L.mofa_last_error()
    assert L.mofa_warp_solve(1, 1, 1, 1, 1, 1, 1, 1.0, 5, 1.0, 1, 1, 1, 1, None) == -1 and b"cg_tol" in L.mofa_last_error()
    system = lambda normals, face, metric, pw, hw: L.mofa_warp_system(1, 1, 1, normals, face, 1, 1, 1, 1, 1, hw, None, 1, 0, 1, metric, pw, 1.0, 1, 1, 1, 1, 1, None)
    assert system(1, 1, 1, 0.01, None) == -1 and b"one of the two" in L.mofa_last_error()
    assert system(None, None, 1, 0.01, None) == -1 and b"one of the two" in L.mofa_last_error()
    assert system(None, None, 2, 0.01, None) == -1 and b"metric" in L.mofa_last_error()
    assert system(None, None, 0, -1.0, None) == -1 and b"point_weight" in L.mofa_last_error()
    assert system(None, None, 0, 0.01, 1) == -1 and b"come together" in L.mofa_last_error()
    assert L.mofa_warp_workspace_doubles(0) == 0 and L.mofa_warp_workspace_doubles(1025) == 12 * 1025 + 2 * (2 + 1)
    assert L.mofa_warp_workspace_doubles(1024 * 1024 + 1) == 12 * (1024 * 1024 + 1) + 2 * (1025 + 2 + 1)


def test_refusals_without_a_gpu():
    import torch
    from mofanerf_amd import lib, mesh
    tv, tf, pv, pf = (torch.from_numpy(np.ascontiguousarray(a)) for a in wr.scene("patch"))
    with pytest.raises(lib.MofaError, match="on the GPU"):
        mesh.warp(tv, tf, pv, pf)
    with pytest.raises(lib.MofaError, match="on the GPU"):
        mesh.warp_to(tv, tf, tv)
    for kw, match in ((dict(metric="colour"), "metric"), (dict(stiffness=()), "stiffness"), (dict(stiffness=(1.0, -0.1)), "stiffness"),
                      (dict(stiffness=(1.0, float("nan"))), "stiffness"), (dict(stiffness="stiff"), "stiffness"), (dict(point_weight=-1.0), "point_weight"),
                      (dict(cg_iterations=0), "cg_iterations"), (dict(cg_iterations=10001), "cg_iterations"), (dict(cg_iterations=2.5), "cg_iterations"),
                      (dict(cg_tol=1.0), "cg_tol"), (dict(cg_tol=-1e-3), "cg_tol"), (dict(iterations=-1), "iterations"), (dict(tol=-1.0), "tol"),
                      (dict(max_distance=0.0), "max_distance"), (dict(grid=0), "grid")):
        with pytest.raises(lib.MofaError, match=match):          # the scalar arguments are refused before any tensor is looked at
            mesh.warp(tv, tf, pv, pf, **kw)
    for kw, match in ((dict(metric="colour"), "metric"), (dict(stiffness=-1.0), "stiffness"), (dict(stiffness=(1.0, 2.0)), "one value"),
                      (dict(point_weight=float("inf")), "point_weight"), (dict(cg_iterations=True), "cg_iterations"), (dict(cg_tol=2.0), "cg_tol")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.warp_to(tv, tf, tv, **kw)

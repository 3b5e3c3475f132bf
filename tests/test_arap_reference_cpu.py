"""The as-rigid-as-possible stiffness's NumPy restatement (tests/arap_reference.py) checked against things that share nothing with it — exact
values, known rigid motions, the orthogonality of every output, numpy's eigen-solver, the two conditions the feature exists for — and
mesh.warp(stiffness_model=...) / mesh.deform's refusals, all without a GPU.  tests/test_gpu_arap.py compares the GPU with the restatement
bit for bit."""
import numpy as np
import pytest

import arap_reference as ar
import dist_reference as dist
import warp_reference as wr

CASES = list(ar.catalogue())
_memo = {}


def fitted(name):
    """(adjacency, R [V,9], fit [V], non-finite count) of a catalogue case, computed once."""
    if name not in _memo:
        verts, faces, d, _ = ar.catalogue()[name]
        adj = wr.adjacency(faces, len(verts))
        _memo[name] = (adj,) + ar.rotations(verts, d, adj)
    return _memo[name]


def edge_sums(verts, adj):
    """(sum_j |e_ij|^2 [V], the second singular value of the neighbourhood's edges over the first [V]) in plain loops."""
    v = dist.widen(verts)
    total, rank2 = np.zeros(len(v)), np.zeros(len(v))
    for i in range(len(v)):
        lst = adj["neighbours"][adj["offsets"][i]:adj["offsets"][i + 1]].astype(np.int64)
        if len(lst):
            e = v[i] - v[lst]
            total[i] = (e * e).sum()
            sv = np.linalg.svd(e, compute_uv=False)
            rank2[i] = sv[1] / sv[0] if len(sv) > 1 and sv[0] > 0 else 0.0
    return total, rank2


# ---- exact values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("rest/")])
def test_at_rest_the_rotations_are_the_identity_bit_for_bit(name):
    """d = 0: S is symmetric, row 0 of N is zero off the diagonal and never rotated, N_00 = tr S is the largest diagonal entry: R = I, fit = 0
    and g = 0 exactly, on every catalogue mesh (the one-edge strip and the vertex without neighbours included)."""
    verts, faces, d, _ = ar.catalogue()[name]
    adj, R, fit, odd = fitted(name)
    assert np.array_equal(R, np.tile(ar.IDENTITY, (len(verts), 1))) and not fit.any() and odd == 0
    g = ar.arap_g(verts, R, adj)
    b = np.random.default_rng(0).standard_normal((len(verts), 3))
    assert not g.any() and np.array_equal(ar.arap_rhs(verts, R, adj, 3.0, b), b)


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("rigid/")])
def test_an_exact_rigid_motion_is_recovered(name):
    """The rotation within 1e-12 wherever the neighbourhood determines it (two independent edges: second singular value > 1e-3 of the first)
    and fit <= 1e-24 sum |e|^2 everywhere, the flat mesh and the one-edge strip included."""
    verts, faces, d, truth = ar.catalogue()[name]
    adj, R, fit, odd = fitted(name)
    total, rank2 = edge_sums(verts, adj)
    determined = rank2 > 1e-3
    err = np.abs(R.reshape(-1, 3, 3) - truth).max((1, 2))
    print(name, "determined", int(determined.sum()), "of", len(verts), "max |R - truth|", err[determined].max() if determined.any() else None,
          "max fit / sum |e|^2", (fit[total > 0] / total[total > 0]).max())
    assert odd == 0 and (fit <= 1e-24 * total).all()
    assert (err[determined] <= 1e-12).all()
    if "strip2" not in name:
        assert determined.any()


@pytest.mark.parametrize("name", CASES)
def test_every_output_is_a_rotation(name):
    adj, R, fit, odd = fitted(name)
    R3 = R.reshape(-1, 3, 3)
    assert np.isfinite(R).all() and np.isfinite(fit).all() and (fit >= 0).all()
    assert np.abs(np.einsum("vji,vjk->vik", R3, R3) - np.eye(3)).max() <= 1e-14 and (np.linalg.det(R3) > 0).all()
    assert (odd > 0) == name.startswith("non_finite/")


def test_a_non_finite_displacement_gives_the_identity_and_is_counted():
    for name in (c for c in CASES if c.startswith("non_finite/")):
        verts, faces, d, _ = ar.catalogue()[name]
        adj, R, fit, odd = fitted(name)
        row = int(np.flatnonzero(~np.isfinite(d).all(1))[0])
        touched = [row] + adj["neighbours"][adj["offsets"][row]:adj["offsets"][row + 1]].tolist()
        assert odd == len(touched) and all(np.array_equal(R[i], ar.IDENTITY) and fit[i] == 0 for i in touched)
        clean = np.setdiff1d(np.arange(len(verts)), touched)
        want = ar.rotations(verts, np.where(np.isfinite(d), d, 0.0), adj)
        far = [i for i in clean if not set(adj["neighbours"][adj["offsets"][i]:adj["offsets"][i + 1]].tolist()) & set(touched)]
        assert np.array_equal(R[far], want[0][far])


@pytest.mark.parametrize("name", [c for c in CASES if c.split("/")[0] in ("noisy", "scaled", "mirrored")])
def test_the_rotation_is_the_maximiser(name):
    """Against numpy's eigen-solver on the same matrix: the quaternion's Rayleigh quotient reaches the largest eigenvalue within
    64 eps |N| (the Jacobi sweeps converged on the right eigenvalue)."""
    verts, faces, d, _ = ar.catalogue()[name]
    adj, R, _, _ = fitted(name)
    N = ar.horn(ar.covariance(dist.widen(verts), d, adj))
    q = np.stack([np.asarray(__import__("icp_reference").rotation_q(r)) for r in R.reshape(-1, 3, 3)])
    top = np.linalg.eigvalsh(N)[:, -1]
    rayleigh = np.einsum("vi,vij,vj->v", q, N, q)
    scale = np.abs(N).sum((1, 2))
    assert (top - rayleigh <= 64 * np.finfo(np.float64).eps * scale).all(), (top - rayleigh).max()


# ---- the sweep count --------------------------------------------------------------------------------------------------------------------
def test_the_shipped_sweep_count_has_two_in_hand():
    """After SWEEPS - 2 sweeps the off-diagonal norm of N is already <= 2^-50 of its norm on the whole catalogue; one sweep fewer is not
    enough (printed: the maximum after 1 .. SWEEPS sweeps)."""
    worst = np.zeros(ar.SWEEPS)
    for name in CASES:
        verts, faces, d, _ = ar.catalogue()[name]
        S = ar.covariance(dist.widen(verts), d, wr.adjacency(faces, len(verts)))
        N = ar.horn(np.where(np.isfinite(S).all((1, 2))[:, None, None], S, 0.0))
        for s in range(ar.SWEEPS):
            worst[s] = max(worst[s], ar.off_norm(ar.jacobi(N, s + 1)[0]).max())
    print("relative off-diagonal norm after 1 ..", ar.SWEEPS, "sweeps:", worst)
    assert ar.SWEEPS == 7 and worst[ar.SWEEPS - 3] <= 2.0 ** -50 and worst[ar.SWEEPS - 4] > 2.0 ** -50


# ---- the two conditions -----------------------------------------------------------------------------------------------------------------
def test_deform_takes_the_surface_along_rigidly():
    """The restatement at the defaults: 2.7e-4 from the rigid motion against 0.164 for warp_to (ratio 606), rotations within 6.3e-4."""
    verts, faces, handles, truth = ar.deform_scene("border")
    out = ar.deform(verts, faces, handles)
    assert out["status"] == "iterations" and out["iterations"] == 40 and out["history"][0]["arap_energy"] == 0.0
    assert ar.deform_condition(out, verts, faces, handles, truth, ar.warp_to_with_handles(verts, faces, handles, truth))


def test_with_few_handles_the_energy_only_falls():
    """Five handles: local/global converges slowly (6.3e-2 from the rigid motion after 40 iterations) — the honest record of the method's
    limit; asserted is only that arap_energy does not grow from one solve to the next."""
    verts, faces, handles, truth = ar.deform_scene("five")
    out = ar.deform(verts, faces, handles)
    energies = [h["arap_energy"] for h in out["history"]]
    print("five handles: max distance", float(np.linalg.norm(dist.widen(out["verts"]) - truth, axis=1).max()), "energy", energies[1], "->", energies[-1])
    assert energies[0] == 0.0 and all(b <= a for a, b in zip(energies[1:], energies[2:]))


def test_arap_keeps_the_edge_lengths_of_a_rotated_template():
    """The patch scene with the template rotated by 15 degrees, plane metric, default schedule: the restatement gives 0.0694 against 0.1316
    (ratio 0.53) and keeps 150 vertices against 123."""
    verts, faces, pv, pf = ar.rotated_template()
    results = {m: ar.warp(verts, faces, pv, pf, stiffness_model=m) for m in ("displacement", "arap")}
    assert not wr.mismatches(results["displacement"], wr.warp(verts, faces, pv, pf)) and "rotations" not in results["displacement"]
    assert all("arap_energy" in h for h in results["arap"]["history"]) and results["arap"]["history"][0]["arap_energy"] == 0.0
    assert ar.warp_condition(results, verts, faces)


# ---- every fault shows ------------------------------------------------------------------------------------------------------------------
def test_every_fault_changes_a_catalogue_result():
    shown = {}
    cat = ar.catalogue()
    for fault in ar.FAULTS:
        shown[fault] = []
        if fault in ("rest_pose_rotations", "moved_float32"):
            verts, faces, handles, _ = ar.deform_scene("five")
            got, want = (ar.deform(verts, faces, handles, iterations=3, faults=f) for f in ((fault,), ()))
            shown[fault] = ar.mismatches(got, want)
            continue
        if fault == "reversed_order":                           # the order of a list shows where its sums round: heights that span 2^40
            verts, faces, targets, _, _ = wr.solver_case(__import__("smooth_reference").wide_fan())
            cases = {"wide_fan": (verts, faces, dist.widen(targets) - dist.widen(verts), None)}
        else:
            cases = cat
        for name, (verts, faces, d, _) in cases.items():
            adj = wr.adjacency(faces, len(verts))
            want = ar.rotations(verts, d, adj)
            got = ar.rotations(verts, d, wr.adjacency(faces, len(verts), (fault,)) if fault == "reversed_order" else adj, (fault,))
            b = np.ones((len(verts), 3))
            rhs = [ar.arap_rhs(verts, want[0], adj, 0.5, b, f) for f in ((fault,), ())]
            if not (dist._same(got[0], want[0]) and dist._same(got[1], want[1]) and dist._same(rhs[0], rhs[1])):
                shown[fault].append(name)
    print({f: len(v) for f, v in shown.items()})
    assert all(shown[f] for f in ar.FAULTS), [f for f in ar.FAULTS if not shown[f]]
    assert any(n.startswith("rest/isolated") for n in shown["tie_highest_index"])      # all-equal diagonals: the tie goes to index 0


# ---- statuses and refusals without a GPU ------------------------------------------------------------------------------------------------
def test_statuses():
    verts, faces, handles, _ = ar.deform_scene("five")
    out = ar.deform(verts[:0], faces[:0], (np.zeros(0, dtype=np.int64), np.zeros((0, 3), dtype=np.float32), 1.0))
    assert out["status"] == "empty" and out["rotations"].shape == (0, 3, 3)
    out = ar.deform(verts, faces, handles, iterations=0)
    assert out["status"] == "iterations" and out["iterations"] == 0 and np.array_equal(out["verts"], verts)
    assert np.array_equal(out["rotations"], np.tile(np.eye(3), (81, 1, 1)))
    out = ar.deform(verts, faces, handles, iterations=5, tol=10.0)
    assert out["status"] == "converged" and out["iterations"] == 1 and len(out["history"]) == 1
    rest = (handles[0], verts[handles[0]], 1.0)                  # handles at rest: nothing moves, the energy stays 0 exactly
    out = ar.deform(verts, faces, rest, iterations=2)
    assert not out["displacement"].any() and all(h["arap_energy"] == 0.0 for h in out["history"])
    with pytest.raises(ValueError):
        ar.warp(*wr.scene("patch"), stiffness_model="rigid")


def test_the_library_validates_its_arguments_before_any_launch():
    from mofanerf_amd import lib
    L = lib.load()
    assert L.mofa_warp_rotations(None, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1 and b"null pointer" in L.mofa_last_error()
    assert L.mofa_warp_rotations(1, 1, 1, None, 1, 1, 1, 1, 1, None) == -1 and b"null neighbours" in L.mofa_last_error()
    assert L.mofa_warp_rotations(1, 1, 1, 1, 1, 0, 1, 1, 1, None) == -1 and b"V = 0" in L.mofa_last_error()
    assert L.mofa_warp_rotations(1, 1, 1, 1, 2 ** 31, 1, 1, 1, 1, None) == -1 and b"E = 2147483648" in L.mofa_last_error()
    assert L.mofa_warp_arap_rhs(1, 2, 1, 1, 1, 1, 1.0, None, 1, None) == -1 and b"null pointer" in L.mofa_last_error()
    assert L.mofa_warp_arap_rhs(1, 2, 1, 1, 1, 1, 1.0, 2, 1, None) == -1 and b"two buffers" in L.mofa_last_error()
    assert L.mofa_warp_arap_rhs(1, 2, 1, 1, 1, 1, -1.0, 3, 1, None) == -1 and b"alpha" in L.mofa_last_error()
    assert L.mofa_warp_arap_rhs(1, 2, 1, 1, 1, 1, float("nan"), 3, 1, None) == -1 and b"alpha" in L.mofa_last_error()


def test_refusals_without_a_gpu():
    import torch
    from mofanerf_amd import lib, mesh
    tv, tf, pv, pf = (torch.from_numpy(np.ascontiguousarray(a)) for a in wr.scene("patch"))
    handles = (torch.tensor([0, 5]), tv[:2].clone(), 1.0)
    with pytest.raises(lib.MofaError, match="stiffness_model"):  # refused before any tensor is looked at
        mesh.warp(tv, tf, pv, pf, stiffness_model="rigid")
    with pytest.raises(lib.MofaError, match="stiffness_model"):
        mesh.warp(None, None, None, None, stiffness_model=None)
    for model in ("displacement", "arap"):
        with pytest.raises(lib.MofaError, match="on the GPU"):
            mesh.warp(tv, tf, pv, pf, stiffness_model=model)
    with pytest.raises(lib.MofaError, match="on the GPU"):
        mesh.deform(tv, tf, handles)
    with pytest.raises(lib.MofaError, match="handles"):
        mesh.deform(tv, tf, None)
    for kw, match in ((dict(stiffness=-1.0), "stiffness"), (dict(stiffness=(1.0, 0.1)), "one value"), (dict(stiffness="stiff"), "stiffness"),
                      (dict(iterations=-1), "iterations"), (dict(iterations=2.5), "iterations"), (dict(tol=-1.0), "tol"), (dict(cg_iterations=0), "cg_iterations"),
                      (dict(cg_iterations=10001), "cg_iterations"), (dict(cg_tol=1.0), "cg_tol")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.deform(tv, tf, handles, **kw)

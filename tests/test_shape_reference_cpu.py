"""The NumPy restatement of the linear shape model (tests/shape_reference.py) on the CPU: exact hand cases, the Gram sum against math.fsum
within the bound its order implies, the Jacobi against numpy.linalg.eigh, the model's properties on a family of height fields, the
convergence of shape_fit, the statuses, every fault switch, and the host side of mofanerf_amd.mesh (the Jacobi, the Cholesky, the inverse
pose) against the restatement bit for bit.  The GPU tests (tests/test_gpu_shape.py) compare the kernels and the public calls with it."""
import math

import numpy as np
import pytest

import dist_reference as dist
import icp_reference as icp
import shape_reference as sr
from mofanerf_amd import lib, mesh

U = 2.0 ** -53
_fits = {}


def fit(name, **kw):
    """One shape_fit of the scene per configuration, shared by the tests that look at it."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _fits:
        faults = set(kw.pop("faults", ()))
        verts, faces = sr.target(cropped=name == "crop")
        if name == "moved":
            s, R, t = icp.known_transform(5.0, 1.0)
            verts = (s * (sr.widen(verts) @ R.T) + t).astype(np.float32)
        _fits[key] = sr.shape_fit(sr.model(), verts, faces, faults=faults, **kw)
    return _fits[key]


TRUTH = sr.member(sr.UNSEEN)


# ---- exact hand cases -------------------------------------------------------------------------------------------------------------------
def test_two_meshes_give_one_mode_along_their_difference():
    a = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    b = a + np.array([[0, 0, 2], [0, 0, 0], [0, 4, 0]], dtype=np.float32)
    m = sr.shape_model(np.stack([a, b]))
    diff = (sr.widen(b) - sr.widen(a)).reshape(-1)
    assert m["modes"].shape == (1, 3, 3) and m["status"] == "ok" and m["n_meshes"] == 2
    assert abs(m["sigma"][0] - np.linalg.norm(diff) / math.sqrt(2.0)) <= 4 * U * m["sigma"][0]
    mode, c = m["modes"].reshape(-1), m["coeffs"][:, 0]
    assert np.abs(np.abs(mode) - np.abs(diff) / math.sqrt(2.0)).max() <= 1e-15 * np.abs(diff).max()       # sigma * unit(diff) = diff / sqrt(2)
    assert c[0] == -c[1] and abs(abs(c[0]) - 1 / math.sqrt(2.0)) <= 1e-15
    assert np.abs(sr.shape_synthesize(m, m["coeffs"]) - sr.widen(np.stack([a, b]))).max() <= 1e-15
    assert np.array_equal(m["mean"], (sr.widen(a) + sr.widen(b)) / 2)
    assert abs(m["explained"][0] - 1.0) <= 1e-15


def test_three_collinear_meshes_give_one_mode():
    a = sr.member(np.array([0.5, 0.2, -0.1]), 5)
    d = np.zeros_like(a)
    d[:, 2] = np.linspace(0.25, 1.0, len(a)).astype(np.float32)
    m = sr.shape_model(np.stack([a, a + d, a + 3 * d]).astype(np.float32))
    assert m["modes"].shape[0] == 1 and m["eigenvalues"][1] <= 1e-14 * m["eigenvalues"][0]


# ---- the Gram sum -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,group,weighted", [(1, 1, False), (257, 1, True), (1023 * 3, 3, True), (2049, 1, False), (1024 * 3 + 3, 3, True)])
def test_gram_lies_within_the_bound_of_its_order_of_math_fsum(N, group, weighted):
    """A term is one product (one rounding) times, with weights, one more; a number then passes through at most 3 additions of its thread
    (the first, to 0.0, is exact) and the 8 of the tree on every level of the sum: d = 1 (+ 1) + 11 levels roundings in all, so
    |sum - exact| <= gamma_d sum |exact terms|, gamma_d = d u / (1 - d u) (Higham, Accuracy and Stability, 4.4); fsum itself adds u |sum|."""
    rng = np.random.default_rng(N)
    R = 4
    P = rng.normal(size=(R, N)) * 10.0 ** rng.integers(-3, 4, size=(R, 1))
    w = rng.uniform(0.0, 2.0, N // group) * (rng.uniform(size=N // group) > 0.2) if weighted else None
    got = sr.gram(P, w, group)
    levels, m = 0, N
    while True:
        m, levels = (m + 1023) // 1024, levels + 1
        if m == 1:
            break
    d = (2 if weighted else 1) + 11 * levels
    gamma = d * U / (1 - d * U)
    wj = np.ones(N) if w is None else w[np.arange(N) // group]
    for k, (a, b) in enumerate(sr.pair_index(R)):
        from fractions import Fraction
        terms = [Fraction(float(wj[j])) * Fraction(float(P[a, j])) * Fraction(float(P[b, j])) for j in range(N)]
        exact, mag = sum(terms), sum(abs(t) for t in terms)
        assert abs(Fraction(float(got[k])) - exact) <= Fraction(gamma) * mag
        assert abs(got[k] - math.fsum(float(t) for t in terms)) <= float(Fraction(gamma) * mag) + 2 * U * float(mag)


def test_gram_ignores_what_a_column_of_weight_zero_holds():
    rng = np.random.default_rng(3)
    P = rng.normal(size=(3, 600))
    w = rng.uniform(0.5, 1.5, 200)
    w[[0, 57, 199]] = 0.0
    Q = P.copy()
    Q[:, 0:3], Q[1, 57 * 3 + 1], Q[2, 199 * 3] = np.nan, np.inf, -np.inf
    assert dist._same(sr.gram(Q, w, 3), sr.gram(P, w, 3)) and np.isfinite(sr.gram(Q, w, 3)).all()
    assert not np.isfinite(sr.gram(Q, w, 3, faults={"keep_rejected"})).all()
    w[5] = np.nan                                                      # `w > 0` is false for NaN too
    assert np.isfinite(sr.gram(P, w, 3)).all()


def test_gram_faults_change_bits():
    rng = np.random.default_rng(4)
    P, w = rng.normal(size=(3, 3 * 1500)), rng.uniform(0.5, 1.5, 1500)
    want = sr.gram(P, w, 3)
    for f in ("chunk_reversed", "weight_first", "group_ignored", "flat_sum"):
        assert not dist._same(sr.gram(P, w, 3, faults={f}), want), f
    assert dist._same(sr.gram_matrix(want, 3), sr.gram_matrix(want, 3).T) and sr.gram_matrix(want, 3)[0, 2] == want[2]


def test_centre_combine_and_plane_rows_by_hand():
    meshes = np.array([[[1, 2, 3]], [[2, 2, 5]], [[6, 2, 1]]], dtype=np.float32)
    mean, X = sr.centre(meshes)
    assert np.array_equal(mean, [3.0, 2.0, 3.0]) and np.array_equal(X[2], [3.0, 0.0, -2.0])
    out = sr.combine(np.array([1.0, 1.0, 1.0]), np.array([[2.0, -1.0]]), np.array([[1.0, 0.0, 2.0], [0.0, 3.0, 1.0]]))
    assert np.array_equal(out, [[3.0, -2.0, 4.0]])
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2]], dtype=np.float32)
    faces = np.array([[0, 1, 2], [0, 0, 1], [0, 1, 9]], dtype=np.int32)
    moved = np.array([[0.2, 0.2, 0.5]] * 4, dtype=np.float32)
    closest = np.array([[0.2, 0.2, 0.0]] * 4, dtype=np.float32)
    modes = np.arange(12, dtype=np.float64).reshape(1, 4, 3)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    P = sr.plane_rows(moved, closest, [0, 1, 2, 7], verts, faces, 2.0, Rz, modes)
    assert np.array_equal(P[:, 0], [2.0 * 2.0, 0.5]) and np.isnan(P[:, 1:]).all()          # degenerate, bad vertex, bad face
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])                     # R^T n = (0, 1, 0) for n = e_z
    assert sr.plane_rows(moved, closest, [0] * 4, verts, faces, 1.0, Rx, modes)[0, 0] == 1.0
    assert sr.plane_rows(moved, closest, [0] * 4, verts, faces, 1.0, Rx, modes, faults={"normal_not_rotated"})[0, 0] == 2.0


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rank", [(2, 2), (8, 3), (24, 24), (40, 12)])
def test_jacobi_equals_eigh(n, rank):
    """eigh's own backward error is a few u |G|: the eigenvalues (those at rounding level included) are compared relative to the largest, and
    on the full-rank matrices each one relative to itself as well."""
    rng = np.random.default_rng(n)
    X = rng.normal(size=(n, rank)) @ rng.normal(size=(rank, 300))
    G = X @ X.T
    lam, W, sweeps = sr.jacobi(G)
    ref, V = np.linalg.eigh(G)
    ref, V = ref[::-1], V[:, ::-1]
    assert sweeps < 12 and (np.diff(lam) <= 0).all()
    assert np.abs(lam - ref).max() <= 1e-12 * ref[0]
    if rank >= n:                                  # full rank: every eigenvalue to its own size (a null space has no relative accuracy)
        assert (np.abs(lam - ref) <= 1e-12 * ref).all()
    assert np.abs(W.T @ W - np.eye(n)).max() <= 1e-13
    for k in range(min(rank, n)):
        v = V[:, k] * (1.0 if V[np.argmax(np.abs(V[:, k])), k] > 0 else -1.0)
        assert W[np.argmax(np.abs(W[:, k])), k] > 0
        gap = min(abs(ref[k] - ref[j]) for j in range(n) if j != k) / ref[0]
        assert np.abs(W[:, k] - v).max() <= 1e-13 / gap
    assert np.abs(G @ W - W * lam).max() <= 1e-12 * ref[0]
    unsorted = sr.jacobi(G, faults={"unsorted"})[0]
    assert n == 2 or (np.diff(unsorted) > 0).any()
    assert any((sr.jacobi(G, faults={"no_sign_rule"})[1][:, k] != W[:, k]).any() for k in range(n)) or n == 2


def test_jacobi_orders_equal_eigenvalues_by_index_and_keeps_a_diagonal_matrix():
    lam, W, sweeps = sr.jacobi(np.diag([2.0, 5.0, 2.0, 7.0]))
    assert lam.tolist() == [7.0, 5.0, 2.0, 2.0] and sweeps == 1
    assert np.array_equal(W, np.eye(4)[:, [3, 1, 0, 2]])


def test_cholesky_solves_and_refuses():
    rng = np.random.default_rng(5)
    B = rng.normal(size=(9, 30))
    A, rhs = B @ B.T, rng.normal(size=9)
    x = sr.cholesky_solve(A, rhs, 0.25)
    assert np.abs((A + 0.25 * np.eye(9)) @ x - rhs).max() <= 1e-12 * np.abs(rhs).max() * np.linalg.cond(A)
    twice = np.array([[2.0, 2.0], [2.0, 2.0]])
    assert sr.cholesky_solve(twice, np.ones(2)) is None and sr.cholesky_solve(twice, np.ones(2), 1e-3) is not None
    assert sr.cholesky_solve(np.zeros((1, 1)), np.ones(1)) is None and sr.cholesky_solve(np.array([[np.nan]]), np.ones(1)) is None
    assert sr.cholesky_solve(np.zeros((0, 0)), np.zeros(0)).shape == (0,)


def test_the_products_host_side_is_the_restatements_bit_for_bit():
    rng = np.random.default_rng(6)
    for n, rank in ((2, 2), (8, 3), (19, 19), (33, 7)):
        X = rng.normal(size=(n, rank)) @ rng.normal(size=(rank, 200))
        G = X @ X.T
        got, want = mesh._shape_jacobi(G), sr.jacobi(G)
        assert dist._same(got[0], want[0]) and dist._same(got[1], want[1]) and got[2] == want[2]
        lam = 0.0 if n % 2 else 0.125
        rhs = rng.normal(size=n)
        a, b = mesh._shape_solve(G + np.eye(n), rhs, lam), sr.cholesky_solve(G + np.eye(n), rhs, lam)
        assert dist._same(a, b)
        sums = G[np.triu_indices(n)]
        assert dist._same(mesh._shape_matrix(sums, n), sr.gram_matrix(sums, n))
        c = rng.normal(size=n - 1)
        (dc, e), (dc2, e2) = mesh._shape_step(sums + 1.0, n - 1, c, lam), sr._normal_step(sums + 1.0, n - 1, c, lam)
        assert e == e2 and ((dc is None and dc2 is None) or dist._same(dc, dc2))
    assert mesh._shape_solve(np.array([[2.0, 2.0], [2.0, 2.0]]), np.ones(2), 0.0) is None
    s, R, t = icp.known_transform(20.0, 1.3)
    q = icp.rotation_q(R)
    T = mesh._shape_inverse((s, tuple(float(v) for v in q), tuple(float(v) for v in t)))
    si, Ri, ti = sr.inverse_transform(s, icp.q_rotation(q), t)
    assert dist._same(np.array(list(T)), np.concatenate([[si], Ri.reshape(-1), ti]))
    back = icp.apply(icp.apply(TRUTH, s, icp.q_rotation(q), t), si, Ri, ti)
    assert np.abs(sr.widen(back) - sr.widen(TRUTH)).max() < 1e-6


# ---- the model on the scene -------------------------------------------------------------------------------------------------------------
def test_model_finds_three_modes_among_eight_examples():
    m = sr.model()
    rel = m["eigenvalues"] / m["eigenvalues"][0]
    assert m["modes"].shape == (3, 169, 3) and m["status"] == "ok" and m["n_meshes"] == 8
    assert rel[2] > 0.1 and abs(rel[3]) < 1e-13                     # rank_tol = 1e-10 has ten orders of margin each way
    flat = m["modes"].reshape(3, -1)
    gram = flat @ flat.T
    assert np.abs(gram - np.diag(np.diag(gram))).max() <= 1e-13 * gram.max()                        # mutually orthogonal
    assert np.abs(np.sqrt(np.diag(gram)) - m["sigma"]).max() <= 1e-14                                # a mode is sigma times a unit vector
    assert np.abs((m["coeffs"] ** 2).sum(0) / 7.0 - 1.0).max() <= 1e-13                              # unit sample variance
    assert np.abs(m["coeffs"].sum(0)).max() <= 1e-12
    back = sr.shape_synthesize(m, m["coeffs"])
    assert np.abs(back - sr.widen(sr.family())).max() <= 1e-7       # the training meshes, up to their float32 rounding (6e-8 |z|), which no mode spans
    assert abs(m["explained"].sum() - 1.0) <= 1e-13 and (np.diff(m["explained"]) < 0).all()
    assert sr.shape_synthesize(m, m["coeffs"][:2], np.float32).dtype == np.float32
    assert sr.shape_model(sr.family(), components=2)["modes"].shape[0] == 2 and sr.shape_model(sr.family(), components=99)["modes"].shape[0] == 7
    assert sr.shape_model(sr.family(), rank_tol=0.5)["modes"].shape[0] == 2


def test_model_faults_are_seen():
    want = sr.model()
    assert "sigma" in sr.mismatches(sr.shape_model(sr.family(), faults={"m_not_m1"}), want)
    assert "eigenvalues" in sr.mismatches(sr.shape_model(sr.family(), faults={"unsorted"}), want)
    assert "modes" in sr.mismatches(sr.shape_model(sr.family(), faults={"no_sign_rule"}), want)
    assert "modes" in sr.mismatches(sr.shape_model(sr.family(), faults={"flat_sum"}), want)
    assert sr.mismatches(sr.shape_model(sr.family()), want) == []


def test_aligned_model_takes_out_a_rigid_motion():
    fam = sr.family()
    moved = fam.copy()
    for m in range(1, 8):
        s, R, t = icp.known_transform(2.0 * m, 1.0)
        moved[m] = (sr.widen(fam[m]) @ R.T + 0.3 * t).astype(np.float32)
    plain, aligned = sr.shape_model(moved), sr.shape_model(moved, align="rigid")
    assert aligned["transforms"].shape == (8, 4, 4) and "transforms" not in plain
    assert aligned["eigenvalues"][:3].sum() < 0.5 * plain["eigenvalues"][:3].sum()
    assert aligned["eigenvalues"][3] < 0.02 * aligned["eigenvalues"][0] < plain["eigenvalues"][3]


def test_project_returns_an_unseen_members_coefficients():
    m = sr.model()
    res = sr.shape_project(m, TRUTH)
    assert res["status"] == "ok" and res["rms"] < 1e-7 and sr.rms_error(res["verts"], TRUTH) < 1e-7
    few = np.zeros(169)
    few[[0, 12, 84, 100, 156, 168, 40, 130]] = 1.0
    noisy = TRUTH.copy()
    noisy[few == 0] = np.nan                                           # only the landmarks are looked at
    assert np.abs(sr.shape_project(m, noisy, weight=few)["coeffs"] - res["coeffs"]).max() < 1e-3      # (8 landmarks: the float32 noise, amplified)
    norms = [float(np.linalg.norm(sr.shape_project(m, TRUTH, regularize=lam)["coeffs"])) for lam in (0.0, 1.0, 10.0, 100.0, 1e4)]
    assert all(a > b for a, b in zip(norms, norms[1:])) and norms[-1] < 0.01 * norms[0]
    assert sr.shape_project(m, TRUTH, components=2)["coeffs"].shape == (2,)
    assert sr.shape_project(m, TRUTH, weight=np.zeros(169))["status"] == "empty"
    twice = dict(m, modes=np.concatenate([m["modes"], m["modes"][:1]]))
    res = sr.shape_project(twice, TRUTH)
    assert res["status"] == "singular" and not res["coeffs"].any()
    assert sr.shape_project(twice, TRUTH, regularize=1e-3)["status"] == "ok"


# ---- shape_fit --------------------------------------------------------------------------------------------------------------------------
def test_fit_plane_metric_lands_on_the_unseen_member():
    """Measured with this restatement: the mean is 0.026 rms from the truth; the plane metric ends 4.5e-9 from it after ONE iteration and
    3.8e-9 after three (148 of 169 vertices used in the first, 123 after: the border rule), the float32 moved points being the limit.
    Required: < 1e-6 after three."""
    assert 0.02 < sr.rms_error(sr.model()["mean"], TRUTH) < 0.03
    one, three = fit("full", iterations=1), fit("full", iterations=3)
    assert sr.rms_error(one["model_verts"], TRUTH) < 1e-6 and sr.rms_error(three["model_verts"], TRUTH) < 1e-6
    assert three["status"] == "iterations" and three["iterations"] == 3 and three["history"][0]["pose"] is None
    assert all(100 <= h["shape"]["used"] < 169 and h["shape"]["rejected"]["border"] > 0 for h in three["history"])
    assert three["history"][2]["shape"]["rms"] < 1e-7 and three["history"][2]["shape"]["step"] < 1e-6
    assert np.array_equal(three["verts"], three["model_verts"].astype(np.float32)) and three["scale"] == 1.0


def test_fit_on_the_cropped_target_shows_the_border_rule():
    """Cropped to centroids x < 0.4: 102 and then 89 vertices used (148 / 123 on the whole target), the same 3.9e-9 after three."""
    full, crop = fit("full", iterations=3), fit("crop", iterations=3)
    assert sr.rms_error(crop["model_verts"], TRUTH) < 1e-6
    assert all(c["shape"]["used"] < f["shape"]["used"] for c, f in zip(crop["history"], full["history"]))
    kept = fit("crop", iterations=3, faults=("kept_border",))
    assert kept["history"][0]["shape"]["used"] > crop["history"][0]["shape"]["used"]
    assert sr.rms_error(kept["model_verts"], TRUTH) > 100 * sr.rms_error(crop["model_verts"], TRUTH)
    off = fit("crop", iterations=3, reject_border=False)
    assert off["history"][0]["shape"]["rejected"]["border"] == 0 and off["history"][0]["shape"]["used"] == kept["history"][0]["shape"]["used"]


def test_fit_point_metric_is_slower_than_the_plane_metric():
    """Measured: 1.3e-3 after three iterations and 3.7e-5 after ten, contracting about 0.6 x per iteration, against 3.8e-9 after three for
    the plane metric: a vertex's closest point is not its partner until the shapes agree, and the plane metric lets it slide."""
    p3, p10 = fit("full", iterations=3, metric="point"), fit("full", iterations=10, metric="point")
    e3, e10 = sr.rms_error(p3["model_verts"], TRUTH), sr.rms_error(p10["model_verts"], TRUTH)
    assert e10 < 0.1 * e3 < 0.1 * sr.rms_error(sr.model()["mean"], TRUTH)
    assert e3 > 1000 * sr.rms_error(fit("full", iterations=3)["model_verts"], TRUTH)
    steps = [h["shape"]["step"] for h in p10["history"]]
    assert all(b < a for a, b in zip(steps, steps[1:]))


def test_fit_with_a_rigid_pose_recovers_a_moved_target():
    """The target moved by known_transform(5 deg, 1): 1.8e-7 rms from the moved truth after 15 iterations (about 0.45 x per iteration).
    Required: < 1e-5."""
    res = fit("moved", iterations=15, pose="rigid")
    s, R, t = icp.known_transform(5.0, 1.0)
    truth = (s * (sr.widen(TRUTH) @ R.T) + t).astype(np.float32)
    assert sr.rms_error(res["verts"], truth) < 1e-5 and sr.rms_error(res["model_verts"], TRUTH) < 1e-4
    assert np.abs(res["rotation"] - R).max() < 1e-4 and res["history"][0]["pose"]["used"] > 100
    bad = fit("moved", iterations=15, pose="rigid", faults=("normal_not_rotated",))
    assert "coeffs" in sr.mismatches(bad, res) and bad["history"][1]["shape"]["step"] != res["history"][1]["shape"]["step"]
    assert fit("moved", iterations=2, pose="similarity")["scale"] != 1.0


def test_fit_regulariser_and_its_fault():
    plain, reg = fit("full", iterations=2), fit("full", iterations=2, regularize=0.05)
    assert np.linalg.norm(reg["coeffs"]) < np.linalg.norm(plain["coeffs"])
    assert "coeffs" in sr.mismatches(fit("full", iterations=2, regularize=0.05, faults=("no_lambda_c",)), reg)
    assert "coeffs" in sr.mismatches(fit("full", iterations=2, faults=("keep_rejected",)), plain)
    assert sr.mismatches(sr.shape_fit(sr.model(), *sr.target(), iterations=2), plain) == []


def test_fit_statuses():
    m = sr.model()
    verts, faces = sr.target()
    assert fit("full", iterations=6, tol=1e-6)["status"] == "converged" and fit("full", iterations=6, tol=1e-6)["iterations"] < 6
    twice = dict(m, modes=np.concatenate([m["modes"], m["modes"][:1]]))
    res = sr.shape_fit(twice, verts, faces, iterations=3)
    assert res["status"] == "singular" and res["iterations"] == 0 and not res["coeffs"].any()
    res = sr.shape_fit(m, verts, faces, iterations=3, max_distance=1e-6)
    assert res["status"] == "no_correspondences" and "beyond" in res["history"][0]["shape"]["rejected"]
    assert sr.shape_fit(m, verts, faces[:0], iterations=3)["status"] == "no_correspondences"
    empty = {k: (v[:0] if k == "mean" else v[:, :0] if k == "modes" else v) for k, v in m.items()}
    assert sr.shape_fit(empty, verts, faces)["status"] == "empty"
    assert sr.shape_fit(m, verts, faces, iterations=1, components=2)["coeffs"].shape == (2,)
    start = sr.shape_fit(m, verts, faces, iterations=1, init_coeffs=fit("full", iterations=3)["coeffs"])
    assert start["history"][0]["shape"]["step"] < 1e-6


# ---- refusals need no GPU ---------------------------------------------------------------------------------------------------------------
def test_public_calls_refuse_cpu_tensors():
    import torch
    with pytest.raises(lib.MofaError):
        mesh.shape_model(torch.zeros(3, 4, 3))
    with pytest.raises(lib.MofaError):
        mesh.shape_synthesize({"mean": torch.zeros(4, 3, dtype=torch.float64), "modes": torch.zeros(1, 4, 3, dtype=torch.float64)}, [[0.0]])
    with pytest.raises(lib.MofaError):
        mesh.shape_project({"mean": 1}, torch.zeros(4, 3))
    with pytest.raises(lib.MofaError):
        mesh.shape_fit({}, torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32))

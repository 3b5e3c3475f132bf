"""The NumPy restatement of the mesh registration (tests/icp_reference.py) judged on the CPU: exact values, the convergence conditions of
the scene catalogue for explicit correspondences, plane- and point-metric ICP and partial overlap (what the border rule is for), the
statuses, every fault switch, and the refusals that need no GPU.  The bounds are conditions on the scheme, far above what it reaches
(5.96e-8, one float32 ulp at 1, wherever a bound says 1e-5), not tolerances tuned to it."""
import os
import re

import numpy as np
import pytest
import torch

import icp_reference as icp
from mofanerf_amd import lib, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [t[0] for t in icp.TRANSFORMS]


def model_of(name):
    return "similarity" if name.startswith("similarity") else "rigid"


def steps(res):
    return " ".join("%.1e" % h["step"] for h in res["history"])


def error(res, truth):
    return float(np.abs(res["moved"].astype(np.float64) - truth).max())


# ---- exact values -----------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_headers():
    text = open(os.path.join(ROOT, "include", "mofanerf_hip.h")).read()
    assert int(re.search(r"#define MOFA_ICP_CHUNK (\d+)", text).group(1)) == icp.CHUNK == mesh.ICP_CHUNK
    assert int(re.search(r"#define MOFA_ICP_TERMS (\d+)", text).group(1)) == icp.TERMS == mesh.ICP_TERMS
    assert {k: tuple(v) for k, v in mesh._ICP_MODEL.items()} == icp.UNKNOWNS
    assert all(f"mofa_icp_{n}" in lib.SIGNATURES for n in ("apply", "terms", "reduce", "terms_reduce", "reject"))


def test_a_dyadic_translation_is_recovered_exactly_in_one_step():
    dst = np.array([(0.5, 0.25, -1.0), (1.5, -0.75, 2.0), (-2.0, 0.125, 0.5), (0.25, 3.0, -0.5)], dtype=np.float32)      # 4 points: sqrt(4) is exact
    offset = np.array([0.5, -0.25, 0.125])
    res = icp.fit_transform((dst - offset).astype(np.float32), dst, model="translation", iterations=1)
    assert np.array_equal(res["translation"], offset) and res["scale"] == 1.0 and np.array_equal(res["rotation"], np.eye(3))
    assert np.array_equal(res["moved"], dst) and res["history"][0]["step"] == 0.5 / 3.75 and res["history"][0]["rms"] == np.sqrt(0.328125)
    again = icp.fit_transform((dst - offset).astype(np.float32), dst, model="translation", iterations=2, tol=0.0)
    assert again["status"] == "converged" and again["history"][1]["step"] == 0.0 and again["iterations"] == 2


def test_the_sums_of_three_points_are_the_hand_computed_ones():
    y = np.array([(1, 2, 3), (-2, 1, 0), (4, -1, 2)], dtype=np.float32)
    c = np.array([(0, 2, 1), (-2, 3, 1), (3, 0, 0)], dtype=np.float32)
    w, mu = np.array([1.0, 2.0, 0.5]), np.array([1.0, 0.0, -1.0])
    A, g, e = np.zeros((7, 7)), np.zeros(7), 0.0
    for i in range(3):                                      # small integers: every product and sum below is exact in any order
        yh, r = y[i].astype(np.float64) - mu, (y[i] - c[i]).astype(np.float64)
        J = np.zeros((3, 7))
        J[:, :3] = -np.array([[0, -yh[2], yh[1]], [yh[2], 0, -yh[0]], [-yh[1], yh[0], 0]])
        J[:, 3:6], J[:, 6] = np.eye(3), yh
        A, g, e = A + w[i] * J.T @ J, g + w[i] * J.T @ r, e + w[i] * r @ r
    sums = icp.two_level(icp.terms(y, c, w, mu, "point"))
    assert np.array_equal(sums[:28], A[np.triu_indices(7)]) and np.array_equal(sums[28:35], g) and sums[35] == e
    assert sums[18] == 3.5 and sums[35] == 1 * 5 + 2 * 5 + 0.5 * 6                     # A_33 = sum w;  e = sum w |r|^2
    n = np.array([(0, 0, 1), (0, 1, 0), (1, 0, 0)], dtype=np.float32)
    A, g, e = np.zeros((7, 7)), np.zeros(7), 0.0
    for i in range(3):
        yh, nn = y[i].astype(np.float64) - mu, n[i].astype(np.float64)
        J = np.concatenate([np.cross(yh, nn), nn, [nn @ yh]])
        r = nn @ (y[i] - c[i]).astype(np.float64)
        A, g, e = A + w[i] * np.outer(J, J), g + w[i] * J * r, e + w[i] * r * r
    sums = icp.two_level(icp.terms(y, c, w, mu, "plane", normals=n))
    assert np.array_equal(sums[:28], A[np.triu_indices(7)]) and np.array_equal(sums[28:35], g) and sums[35] == e
    assert not icp.terms(y, c, np.array([1.0, 0.0, 1.0]), mu, "plane", normals=n)[1].any()


def test_the_two_level_sum_is_the_written_order():
    rng = np.random.default_rng(3)
    for M in (1, 255, 256, 257, 1023, 1024, 1025, 2049, 5000):
        rows = rng.standard_normal((M, 2)) * 10.0 ** rng.integers(-8, 8, (M, 2))
        want = []
        for k0 in range(0, M, 1024):                        # scalar by scalar, as one workgroup does it
            p = [[0.0, 0.0] for _ in range(256)]
            for t in range(256):
                for i in range(k0 + t, min(k0 + 1024, M), 256):
                    p[t] = [p[t][0] + rows[i, 0], p[t][1] + rows[i, 1]]
            w = 128
            while w:
                for t in range(w):
                    p[t] = [p[t][0] + p[t + w][0], p[t][1] + p[t + w][1]]
                w //= 2
            want.append(p[0])
        assert np.array_equal(icp.chunk_sums(rows), np.array(want)), M
    assert icp.two_level(np.zeros((0, 5))).tolist() == [0.0] * 5


def test_the_solve_and_the_quaternions():
    rng = np.random.default_rng(5)
    B = rng.standard_normal((40, 7))
    H, g = B.T @ B, rng.standard_normal(7)
    sums = np.concatenate([H[np.triu_indices(7)], g, [0.0]])
    for name, idx in icp.UNKNOWNS.items():
        x = icp.solve(sums, idx)
        want = np.zeros(7)
        want[list(idx)] = np.linalg.solve(H[np.ix_(idx, idx)], -g[list(idx)])
        assert np.abs(x - want).max() < 1e-12, name
    assert icp.solve(np.zeros(36), icp.UNKNOWNS["rigid"]) is None
    for name, angle, scale in icp.TRANSFORMS:
        _, R, _ = icp.known_transform(angle, scale)
        q = icp.rotation_q(R)
        assert np.abs(icp.q_rotation(q) - R).max() < 1e-15 and abs(q @ q - 1) < 1e-15
    for R in (np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])):          # half turns: the three other branches
        assert np.array_equal(icp.q_rotation(icp.rotation_q(R)), R)
    assert icp.compose(icp.IDENTITY, np.array([0, 0, 0, 0, 0, 0, -1.0]), np.zeros(3)) is None


def test_the_border_flags_and_the_reject_rule():
    verts, faces = icp.flat_square()
    fb, vb = icp.border_flags(faces, len(verts))
    rim = np.zeros((5, 5), dtype=bool)
    rim[[0, -1]], rim[:, [0, -1]] = True, True
    assert np.array_equal(vb.reshape(5, 5).astype(bool), rim) and int(sum(bin(b).count("1") for b in fb)) == 16
    f = int(np.flatnonzero((fb == 1) | (fb == 2) | (fb == 4))[0])
    k = int(np.log2(fb[f]))
    on_edge, at_vertex = np.full(3, 0.5, dtype=np.float32), np.zeros(3, dtype=np.float32)
    on_edge[k], at_vertex[(k + 1) % 3] = 0.0, 1.0
    inner = int(np.flatnonzero(fb == 0)[0])
    got = icp.reject([f, f, f, inner, -1], np.stack([on_edge, at_vertex, np.full(3, 1 / 3, dtype=np.float32), on_edge, on_edge]), faces, fb, vb)
    assert got.tolist() == [1, 1, 0, 0, 0]


def test_the_trim_rule_keeps_ties():
    d2 = np.array([4.0, 1.0, 1.0, 1.0, 9.0, 0.5, 7.0])
    valid = np.array([1, 1, 1, 1, 1, 1, 0], dtype=bool)
    assert icp.trim_keep(d2, valid, 0.5).tolist() == [False, True, True, True, False, True, False]        # k = 3: the tied 1.0s all stay
    assert icp.trim_keep(d2, valid, 0.5, {"trim_count"}).sum() == 3
    assert np.array_equal(icp.trim_keep(d2, valid, 1.0), valid) and np.array_equal(icp.trim_keep(d2, valid, None), valid)


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------
def test_the_catalogue_is_the_issue_s():
    verts, faces = icp.patch()
    assert verts.shape == (289, 3) and faces.shape == (512, 3) and len(icp.crop()[1]) < 512
    assert len(icp.samples(0.8)[0]) == 1352 and len(icp.samples(0.9)[0]) == 1682
    for name in NAMES:
        src, truth, _ = icp.source(name)
        off = np.linalg.norm(src.astype(np.float64) - truth, axis=1)
        print(f"{name}: starts {off.min():.3f} .. {off.max():.3f} off")


@pytest.mark.parametrize("name", NAMES)
def test_explicit_correspondences_converge(name):
    src, truth, _ = icp.source(name)
    res = icp.fit_transform(src, truth, model=model_of(name), iterations=8)
    print(f"{name}: error {error(res, truth):.3e}, steps {steps(res)}")
    assert error(res, truth) <= 1e-5 and res["iterations"] == 8
    s, R, t = icp.known_transform(*next(t[1:] for t in icp.TRANSFORMS if t[0] == name))
    assert abs(res["scale"] - s) < 1e-6 and np.abs(res["rotation"] - R).max() < 1e-6 and np.abs(res["translation"] - t).max() < 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_plane_metric_icp_converges_on_the_full_patch(name):
    src, truth, _ = icp.source(name)
    res = icp.register(src, *icp.patch(), model=model_of(name), metric="plane", iterations=15)
    print(f"{name}: error {error(res, truth):.3e}, steps {steps(res)}")
    assert error(res, truth) <= 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_point_metric_icp_converges_linearly(name):
    src, truth, _ = icp.source(name)
    res = icp.register(src, *icp.patch(), model=model_of(name), metric="point", iterations=40)
    first, last = res["history"][0]["rms"], res["history"][-1]["rms"]
    print(f"{name}: rms {first:.4f} -> {last:.4f} ({first / last:.1f} x), error left {error(res, truth):.4f}")
    assert last <= first / 5


@pytest.mark.parametrize("name", ["rigid5", "rigid10"])
def test_partial_overlap_needs_the_border_rule(name):
    src, truth, _ = icp.source(name, 0.9)
    verts, faces = icp.crop()
    with_rule = icp.register(src, verts, faces, iterations=30, reject_border=True)
    without = icp.register(src, verts, faces, iterations=30, reject_border=False, trim=None)
    trimmed = icp.register(src, verts, faces, iterations=30, reject_border=False, trim=0.7)
    print(f"{name}: border rule {error(with_rule, truth):.3e} ({with_rule['history'][-1]['used']} of {len(src)} used), without "
          f"{error(without, truth):.3e}, trim 0.7 {error(trimmed, truth):.3e} ({trimmed['history'][-1]['used']} used)")
    assert error(with_rule, truth) <= 1e-5 and with_rule["history"][-1]["rejected"]["border"] > 0
    assert error(without, truth) > 1e-2
    assert error(trimmed, truth) <= 1e-5


# ---- statuses ---------------------------------------------------------------------------------------------------------------------------
def test_the_statuses():
    verts, faces = icp.flat_square()
    pts = icp.displaced(np.stack([np.linspace(0.1, 0.9, 12), np.linspace(0.9, 0.2, 12) ** 2, np.zeros(12)], -1).astype(np.float32), 5.0, 1.0)
    res = icp.register(pts, verts, faces, model="rigid", metric="plane", iterations=5)
    assert res["status"] == "singular" and res["iterations"] == 0 and res["scale"] == 1.0 and np.isnan(res["history"][0]["step"])
    assert icp.register(pts, verts, faces, model="rigid", metric="point", iterations=3)["status"] == "iterations"     # the point metric holds it
    far = icp.register(pts + np.float32(5), verts, faces, max_distance=0.5, iterations=5)
    assert far["status"] == "no_correspondences" and far["history"][0]["rejected"]["beyond"] == 12 and far["history"][0]["used"] == 0
    assert icp.register(np.zeros((0, 3), dtype=np.float32), verts, faces)["status"] == "empty"
    assert icp.fit_transform(np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.float32))["status"] == "empty"
    src, truth, _ = icp.source("rigid10")
    full = icp.fit_transform(src, truth, iterations=8)
    early = icp.fit_transform(src, truth, iterations=8, tol=1e-4)
    n = len(early["history"])
    assert early["status"] == "converged" and n < 8 and early["history"][-1]["step"] <= 1e-4 < early["history"][-2]["step"]
    assert [(h["step"], h["rms"], h["used"]) for h in early["history"]] == [(h["step"], h["rms"], h["used"]) for h in full["history"][:n]]
    assert early["iterations"] == n and np.array_equal(early["moved"], icp.fit_transform(src, truth, iterations=n)["moved"])


def test_an_init_is_taken_up():
    src, truth, _ = icp.source("similarity10")
    first = icp.fit_transform(src[::50], truth[::50], model="similarity", iterations=3)
    res = icp.register(src, *icp.patch(), model="similarity", iterations=4, init=first)
    assert error(res, truth) <= 1e-5 and res["history"][0]["rms"] < 1e-3
    again = icp.register(src, *icp.patch(), model="similarity", iterations=4, init=first["matrix"])
    assert error(again, truth) <= 1e-5


# ---- faults -----------------------------------------------------------------------------------------------------------------------------
def _fit(faults, **kw):
    src, truth, _ = icp.source("rigid10")
    return icp.fit_transform(src, truth, iterations=3, faults=faults, **kw)


def _fit_with_a_nan(faults):
    src, truth, _ = icp.source("rigid10")
    src = src.copy()
    src[7] = np.nan
    return icp.fit_transform(src, truth, iterations=2, faults=faults)


def _fit_plane_similarity(faults):
    src, truth, _ = icp.source("similarity10")
    verts, faces = icp.patch()
    res = icp.dist.brute_force(truth, verts, faces)
    normals = icp.face_normals(verts, faces, res["face"])[0].astype(np.float32)
    return icp.fit_transform(src, truth, normals=normals, model="similarity", metric="plane", iterations=3, faults=faults)


def _crop(faults):
    return icp.register(icp.source("rigid5", 0.9)[0], *icp.crop(), iterations=2, faults=faults)


def _cube_trim(faults):
    g = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    a, b = (x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij"))
    side = lambda k, h: np.roll(np.stack([np.full_like(a, h), a, b], -1), k, axis=1)
    pts = np.concatenate([side(k, h) for k in range(3) for h in (-0.125, 1.0625)])          # 54 points, 27 at each of two distances
    return icp.register(icp.displaced(pts, 0.0, 1.0), *icp.cube(), iterations=1, trim=0.4, reject_border=False, faults=faults)


FAULT_CASES = {"no_pivot": _fit, "cross_sign": _fit, "plane_no_scale": _fit_plane_similarity, "keep_rejected": _fit_with_a_nan,
               "border_wrong_edge": _crop, "trim_count": _cube_trim, "compose_reversed": _fit, "dq_not_unit": _fit, "no_recentre": _fit,
               "flat_sum": _fit}


def test_every_fault_has_a_case():
    assert set(FAULT_CASES) == set(icp.FAULTS) and len(icp.FAULTS) >= 10


@pytest.mark.parametrize("fault", icp.FAULTS)
def test_a_fault_changes_a_catalogue_case(fault):
    clean, faulty = FAULT_CASES[fault](()), FAULT_CASES[fault]({fault})
    bad = icp.mismatches(faulty, clean)
    print(f"{fault}: {bad}")
    assert bad
    assert not icp.mismatches(FAULT_CASES[fault](()), clean)


# ---- refusals that need no GPU ----------------------------------------------------------------------------------------------------------
def test_cpu_tensors_and_bad_arguments_are_refused():
    verts, faces = (torch.from_numpy(x) for x in icp.patch())
    pts = torch.from_numpy(icp.source("rigid5")[0])
    for call in (lambda: mesh.transform_points(pts, 1.0, np.eye(3), np.zeros(3)), lambda: mesh.fit_transform(pts, pts),
                 lambda: mesh.register(pts, verts, faces), lambda: mesh.register_meshes(verts, faces, verts, faces, 0.5)):
        with pytest.raises(lib.MofaError):
            call()
    for kw in (dict(model="affine"), dict(metric="line"), dict(iterations=-1), dict(iterations=1.5), dict(tol=-1.0), dict(tol=float("nan"))):
        with pytest.raises(lib.MofaError):
            mesh._icp_args("register", **{**dict(model="rigid", metric="plane", iterations=3, tol=0.0), **kw})
    for init in ({"scale": 1.0}, np.zeros((4, 4)), np.eye(3), {"scale": -1.0, "rotation": np.eye(3), "translation": np.zeros(3)}):
        with pytest.raises(lib.MofaError):
            mesh._icp_init("register", init)


def test_the_products_host_step_is_the_restatements():
    """The solve and the composition need no GPU: mesh.py's against the restatement's, bit for bit, over a converging sequence."""
    src, truth, _ = icp.source("similarity10")
    mu, extent = icp.box_of(truth)
    state_p, state_r = mesh._ICP_IDENTITY, icp.IDENTITY
    for _ in range(4):
        moved = icp.apply(src, state_r[0], icp.q_rotation(state_r[1]), state_r[2])
        sums = icp.two_level(icp.terms(moved, truth, np.ones(len(src)), mu, "point"))
        for model, idx in icp.UNKNOWNS.items():
            assert np.array_equal(np.array(mesh._icp_solve([float(v) for v in sums], idx)), icp.solve(sums, idx)), model
        x = icp.solve(sums, icp.UNKNOWNS["similarity"])
        state_p = mesh._icp_compose(state_p, [float(v) for v in x], tuple(float(v) for v in mu))
        state_r = icp.compose(state_r, x, mu)
        assert state_p[0] == state_r[0] and np.array_equal(np.array(state_p[1]), state_r[1]) and np.array_equal(np.array(state_p[2]), state_r[2])
        assert mesh._icp_step_size([float(v) for v in x], extent) == icp.step_size(x, extent)
        assert np.array_equal(np.array(mesh._quat_rotation(state_p[1])).reshape(3, 3), icp.q_rotation(state_r[1]))
    assert mesh._icp_extent(np.stack([truth.min(0), truth.max(0)])) == (tuple(float(v) for v in mu), extent)
    for name, angle, scale in icp.TRANSFORMS:
        R = icp.known_transform(angle, scale)[1]
        assert np.array_equal(np.array(mesh._rotation_quat([float(v) for v in R.reshape(-1)])), icp.rotation_q(R))

"""The linear shape model on the GPU (``mofa_shape_*``, ``mesh.shape_model`` / ``shape_synthesize`` / ``shape_project`` / ``shape_fit`` /
``write_shape_model`` / ``read_shape_model``) against the NumPy restatement (tests/shape_reference.py; tests/test_shape_reference_cpu.py
shows what it catches), bit for bit:

* the Gram kernel and the wide reduce with N around every boundary of the summation (1, 2, 255 .. 257, the chunk of 1024 +- 1, two
  chunks + 1, and 1024^2 + 1: a third level), R around the 8 x 8 pair tile and beyond mofa_icp_reduce's 36 columns, both groups, no
  weights, weights with zeros, NaN and inf under weight 0, values scaled by 1e-6 and 1e6; two runs give equal bytes;
* centre, combine and the plane rows at the same sizes, a face outside the mesh and a degenerate face included;
* the public calls: every returned array and every history entry, the grid changing no byte, the convergence conditions of the CPU test
  on the GPU's own result, the file round trip, the refusals;
* ``register`` and ``warp`` still return what their restatements say.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dist_reference as dist
import icp_reference as icp
import shape_reference as sr
from mofanerf_amd import lib, mesh

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = icp.CHUNK
SIZES = (1, 2, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, CHUNK * CHUNK + 1)
ROWS = (1, 2, 7, 8, 9, 17, 37)
TRUTH = sr.member(sr.UNSEEN)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(res):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def same(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return dist._same(got, np.asarray(want))


def gpu_model():
    return mesh.shape_model(dev(sr.family()))


def moved_target():
    verts, faces = sr.target()
    s, R, t = icp.known_transform(5.0, 1.0)
    return (s * (sr.widen(verts) @ R.T) + t).astype(np.float32), faces


# ---- the Gram kernel --------------------------------------------------------------------------------------------------------------------
def gram_case(R, n_weights, group, pattern, scale=1.0):
    rng = np.random.default_rng(R * 7919 + n_weights % 9973 + group)
    N = n_weights * group
    P = rng.normal(size=(R, N)) * scale
    if pattern == "none":
        return P, None
    w = rng.uniform(0.25, 2.0, n_weights)
    w[rng.uniform(size=n_weights) < 0.3] = 0.0
    if pattern == "poison":
        dead = np.repeat(w == 0.0, group)
        P[:, dead] = np.where(rng.uniform(size=(R, int(dead.sum()))) < 0.5, np.nan, np.inf)
        w[:1] = 0.0 if n_weights > 1 else w[:1]
    return P, w


def gpu_gram(P, w, group):
    R, N = P.shape
    return mesh._shape_gram(dev(P), R, N, None if w is None else dev(w), group)


@pytest.mark.parametrize("N", SIZES)
def test_gram_equals_the_restatement_at_every_size(N):
    R = 3 if N > 4 * CHUNK else 9
    for group in (1, 3):
        n_weights = N if group == 1 else (N + 2) // 3 if N > 4 * CHUNK else N
        for pattern in ("none", "zeros", "poison"):
            P, w = gram_case(R, n_weights, group, pattern)
            got = gpu_gram(P, w, group)
            assert same(got, sr.gram(P, w, group)), (N, group, pattern)
            assert np.isfinite(got).all()
            assert gpu_gram(P, w, group).tobytes() == got.tobytes()


@pytest.mark.parametrize("R", ROWS)
def test_gram_equals_the_restatement_at_every_row_count(R):
    for group, n_weights in ((1, 2 * CHUNK + 1), (3, 343)):
        for pattern, scale in (("none", 1.0), ("zeros", 1e-6), ("poison", 1e6)):
            P, w = gram_case(R, n_weights, group, pattern, scale)
            got = gpu_gram(P, w, group)
            assert got.shape == (R * (R + 1) // 2,) and same(got, sr.gram(P, w, group)), (R, group, pattern)


def test_gram_all_rejected_is_exact_zero_and_the_reduce_is_icp_reduces():
    P, _ = gram_case(9, 1500, 1, "none")
    got = gpu_gram(P, np.zeros(1500), 1)
    assert not got.any() and not np.signbit(got).any()
    rows = np.random.default_rng(1).normal(size=(2 * CHUNK + 5, 50))
    out = torch.empty(3, 50, dtype=torch.float64, device=DEV)
    held = dev(rows)                                               # (held: a temporary's memory is handed out again)
    lib.check(lib.load().mofa_shape_reduce(held.data_ptr(), len(rows), 50, out.data_ptr(), lib.stream()), "mofa_shape_reduce")
    assert same(out, icp.chunk_sums(rows))
    narrow = mesh._icp_reduce(dev(rows[:, :36].copy()), len(rows), 36)
    wide = torch.empty(3, 36, dtype=torch.float64, device=DEV)
    held = dev(rows[:, :36].copy())
    lib.check(lib.load().mofa_shape_reduce(held.data_ptr(), len(rows), 36, wide.data_ptr(), lib.stream()), "mofa_shape_reduce")
    assert same(mesh._icp_reduce(wide, 3, 36), narrow.cpu().numpy())


# ---- centre, combine, plane rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_centre_and_combine_equal_the_restatement(n):
    rng = np.random.default_rng(n)
    M = 2 if n > 4 * CHUNK else 5                                  # (small at the third-level size, as R is for the Gram kernel)
    meshes = (rng.normal(size=(M, n)) * 10.0 ** rng.integers(-3, 4, size=(1, n))).astype(np.float32)
    mean, X = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(M, n, dtype=torch.float64, device=DEV)
    held = dev(meshes)
    lib.check(lib.load().mofa_shape_centre(lib.ptr(held), M, n, mean.data_ptr(), X.data_ptr(), lib.stream()), "mofa_shape_centre")
    want_mean, want_X = sr.centre(meshes)
    assert same(mean, want_mean) and same(X, want_X)
    coef = rng.normal(size=(3, M))
    assert same(mesh._shape_combine(None, coef, X, n), sr.combine(None, coef, want_X))
    assert same(mesh._shape_combine(mean, coef, X, n), sr.combine(want_mean, coef, want_X))
    assert same(mesh._shape_combine(mean, coef[:1, :1], X[:1], n), sr.combine(want_mean, coef[:1, :1], want_X[:1]))


@pytest.mark.parametrize("V", SIZES)
def test_plane_rows_equal_the_restatement(V):
    rng = np.random.default_rng(V)
    verts, faces = icp.patch()
    verts = np.concatenate([verts, verts[:1]])                                   # a degenerate face: two equal corners
    faces = np.concatenate([faces, np.array([[0, len(verts) - 1, 5]], dtype=np.int32)])
    face = rng.integers(0, len(faces), V).astype(np.int32)
    face[::7] = np.array([-1, len(faces), len(faces) - 1, 2 ** 31 - 1])[np.arange(len(face[::7])) % 4]
    moved = rng.uniform(-1, 1, (V, 3)).astype(np.float32)
    closest = (moved + rng.normal(size=(V, 3)) * 0.05).astype(np.float32)
    s, R, t = icp.known_transform(20.0, 1.3)
    for K in ((0, 2) if V > 4 * CHUNK else (0, 1, 4)):             # (few modes at the third-level size)
        modes = rng.normal(size=(K, V, 3))
        P = torch.full((K + 1, V), 7.0, dtype=torch.float64, device=DEV)
        T = (C.c_double * 13)(s, *R.reshape(-1), *t)
        d = [dev(a) for a in (moved, closest, face, verts, faces, modes)]               # (held while the kernel reads them)
        lib.check(lib.load().mofa_shape_plane_rows(lib.ptr(d[0]), lib.ptr(d[1]), d[2].data_ptr(), lib.ptr(d[3]), len(verts), d[4].data_ptr(), len(faces),
                                                   T, d[5].data_ptr() if K else None, K, V, P.data_ptr(), lib.stream()), "mofa_shape_plane_rows")
        want = sr.plane_rows(moved, closest, face, verts, faces, s, R, modes)
        assert same(P, want) and np.isnan(want[:, 0]).all()
        if V > 21:
            assert np.isnan(want[:, 14]).all() and np.isnan(want[:, 21]).all() and np.isfinite(want).any()


# ---- the public calls -------------------------------------------------------------------------------------------------------------------
def test_shape_model_equals_the_restatement():
    got = host(gpu_model())
    assert not sr.mismatches(got, sr.model()) and got["modes"].shape == (3, 169, 3) and got["modes"].dtype == np.float64
    again = host(gpu_model())
    assert again["modes"].tobytes() == got["modes"].tobytes() and again["coeffs"].tobytes() == got["coeffs"].tobytes()
    for kw in (dict(components=2), dict(rank_tol=0.5), dict(components=99)):
        assert not sr.mismatches(host(mesh.shape_model(dev(sr.family()), **kw)), sr.shape_model(sr.family(), **kw)), kw
    timed = host(mesh.shape_model(dev(sr.family()), timing=True))
    assert set(timed.pop("times")) == {"align", "gram", "jacobi", "modes"} and not sr.mismatches(timed, sr.model())
    pair = sr.family()[:2]
    assert not sr.mismatches(host(mesh.shape_model(dev(pair))), sr.shape_model(pair))


@pytest.mark.parametrize("align", ["rigid", "similarity"])
def test_shape_model_with_alignment_equals_the_restatement(align):
    fam = sr.family()[:5].copy()
    for m in range(1, 5):
        s, R, t = icp.known_transform(3.0 * m, 1.0 + 0.02 * m if align == "similarity" else 1.0)
        fam[m] = (s * (sr.widen(fam[m]) @ R.T) + 0.3 * t).astype(np.float32)
    got, want = host(mesh.shape_model(dev(fam), align=align)), sr.shape_model(fam, align=align)
    assert not sr.mismatches(got, want) and got["transforms"].shape == (5, 4, 4)
    assert got["eigenvalues"][:3].sum() < sr.shape_model(fam)["eigenvalues"][:3].sum()


def test_shape_synthesize_equals_the_restatement():
    model, want = gpu_model(), sr.model()
    coeffs = np.random.default_rng(2).normal(size=(4, 3))
    for c in (coeffs, coeffs[:, :2], coeffs[:1, :0]):
        assert same(mesh.shape_synthesize(model, c), sr.shape_synthesize(want, c))
        assert same(mesh.shape_synthesize(model, dev(c), dtype=torch.float32), sr.shape_synthesize(want, c, np.float32))
    assert tuple(mesh.shape_synthesize(model, np.zeros((0, 3))).shape) == (0, 169, 3)
    assert same(mesh.shape_synthesize(model, want["coeffs"][:1], dtype=torch.float32), sr.shape_synthesize(want, want["coeffs"][:1], np.float32))


def test_shape_project_equals_the_restatement():
    model, want = gpu_model(), sr.model()
    few = np.zeros(169)
    few[[0, 12, 84, 100, 156, 168, 40, 130]] = np.array([1.0, 0.5, 2.0, 1.0, 1.0, 3.0, 1.0, 0.25])
    noisy = TRUTH.copy()
    noisy[few == 0] = np.nan
    for verts, kw in ((TRUTH, {}), (TRUTH, dict(regularize=10.0)), (noisy, dict(weight=few)), (noisy, dict(weight=few, regularize=0.5, components=2)),
                      (noisy, {}), (TRUTH, dict(weight=np.zeros(169)))):
        g = dict(kw, weight=dev(kw["weight"])) if "weight" in kw else kw
        got, ref = host(mesh.shape_project(model, dev(verts), **g)), sr.shape_project(want, verts, **kw)
        assert not sr.mismatches(got, ref), (kw, sr.mismatches(got, ref))
    res = mesh.shape_project(model, dev(TRUTH))
    assert res["status"] == "ok" and res["rms"] < 1e-7 and sr.rms_error(res["verts"].cpu().numpy(), TRUTH) < 1e-7
    twice = dict(model, modes=torch.cat([model["modes"], model["modes"][:1]]).contiguous())
    assert mesh.shape_project(twice, dev(TRUTH))["status"] == "singular"


FITS = (("full", dict(iterations=3)), ("crop", dict(iterations=3)), ("full", dict(iterations=3, metric="point")),
        ("crop", dict(iterations=2, metric="point", reject_border=False)), ("moved", dict(iterations=4, pose="rigid")),
        ("moved", dict(iterations=3, pose="similarity", metric="point")), ("moved", dict(iterations=3, pose="similarity", regularize=0.05)),
        ("full", dict(iterations=3, max_distance=0.03)), ("crop", dict(iterations=2, reject_border=False, components=2)),
        ("full", dict(iterations=6, tol=1e-6)), ("full", dict(iterations=2, max_distance=1e-6)))


def target_of(name):
    return moved_target() if name == "moved" else sr.target(cropped=name == "crop")


@pytest.mark.parametrize("name,kw", FITS, ids=[f"{n}-{i}" for i, (n, _) in enumerate(FITS)])
def test_shape_fit_equals_the_restatement(name, kw):
    verts, faces = target_of(name)
    want = sr.shape_fit(sr.model(), verts, faces, **kw)
    got = host(mesh.shape_fit(gpu_model(), dev(verts), dev(faces), **kw))
    bad = sr.mismatches(got, want)
    print(name, kw, want["status"], [h["shape"]["used"] for h in want["history"]], sr.rms_error(want["model_verts"], TRUTH))
    assert not bad, (kw, bad, got["status"], want["status"])
    assert got["verts"].dtype == np.float32 and got["model_verts"].dtype == np.float64 and len(got["grid"]) == 3


def test_the_grid_changes_no_byte_and_two_runs_agree():
    verts, faces = moved_target()
    kw = dict(iterations=3, pose="rigid")
    model = gpu_model()
    runs = [host(mesh.shape_fit(model, dev(verts), dev(faces), grid=g, **kw)) for g in (1, 5, None, None)]
    assert runs[0]["grid"] == (1, 1, 1) and runs[1]["grid"] == (5, 5, 5)
    for r in runs[1:]:
        r = dict(r, grid=runs[0]["grid"])
        assert not sr.mismatches(r, runs[0])
    timed = host(mesh.shape_fit(model, dev(verts), dev(faces), timing=True, **kw))
    assert set(timed.pop("times")) == {"bin", "query", "rows", "gram", "host"} and not sr.mismatches(dict(timed, grid=(1, 1, 1)), runs[0])


def test_it_converges_on_the_gpu():
    """The CPU test's conditions on the GPU's own results."""
    model = gpu_model()
    verts, faces = (dev(a) for a in sr.target())
    plane = mesh.shape_fit(model, verts, faces, iterations=3)
    assert sr.rms_error(plane["model_verts"].cpu().numpy(), TRUTH) < 1e-6
    crop = mesh.shape_fit(model, *(dev(a) for a in sr.target(cropped=True)), iterations=3)
    assert sr.rms_error(crop["model_verts"].cpu().numpy(), TRUTH) < 1e-6
    assert all(c["shape"]["used"] < f["shape"]["used"] for c, f in zip(crop["history"], plane["history"]))
    point = mesh.shape_fit(model, verts, faces, iterations=3, metric="point")
    assert sr.rms_error(point["model_verts"].cpu().numpy(), TRUTH) > 1000 * sr.rms_error(plane["model_verts"].cpu().numpy(), TRUTH)
    mv, mf = moved_target()
    rigid = mesh.shape_fit(model, dev(mv), dev(mf), iterations=15, pose="rigid")
    s, R, t = icp.known_transform(5.0, 1.0)
    assert sr.rms_error(rigid["verts"].cpu().numpy(), (s * (sr.widen(TRUTH) @ R.T) + t).astype(np.float32)) < 1e-5
    twice = dict(model, modes=torch.cat([model["modes"], model["modes"][:1]]).contiguous())
    assert mesh.shape_fit(twice, verts, faces, iterations=2)["status"] == "singular"
    assert mesh.shape_fit(model, verts, faces[:0].contiguous(), iterations=2)["status"] == "no_correspondences"


def test_file_round_trip_keeps_every_bit(tmp_path):
    model = gpu_model()
    faces = sr.field_faces(sr.N_GRID)
    mesh.write_shape_model(str(tmp_path / "model.npz"), model, dev(faces))
    back = mesh.read_shape_model(str(tmp_path / "model.npz"), DEV)
    assert back["modes"].is_cuda and back["modes"].dtype == torch.float64 and np.array_equal(back.pop("faces").cpu().numpy(), faces)
    assert not sr.mismatches(host(back), host(model)) and set(back) == set(model)
    assert same(mesh.shape_synthesize(back, [[1.0, -1.0, 0.5]]), sr.shape_synthesize(sr.model(), [[1.0, -1.0, 0.5]]))
    with np.load(tmp_path / "model.npz", allow_pickle=False) as z:
        assert set(z.files) == {"mean", "modes", "sigma", "eigenvalues", "coeffs", "explained", "n_meshes", "faces"}
    np.savez(tmp_path / "other.npz", mean=np.zeros((3, 3)))
    with pytest.raises(lib.MofaError):
        mesh.read_shape_model(str(tmp_path / "other.npz"), DEV)


# ---- what was there before --------------------------------------------------------------------------------------------------------------
def test_register_and_warp_are_unchanged():
    import warp_reference as wr
    verts, faces = icp.crop()
    src, _, _ = icp.source("rigid10", 0.9)
    kw = dict(model="rigid", metric="plane", iterations=5)
    assert not icp.mismatches(host(mesh.register(dev(src), dev(verts), dev(faces), **kw)), icp.register(src, verts, faces, **kw))
    kw = dict(metric="plane", stiffness=(1.0, 0.1), iterations=2)
    tv, tf, pv, pf = wr.scene("crop")
    assert not wr.mismatches(host(mesh.warp(dev(tv), dev(tf), dev(pv), dev(pf), **kw)), wr.warp(tv, tf, pv, pf, **kw))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise():
    fam, model = dev(sr.family()), gpu_model()
    verts, faces = (dev(a) for a in sr.target())
    nan = fam.clone()
    nan[3, 5, 1] = float("nan")
    for bad in (lambda: mesh.shape_model(fam.cpu()), lambda: mesh.shape_model(fam.double()), lambda: mesh.shape_model(fam[:1]),
                lambda: mesh.shape_model(fam[0]), lambda: mesh.shape_model(torch.zeros(257, 4, 3, device=DEV)), lambda: mesh.shape_model(nan),
                lambda: mesh.shape_model(fam, align="affine"), lambda: mesh.shape_model(fam, components=-1), lambda: mesh.shape_model(fam, rank_tol=2.0),
                lambda: mesh.shape_model(torch.zeros(3, 0, 3, device=DEV)),
                lambda: mesh.shape_synthesize(model, np.zeros((1, 4))), lambda: mesh.shape_synthesize(model, [[float("nan")]]),
                lambda: mesh.shape_synthesize(model, [[0.0]], dtype=torch.float16), lambda: mesh.shape_synthesize(host(model), [[0.0]]),
                lambda: mesh.shape_synthesize(dict(model, modes=model["modes"].float()), [[0.0]]),
                lambda: mesh.shape_project(model, dev(TRUTH[:5])), lambda: mesh.shape_project(model, dev(TRUTH), regularize=-1.0),
                lambda: mesh.shape_project(model, dev(TRUTH), weight=dev(-np.ones(169))), lambda: mesh.shape_project(model, dev(TRUTH).cpu()),
                lambda: mesh.shape_fit(model, verts, faces, metric="line"), lambda: mesh.shape_fit(model, verts, faces, pose="affine"),
                lambda: mesh.shape_fit(model, verts, faces, iterations=-1), lambda: mesh.shape_fit(model, verts, faces, max_distance=0.0),
                lambda: mesh.shape_fit(model, verts, faces, regularize=float("inf")), lambda: mesh.shape_fit(model, verts, faces, grid=0),
                lambda: mesh.shape_fit(model, verts, faces, init_coeffs=[0.0]), lambda: mesh.shape_fit(model, verts.cpu(), faces),
                lambda: mesh.shape_fit(model, verts, faces.long()), lambda: mesh.shape_fit(model, verts, faces, components=1.5)):
        with pytest.raises(lib.MofaError):
            bad()
    L = lib.load()
    P = torch.zeros(2, 8, dtype=torch.float64, device=DEV)
    out = torch.zeros(8, dtype=torch.float64, device=DEV)
    assert L.mofa_shape_gram(P.data_ptr(), 0, 8, None, 1, out.data_ptr(), lib.stream()) != 0
    assert L.mofa_shape_gram(P.data_ptr(), 257, 8, None, 1, out.data_ptr(), lib.stream()) != 0
    assert L.mofa_shape_gram(P.data_ptr(), 2, 8, None, 2, out.data_ptr(), lib.stream()) != 0
    assert L.mofa_shape_gram(P.data_ptr(), 2, 8, out.data_ptr(), 3, out.data_ptr(), lib.stream()) != 0        # 8 columns, group 3
    assert L.mofa_shape_gram(None, 2, 8, None, 1, out.data_ptr(), lib.stream()) != 0
    assert L.mofa_shape_reduce(out.data_ptr(), 8, 1, out.data_ptr(), lib.stream()) != 0
    assert L.mofa_shape_centre(None, 2, 8, out.data_ptr(), P.data_ptr(), lib.stream()) != 0
    assert L.mofa_shape_combine(None, out.data_ptr(), P.data_ptr(), 1, 0, 8, out.data_ptr(), lib.stream()) != 0

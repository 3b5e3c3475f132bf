"""Mesh registration on the GPU (``mofa_icp_*``, ``mesh.transform_points`` / ``fit_transform`` / ``register`` / ``register_meshes``) against the
NumPy restatement (tests/icp_reference.py; tests/test_icp_reference_cpu.py shows what it catches):

* ``transform_points`` is the restatement's bit for bit, N = 0 and 1 and a large translation included;
* the 36 terms, their two-level sum and the fused launch are the restatement's bit for bit for both metrics, with N around every
  boundary of the summation (1, 255, 256, 257, the chunk of 1024 +- 1, two chunks + 1, and 1024^2 + 1: a third level) and rejected rows in
  prescribed patterns (none, all, every other, one whole chunk);
* the reject kernel equals the restatement on the crop, with queries on its edges and vertices;
* ``fit_transform`` over 8 steps and ``register`` over 10 iterations are the restatement's bit for bit — transform, moved points and
  every history entry — for every model, both metrics, with and without trim and border rule; the grid changes no bit and two runs
  give equal bytes;
* the convergence conditions of the CPU tests hold on the GPU's own result;
* ``register_meshes`` recovers a moved cube; the sample weights reach the sums and the weight-0 vertices do not change them;
* bad arguments on device tensors raise ``MofaError``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dist_reference as dist
import icp_reference as icp
from mofanerf_amd import lib, mesh

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = [t[0] for t in icp.TRANSFORMS]
CHUNK = icp.CHUNK
SIZES = (1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, CHUNK * CHUNK + 1)
PATTERNS = ("none", "all", "every_other", "one_chunk")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(res):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def same(got, want):
    return dist._same(np.asarray(got), np.asarray(want))


def model_of(name):
    return "similarity" if name.startswith("similarity") else "rigid"


def error(res, truth):
    return float(np.abs(np.asarray(res["moved"]).astype(np.float64) - truth).max())


# ---- transform_points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 1000])
def test_transform_points_equals_the_restatement(N):
    rng = np.random.default_rng(N)
    pts = rng.uniform(-2, 2, (N, 3)).astype(np.float32)
    for s, (_, R, _), t in ((1.0, icp.known_transform(10, 1), icp.OFFSET), (1.1, icp.known_transform(20, 1), np.array([1e6, -3e5, 7.25])),
                            (0.37, icp.known_transform(5, 1), np.zeros(3))):
        got = mesh.transform_points(dev(pts), s, R, t)
        assert got.dtype == torch.float32 and tuple(got.shape) == (N, 3) and same(got.cpu().numpy(), icp.apply(pts, s, R, t))
    assert same(mesh.transform_points(dev(pts), 1.0, torch.eye(3), torch.zeros(3)).cpu().numpy(), pts)


# ---- terms and reduce -------------------------------------------------------------------------------------------------------------------
def correspondences(N, pattern):
    """Moved points near the patch, target points, faces (a few outside the mesh), explicit normals and weights with the rejected rows of
    ``pattern``."""
    rng = np.random.default_rng(N % 9973)
    verts, faces = icp.patch()
    moved = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    target = (moved + rng.normal(0, 0.05, (N, 3))).astype(np.float32)
    face = rng.integers(0, len(faces), N).astype(np.int32)
    face[::97] = -1
    face[5::211] = len(faces)
    normals = rng.standard_normal((N, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(np.float32)
    weight = rng.uniform(0.5, 2.0, N)
    i = np.arange(N)
    weight[{"none": np.zeros(N, dtype=bool), "all": np.ones(N, dtype=bool), "every_other": i % 2 == 1,
            "one_chunk": (i >= CHUNK) & (i < 2 * CHUNK) if N > CHUNK else i < 0}[pattern]] = 0.0
    return moved, target, face, normals, weight


def gpu_sums(moved, target, face, normals, weight, mu, metric, fused, keep=True):
    """(terms [N,36] or None, the 36 sums) through the C ABI."""
    L, N = lib.load(), len(moved)
    verts, faces = icp.patch()
    m, t, w, v, f = dev(moved), dev(target), dev(weight), dev(verts), dev(faces)
    fc = dev(face) if face is not None else None
    nr = dev(normals) if normals is not None else None
    args = (m.data_ptr(), t.data_ptr(), nr.data_ptr() if nr is not None else None, fc.data_ptr() if fc is not None else None, v.data_ptr(),
            len(verts), f.data_ptr(), len(faces), w.data_ptr(), N, (C.c_double * 3)(*mu), mesh._ICP_METRIC[metric])
    n = (N + CHUNK - 1) // CHUNK
    if fused:
        rows = torch.full((n, icp.TERMS), float("nan"), dtype=torch.float64, device=DEV)
        lib.check(L.mofa_icp_terms_reduce(*args, rows.data_ptr(), lib.stream()), "mofa_icp_terms_reduce")
        return None, mesh._icp_reduce(rows, n, icp.TERMS).cpu().numpy()
    terms = torch.full((N, icp.TERMS), float("nan"), dtype=torch.float64, device=DEV)
    lib.check(L.mofa_icp_terms(*args, terms.data_ptr(), lib.stream()), "mofa_icp_terms")
    return terms.cpu().numpy() if keep else None, mesh._icp_reduce(terms, N, icp.TERMS).cpu().numpy()


@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("N", SIZES)
def test_terms_and_sums_equal_the_restatement(N, metric):
    mu = (0.125, -0.3, 0.2)
    verts, faces = icp.patch()
    big = N > 4 * CHUNK                    # the third level: two patterns, and the [N,36] matrix stays on the device
    for pattern in (PATTERNS[2:] if big else PATTERNS):
        moved, target, face, normals, weight = correspondences(N, pattern)
        want_terms = icp.terms(moved, target, weight, mu, metric, face=face, verts=verts, faces=faces)
        want = icp.two_level(want_terms)
        terms, sums = gpu_sums(moved, target, face if metric == "plane" else None, None, weight, mu, metric, fused=False, keep=not big)
        assert big or same(terms, want_terms), (pattern, "terms")
        assert same(sums, want), (pattern, "reduce")
        assert same(gpu_sums(moved, target, face if metric == "plane" else None, None, weight, mu, metric, fused=True)[1], want), (pattern, "fused")
        if pattern == "all":
            assert not want.any() and not np.signbit(sums).any()
        if pattern == "one_chunk" and N > CHUNK:
            assert not want_terms[CHUNK:2 * CHUNK].any() and want_terms[:CHUNK].any()
    if metric == "plane" and N <= 2 * CHUNK + 1:                                       # explicit normals instead of the closest faces
        moved, target, face, normals, weight = correspondences(N, "every_other")
        want = icp.two_level(icp.terms(moved, target, weight, mu, "plane", normals=normals))
        assert same(gpu_sums(moved, target, None, normals, weight, mu, "plane", fused=True)[1], want)
        assert same(gpu_sums(moved, target, None, normals, weight, mu, "plane", fused=False)[1], want)


@pytest.mark.parametrize("ncols", [1, 5, 12, 13, 36])
def test_reduce_takes_any_width(ncols):
    rng = np.random.default_rng(ncols)
    rows = rng.standard_normal((3 * CHUNK + 17, ncols)) * 10.0 ** rng.integers(-6, 6, (3 * CHUNK + 17, ncols))
    assert same(mesh._icp_reduce(dev(rows), len(rows), ncols).cpu().numpy(), icp.two_level(rows))
    with pytest.raises(lib.MofaError):
        mesh._icp_reduce(dev(np.zeros((4, 37))), 4, 37)


# ---- the reject kernel ------------------------------------------------------------------------------------------------------------------
def test_the_reject_kernel_equals_the_restatement_on_the_crop():
    verts, faces = icp.crop()
    q = dist.queries_for(verts, faces, 7, seed=11)
    q = np.concatenate([q, verts[::7], (verts[faces[::5, 0]].astype(np.float64) + verts[faces[::5, 1]]).astype(np.float32) / 2])
    v, f = dev(verts), dev(faces)
    res = mesh.closest_points(dev(q), v, f)
    fb, vb = mesh._border_flags("test", f, len(verts), len(faces))
    want_fb, want_vb = icp.border_flags(faces, len(verts))
    assert fb.dtype == torch.uint8 and np.array_equal(fb.cpu().numpy(), want_fb) and np.array_equal(vb.cpu().numpy(), want_vb)
    got = torch.full((len(q),), 7, dtype=torch.uint8, device=DEV)
    lib.check(lib.load().mofa_icp_reject(res["face"].data_ptr(), res["bary"].data_ptr(), len(q), f.data_ptr(), len(faces), len(verts),
                                         fb.data_ptr(), vb.data_ptr(), got.data_ptr(), lib.stream()), "mofa_icp_reject")
    face, bary = res["face"].cpu().numpy(), res["bary"].cpu().numpy()
    want = icp.reject(face, bary, faces, want_fb, want_vb)
    zeros = (bary == 0).sum(1)
    print(f"{len(q)} queries: {int((zeros == 1).sum())} on edges, {int((zeros == 2).sum())} on vertices, {int(want.sum())} rejected, "
          f"{int((face < 0).sum())} without a face")
    assert np.array_equal(got.cpu().numpy(), want)
    assert (zeros == 1).sum() > 20 and (zeros == 2).sum() > 20 and 0 < want.sum() < (face >= 0).sum()
    assert (want[zeros == 1] == 0).any() and (want[zeros == 2] == 0).any()          # inner edges and vertices stay
    assert not dist.mismatches(host(res), dist.brute_force(q, verts, faces))


# ---- fit_transform ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["translation", "rigid", "similarity"])
@pytest.mark.parametrize("name", NAMES)
def test_fit_transform_equals_the_restatement(name, model):
    src, truth, weight = icp.source(name)
    got = host(mesh.fit_transform(dev(src), dev(truth), model=model, iterations=8))
    want = icp.fit_transform(src, truth, model=model, iterations=8)
    assert not icp.mismatches(got, want) and len(got["history"]) == 8
    if model == model_of(name):
        assert error(got, truth) <= 1e-5
    got = host(mesh.fit_transform(dev(src), dev(truth), weight=dev(weight), model=model, iterations=3))
    assert not icp.mismatches(got, icp.fit_transform(src, truth, weight=weight, model=model, iterations=3))


def test_fit_transform_with_normals_holes_and_an_init():
    src, truth, _ = icp.source("similarity10")
    verts, faces = icp.patch()
    normals = icp.face_normals(verts, faces, dist.brute_force(truth, verts, faces)["face"])[0].astype(np.float32)
    src = src.copy()
    src[3], src[900, 1] = np.nan, np.inf
    first = icp.fit_transform(src[::40], truth[::40], model="similarity", iterations=2)
    for init in (None, first, first["matrix"]):
        got = host(mesh.fit_transform(dev(src), dev(truth), normals=dev(normals), model="similarity", metric="plane", iterations=4, init=init))
        want = icp.fit_transform(src, truth, normals=normals, model="similarity", metric="plane", iterations=4, init=init)
        assert not icp.mismatches(got, want) and got["history"][0]["rejected"]["non_finite"] == 2
    early = host(mesh.fit_transform(dev(src), dev(truth), iterations=8, tol=1e-4))
    assert early["status"] == "converged" and not icp.mismatches(early, icp.fit_transform(src, truth, iterations=8, tol=1e-4))
    empty = mesh.fit_transform(dev(src[:0]), dev(truth[:0]))
    assert empty["status"] == "empty" and empty["scale"] == 1.0 and np.array_equal(empty["matrix"], np.eye(4)) and tuple(empty["moved"].shape) == (0, 3)


# ---- register ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reject_border", [True, False])
@pytest.mark.parametrize("trim", [None, 0.7])
@pytest.mark.parametrize("metric", ["plane", "point"])
@pytest.mark.parametrize("target", ["patch", "crop"])
def test_register_equals_the_restatement(target, metric, trim, reject_border):
    verts, faces = icp.patch() if target == "patch" else icp.crop()
    src, truth, _ = icp.source("rigid10", 0.8 if target == "patch" else 0.9)
    kw = dict(model="rigid", metric=metric, iterations=10, trim=trim, reject_border=reject_border, tol=0.0)
    got = host(mesh.register(dev(src), dev(verts), dev(faces), **kw))
    want = icp.register(src, verts, faces, **kw)
    print(f"{target} {metric} trim={trim} border={reject_border}: {want['status']}, error {error(want, truth):.3e}, used {want['history'][-1]['used']}, "
          f"rejected {want['history'][-1]['rejected']}")
    assert not icp.mismatches(got, want) and len(got["history"]) == 10
    for grid in (1, (5, 3, 2)):
        other = host(mesh.register(dev(src), dev(verts), dev(faces), grid=grid, **kw))
        assert not icp.mismatches(other, got) and other["grid"] == ((1, 1, 1) if grid == 1 else grid)
    again = host(mesh.register(dev(src), dev(verts), dev(faces), **kw))
    assert again["moved"].tobytes() == got["moved"].tobytes() and again["matrix"].tobytes() == got["matrix"].tobytes()


def test_register_similarity_weights_max_distance_and_tol():
    verts, faces = icp.patch()
    src, truth, weight = icp.source("similarity10")
    weight = weight.copy()
    weight[::3] = 0.0
    kw = dict(model="similarity", iterations=6, max_distance=0.2, pivot=(0.1, 0.2, 0.3))
    got = host(mesh.register(dev(src), dev(verts), dev(faces), weight=dev(weight), **kw))
    want = icp.register(src, verts, faces, weight=weight, **kw)
    assert not icp.mismatches(got, want) and "beyond" in got["history"][0]["rejected"] and got["history"][0]["used"] <= (weight > 0).sum()
    early = host(mesh.register(dev(src), dev(verts), dev(faces), model="similarity", iterations=15, tol=1e-6))
    assert early["status"] == "converged" and not icp.mismatches(early, icp.register(src, verts, faces, model="similarity", iterations=15, tol=1e-6))
    timed = mesh.register(dev(src), dev(verts), dev(faces), model="similarity", iterations=3, timing=True)
    assert sorted(timed["times"]) == ["bin", "host", "query", "terms"] and all(t > 0 for t in timed["times"].values())


def test_the_statuses_on_the_gpu():
    verts, faces = icp.flat_square()
    pts = icp.displaced(np.stack([np.linspace(0.1, 0.9, 12), np.linspace(0.9, 0.2, 12) ** 2, np.zeros(12)], -1).astype(np.float32), 5.0, 1.0)
    v, f = dev(verts), dev(faces)
    for kw in (dict(metric="plane"), dict(metric="point", iterations=3), dict(max_distance=1e-3), dict(model="translation", metric="plane")):
        got, want = host(mesh.register(dev(pts), v, f, **kw)), icp.register(pts, verts, faces, **kw)
        assert not icp.mismatches(got, want), kw
    assert mesh.register(dev(pts), v, f, metric="plane")["status"] == "singular"
    assert mesh.register(dev(pts), v, f, max_distance=1e-3)["status"] == "no_correspondences"
    empty = mesh.register(dev(pts[:0]), v, f)
    assert empty["status"] == "empty" and empty["iterations"] == 0 and empty["history"] == []
    none = mesh.register(dev(pts), v, f[:0])
    assert none["status"] == "no_correspondences" and same(none["moved"].cpu().numpy(), pts)


@pytest.mark.parametrize("name", NAMES)
def test_the_plane_metric_converges_on_the_gpu(name):
    src, truth, _ = icp.source(name)
    res = host(mesh.register(dev(src), *(dev(x) for x in icp.patch()), model=model_of(name), metric="plane", iterations=15))
    print(f"{name}: error {error(res, truth):.3e} after {res['iterations']} iterations, steps {' '.join('%.1e' % h['step'] for h in res['history'])}")
    assert error(res, truth) <= 1e-5


@pytest.mark.parametrize("name", ["rigid5", "rigid10"])
def test_partial_overlap_needs_the_border_rule_on_the_gpu(name):
    src, truth, _ = icp.source(name, 0.9)
    v, f = (dev(x) for x in icp.crop())
    with_rule = host(mesh.register(dev(src), v, f, iterations=30, reject_border=True))
    without = host(mesh.register(dev(src), v, f, iterations=30, reject_border=False, trim=None))
    trimmed = host(mesh.register(dev(src), v, f, iterations=30, reject_border=False, trim=0.7))
    print(f"{name}: border rule {error(with_rule, truth):.3e} ({with_rule['history'][-1]['used']} of {len(src)} used), without "
          f"{error(without, truth):.3e}, trim 0.7 {error(trimmed, truth):.3e} ({trimmed['history'][-1]['used']} used)")
    assert error(with_rule, truth) <= 1e-5 and error(without, truth) > 1e-2 and error(trimmed, truth) <= 1e-5


# ---- register_meshes --------------------------------------------------------------------------------------------------------------------
def test_register_meshes_recovers_a_moved_cube():
    verts, faces = icp.cube()
    moved_verts = icp.displaced(verts, 5.0, 1.0)
    a, fa, b = dev(moved_verts), dev(faces), dev(verts)
    got = host(mesh.register_meshes(a, fa, b, fa, 0.25, iterations=12))
    want = icp.register_meshes(moved_verts, faces, verts, faces, 0.25, iterations=12)
    assert not icp.mismatches(got, want) and same(got["verts"], want["verts"]) and got["n_samples"] == want["n_samples"] == len(got["moved"]) - 8
    s, R, t = icp.known_transform(5.0, 1.0)
    print(f"cube: vertices {np.abs(got['verts'].astype(np.float64) - verts).max():.3e} off, {got['n_samples']} samples, status {got['status']}")
    assert np.abs(got["verts"].astype(np.float64) - verts).max() <= 1e-5
    assert np.abs(got["rotation"] - R).max() < 1e-5 and np.abs(got["translation"] - t).max() < 1e-5
    pts, _, weight = mesh.sample_faces(a, fa, 0.25)
    alone = host(mesh.register(pts, b, fa, weight=weight, iterations=12))                  # the vertices at weight 0 change no sum
    assert alone["matrix"].tobytes() == got["matrix"].tobytes() and [h["rms"] for h in alone["history"]] == [h["rms"] for h in got["history"]]
    tetra_v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], dtype=np.float32)     # unequal faces: unequal weights
    tetra_f = np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], dtype=np.int32)
    tv = icp.displaced(tetra_v, 5.0, 1.0)
    got = host(mesh.register_meshes(dev(tv), dev(tetra_f), dev(tetra_v), dev(tetra_f), 0.3, iterations=4, reject_border=False))
    assert not icp.mismatches(got, icp.register_meshes(tv, tetra_f, tetra_v, tetra_f, 0.3, iterations=4, reject_border=False))
    flat = host(mesh.register(mesh.sample_faces(dev(tv), dev(tetra_f), 0.3)[0], dev(tetra_v), dev(tetra_f), iterations=4, reject_border=False))
    assert flat["history"][0]["rms"] != got["history"][0]["rms"] and flat["matrix"].tobytes() != got["matrix"].tobytes()      # the area weights count


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    verts, faces = icp.patch()
    v, f, p = dev(verts), dev(faces), dev(icp.source("rigid5")[0])
    N = len(p)
    bad_f = faces.copy()
    bad_f[10, 1] = len(verts)
    bad_v = verts.copy()
    bad_v[5, 2] = np.nan
    calls = [lambda: mesh.register(p, v, dev(bad_f)), lambda: mesh.register(p, dev(bad_v), f), lambda: mesh.register(p.double(), v, f),
             lambda: mesh.register(p[:, :2].contiguous(), v, f), lambda: mesh.register(p, v, f.long()), lambda: mesh.register(p.cpu(), v, f),
             lambda: mesh.register(p, v, f, weight=-torch.ones(N, dtype=torch.float64, device=DEV)),
             lambda: mesh.register(p, v, f, weight=torch.ones(N, device=DEV)), lambda: mesh.register(p, v, f, weight=torch.ones(N - 1, dtype=torch.float64, device=DEV)),
             lambda: mesh.register(p, v, f, weight=torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)),
             lambda: mesh.register(p, v, f, trim=0.0), lambda: mesh.register(p, v, f, trim=1.5), lambda: mesh.register(p, v, f, trim=float("nan")),
             lambda: mesh.register(p, v, f, model="affine"), lambda: mesh.register(p, v, f, metric="line"), lambda: mesh.register(p, v, f, max_distance=0.0),
             lambda: mesh.register(p, v, f, grid=0), lambda: mesh.register(p, v, f, iterations=-2), lambda: mesh.register(p, v, f, pivot=(0, np.inf, 0)),
             lambda: mesh.register(p, v, f, init=np.zeros((4, 4))), lambda: mesh.fit_transform(p, p[:-1].contiguous()),
             lambda: mesh.fit_transform(p, p, metric="plane"), lambda: mesh.fit_transform(p, p, normals=p[:-1].contiguous(), metric="plane"),
             lambda: mesh.fit_transform(p, p, model="warp"), lambda: mesh.transform_points(p, float("nan"), np.eye(3), np.zeros(3)),
             lambda: mesh.transform_points(p, 1.0, np.eye(4), np.zeros(3)), lambda: mesh.register_meshes(v, f, v, f, 0.0),
             lambda: mesh.register_meshes(v, f, v, f, 0.5, weight=None)]
    for i, call in enumerate(calls):
        with pytest.raises(lib.MofaError):
            call()
            pytest.fail(f"call {i} was not refused")
    L = lib.load()
    w = torch.ones(N, dtype=torch.float64, device=DEV)
    out = torch.zeros(1, 36, dtype=torch.float64, device=DEV)
    mu = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert L.mofa_icp_terms_reduce(p.data_ptr(), p.data_ptr(), None, None, None, 0, None, 0, w.data_ptr(), N, mu, 1, out.data_ptr(), lib.stream()) != 0
    assert L.mofa_icp_terms_reduce(p.data_ptr(), p.data_ptr(), None, None, None, 0, None, 0, w.data_ptr(), N, mu, 2, out.data_ptr(), lib.stream()) != 0
    assert L.mofa_icp_reduce(out.data_ptr(), 1, 36, out.data_ptr(), lib.stream()) != 0
    assert L.mofa_icp_apply(p.data_ptr(), 0, (C.c_double * 13)(), p.data_ptr(), lib.stream()) != 0

"""Non-rigid mesh registration on the GPU (``mofa_warp_*``, ``mesh.warp_to`` / ``mesh.warp``) against the NumPy restatement
(tests/warp_reference.py; tests/test_warp_reference_cpu.py shows what it catches), everything bit for bit (``dist_reference._same``):

* the per-vertex system and the product with D + alpha L (x) I3, with its fused first-level inner product, on every catalogue mesh, for
  both metrics, with rejected vertices in prescribed patterns (none, all, every other, one whole chunk), handles included, and on strips
  sized at every boundary of the summation (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049);
* the inner product at those sizes, and one inner product and one three-step solve at 1024^2 + 1 vertices: a third level of the sum;
* ``warp_to``: displacement, vertices and the whole solve record — a solve that freezes on its tolerance half-way, one that never
  freezes, a start that is taken up, the vertex without neighbours or weight that keeps d = 0, and a breakdown on a system made by hand;
* ``warp`` on the patch and the cropped patch: vertices, displacement and every history entry, for both metrics, with and without the
  border rule, with handles and with ``max_distance``; the grid changes no byte, two runs give equal bytes, and the CPU test's warp and
  exact-value conditions hold on the GPU's own result;
* an index out of range is counted and writes nothing; bad arguments on device tensors raise ``MofaError``.
"""
import numpy as np
import pytest
import torch

import dist_reference as dist
import icp_reference as icp
import warp_reference as wr
from mofanerf_amd import lib, mesh

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = icp.CHUNK
SIZES = (1, 2, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
BIG = CHUNK * CHUNK + 1
PATTERNS = ("none", "all", "every_other", "one_chunk")
MESHES = [name for name, _ in wr.SOLVER_MESHES] + ["patch", "crop"]
_refs = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return dist._same(got, np.asarray(want))


def reference(scene, **kw):
    """warp_reference.warp on a catalogue scene, computed once per setting and never written to."""
    key = (scene,) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _refs:
        _refs[key] = wr.warp(*wr.scene(scene), **kw)
    return _refs[key]


def host(res):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def pattern_weight(weight, pattern):
    w = np.array(weight, dtype=np.float64)
    if pattern == "all":
        w[:] = 0.0
    elif pattern == "every_other":
        w[::2] = 0.0
    elif pattern == "one_chunk":
        w[:CHUNK] = 0.0
    return w


def catalogue_case(name):
    """(verts, faces, targets, weight, explicit normals or None, closest faces or None, target mesh or (None, None), moved) of a mesh."""
    if name in ("patch", "crop"):
        tv, tf, pv, pf = wr.scene(name)
        moved = wr.apply(tv, 0.01 * np.sin(np.arange(3 * len(tv), dtype=np.float64)).reshape(-1, 3))
        res = dist.brute_force(moved, pv, pf)
        face = res["face"].copy()
        face[::17] = len(pf) + 3                                 # a few faces outside the mesh: rejected by the plane metric, not a fault
        return tv, tf, res["closest"], np.linspace(0.5, 1.5, len(tv)), None, face, (pv, pf), moved
    verts, faces, targets, weight, normals = wr.solver_case(name)
    return verts, faces, targets, weight, normals, None, (None, None), wr.apply(verts, 0.05 * np.cos(np.arange(3 * len(verts), dtype=np.float64)).reshape(-1, 3))


def gpu_system(verts, faces, moved, targets, weight, metric, alpha, pw, normals, face, tmesh, hweight, hpos, K=1, tol=0.0):
    """The system on the GPU through mesh._WarpSolver: (solver, the device tensors that must stay alive)."""
    V = len(verts)
    tv, tf = tmesh
    adj = mesh.vertex_adjacency(dev(faces), V) if len(faces) else None
    graph = (adj["offsets"], adj["neighbours"], int(adj["neighbours"].shape[0])) if adj is not None else mesh._warp_graph(None, V, torch.device(DEV, 0))
    solver = mesh._WarpSolver(V, graph, K, tol, torch.device(DEV, 0))
    keep = [dev(verts), dev(moved), dev(targets), dev(normals), dev(face), dev(tv), dev(tf), dev(weight), dev(hweight), dev(hpos)]
    solver.system(keep[0], keep[1], keep[2], keep[3] if face is None else None, keep[4], keep[5], 0 if tv is None else len(tv), keep[6],
                  0 if tf is None else len(tf), keep[7], keep[8], keep[9], metric, pw, alpha)
    return solver, keep


def gpu_matvec(solver, p, alpha):
    V = solver.V
    n = (V + CHUNK - 1) // CHUNK
    q = torch.full((V, 3), 7.0, dtype=torch.float64, device=DEV)
    partial, bad = torch.empty(n, dtype=torch.float64, device=DEV), torch.full((n,), -1, dtype=torch.int64, device=DEV)
    lib.check(lib.load().mofa_warp_matvec(solver.D.data_ptr(), p.data_ptr(), solver.offsets.data_ptr(), solver.nbr.data_ptr() if solver.E else None,
                                          solver.E, V, alpha, q.data_ptr(), partial.data_ptr(), bad.data_ptr(), lib.stream()), "mofa_warp_matvec")
    return q, partial, bad


def gpu_dot(a, b):
    V = int(a.shape[0])
    n = (V + CHUNK - 1) // CHUNK
    partial = torch.empty(n, 1, dtype=torch.float64, device=DEV)
    lib.check(lib.load().mofa_warp_dot(a.data_ptr(), b.data_ptr(), V, partial.data_ptr(), lib.stream()), "mofa_warp_dot")
    return float(mesh._icp_reduce(partial, n, 1).cpu()[0])


def check_system_and_matvec(case, metric, pattern, handles, alpha=0.7, pw=1e-2):
    verts, faces, targets, weight, normals, face, tmesh, moved = case
    V = len(verts)
    w = pattern_weight(weight, pattern)
    hweight = hpos = None
    if handles:
        hweight, hpos = wr.handle_arrays((np.arange(0, V, 3), (dist.widen(verts)[::3] + 0.25).astype(np.float32), np.linspace(1.0, 3.0, len(range(0, V, 3)))), V)
    adj = wr.adjacency(faces, V)
    want = wr.system(verts, moved, targets, w, adj, metric, alpha, pw, normals=normals if face is None else None, face=face, tverts=tmesh[0],
                     tfaces=tmesh[1], hweight=hweight, hpos=hpos)
    solver, keep = gpu_system(verts, faces, moved, targets, w, metric, alpha, pw, normals, face, tmesh, hweight, hpos)
    got = (solver.D, solver.b, solver.minv, solver.energy)
    bad = [name for name, g, x in zip(("D", "b", "minv", "energy"), got, want) if not same(g, x)]
    assert not bad and int(solver.bad_system.sum()) == 0, (metric, pattern, handles, bad)
    p = np.random.default_rng(V).standard_normal((V, 3)) * 10.0 ** np.random.default_rng(V + 1).integers(-3, 4, (V, 1))
    q, partial, counted = gpu_matvec(solver, dev(p), alpha)
    wq = wr.matvec(want[0], p, adj, alpha)
    assert same(q, wq) and int(counted.sum()) == 0, (metric, pattern, "matvec")
    assert same(partial, icp.chunk_sums(wr.dot_terms(p, wq)[:, None])[:, 0]), (metric, pattern, "first level of p . q")


# ---- system and matvec ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("name", MESHES)
def test_system_and_matvec_equal_the_restatement_on_the_catalogue(name, metric):
    case = catalogue_case(name)
    for pattern in PATTERNS[:3]:                                # (no catalogue mesh holds a whole chunk: "one_chunk" runs on the strips)
        check_system_and_matvec(case, metric, pattern, handles=pattern == "every_other")


@pytest.mark.parametrize("V", SIZES)
def test_system_and_matvec_at_every_boundary_of_the_summation(V):
    verts, faces, targets, weight, normals = wr.solver_case(wr.strip(V))
    moved = wr.apply(verts, np.full((V, 3), 0.03125))
    for metric, pattern in (("plane", "none"), ("point", "every_other"), ("plane", "one_chunk"), ("point", "all")):
        check_system_and_matvec((verts, faces, targets, weight, normals, None, (None, None), moved), metric, pattern, handles=pattern == "one_chunk")


@pytest.mark.parametrize("V", SIZES)
def test_the_inner_product_equals_the_restatement(V):
    rng = np.random.default_rng(V)
    a, b = rng.standard_normal((V, 3)) * 10.0 ** rng.integers(-8, 8, (V, 1)), rng.standard_normal((V, 3))
    assert gpu_dot(dev(a), dev(b)) == wr.dot(a, b)


def test_a_third_level_of_the_sum():
    """1024^2 + 1 vertices: 1025 first-level sums, 2 second-level ones and a third level; one inner product and a solve of three steps."""
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((BIG, 3)) * 10.0 ** rng.integers(-4, 4, (BIG, 1)), rng.standard_normal((BIG, 3))
    assert gpu_dot(dev(a), dev(b)) == wr.dot(a, b)
    verts, faces = wr.strip(BIG)
    targets = (dist.widen(verts) + np.stack([0.1 * np.sin(0.01 * np.arange(BIG)), 0.05 * np.cos(0.003 * np.arange(BIG)), rng.standard_normal(BIG) * 0.02], -1)).astype(np.float32)
    weight = 0.5 + rng.random(BIG)
    want = wr.warp_to(verts, faces, targets, weight, stiffness=2.0, cg_iterations=3, cg_tol=1e-8)
    got = mesh.warp_to(dev(verts), dev(faces), dev(targets), dev(weight), stiffness=2.0, cg_iterations=3, cg_tol=1e-8)
    assert same(got[1], want[1]) and same(got[0], want[0]) and not wr.solve_mismatches(got[2], want[2]) and got[2]["steps"] == 3


# ---- warp_to ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["point", "plane"])
@pytest.mark.parametrize("name", ["strip257", "odd_mesh", "isolated", "strip1", "strip2"])
def test_warp_to_equals_the_restatement(name, metric):
    verts, faces, targets, weight, normals = wr.solver_case(name)
    V = len(verts)
    init = 0.01 * np.cos(np.arange(3 * V, dtype=np.float64)).reshape(V, 3)
    for kw, expect in ((dict(stiffness=1.0, cg_iterations=60, cg_tol=1e-3), "tolerance" if V > 2 else None),       # freezes half-way
                       (dict(stiffness=0.5, cg_iterations=7, cg_tol=0.0), "iterations" if name == "strip257" else None),      # never freezes
                       (dict(stiffness=3.0, cg_iterations=20, cg_tol=1e-8, point_weight=0.25, init=init), None)):
        want = wr.warp_to(verts, faces, targets, weight, normals, metric, **kw)
        g = dict(kw, init=dev(kw["init"])) if "init" in kw else kw
        got = mesh.warp_to(dev(verts), dev(faces), dev(targets), dev(weight), dev(normals), metric, **g)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.float64 and len(got[2]["rho"]) == kw["cg_iterations"] + 1
        assert same(got[1], want[1]) and same(got[0], want[0]) and not wr.solve_mismatches(got[2], want[2]), (name, metric, kw)
        if expect:
            assert got[2]["stop"] == expect and (expect != "tolerance" or 0 < got[2]["steps"] < kw["cg_iterations"] - 1)
            if expect == "tolerance":                           # frozen: the history stays flat from the step that froze
                assert (got[2]["rho"][got[2]["steps"]:] == got[2]["rho"][got[2]["steps"]]).all()
    if name == "isolated":
        _, d, _ = mesh.warp_to(dev(verts), dev(faces), dev(targets), dev(weight), dev(normals), metric, stiffness=1.0)
        assert not d[4].cpu().numpy().any() and d[:4].cpu().numpy().all()      # no neighbour, no weight: d = 0


def test_exact_values_hold_on_the_gpu():
    """stiffness = 0, the point metric, unit weights, one step: a == 1.0 and the warped vertices are the targets bit for bit."""
    for name in ("strip257", "odd_mesh", "tetrahedron"):
        verts, faces, targets, _, _ = wr.solver_case(name)
        out, d, solve = mesh.warp_to(dev(verts), dev(faces), dev(targets), stiffness=0.0, cg_iterations=1)
        assert same(out, targets) and solve["steps"] == 1 and solve["stop"] == "iterations"
        assert np.array_equal(d.cpu().numpy(), dist.widen(targets) - dist.widen(verts))


def test_a_breakdown_freezes_the_solve_at_its_first_step():
    """An indefinite system made by hand (D = -w I, no stiffness): p . q < 0 at step 0 with rho_0 > 0 — the record mesh.warp calls
    "singular" — and x keeps its start's bits."""
    verts, faces, targets, weight, _ = wr.solver_case("tetrahedron")
    adj = wr.adjacency(faces, 4)
    D, b, minv, _ = wr.system(verts, verts, targets, weight, adj, "point", 0.0)
    start = np.full((4, 3), -0.0)
    _, want = wr.cg(-D, b, minv, adj, 0.0, start, 5, 1e-8)
    solver, keep = gpu_system(verts, faces, verts, targets, weight, "point", 0.0, 1e-2, None, None, (None, None), None, None, K=5, tol=1e-8)
    solver.D.neg_()
    x = dev(start)
    solver.solve(0.0, x)
    rho, steps, stop = solver.record("test", solver.tail().cpu().numpy())
    assert (stop, steps) == ("breakdown", 0) == (want["stop"], want["steps"]) and same(rho, want["rho"]) and rho[0] > 0
    assert same(x, start)                                       # (-0.0 stays -0.0: nothing was written)


def test_an_index_out_of_range_is_counted_and_writes_nothing():
    verts, faces, targets, weight, _ = wr.solver_case("strip257")
    solver, keep = gpu_system(verts, faces, verts, targets, weight, "point", 1.0, 1e-2, None, None, (None, None), None, None)
    good_nbr = solver.nbr
    nbr = good_nbr.clone()
    nbr[int(solver.offsets[100])] = 257                         # vertex 100's first neighbour lies one past the mesh
    solver.nbr = nbr
    p = dev(np.random.default_rng(0).standard_normal((257, 3)))
    q, partial, bad = gpu_matvec(solver, p, 1.0)
    assert bad.tolist() == [1] and (q[100] == 7.0).all() and not (q[99] == 7.0).any() and not (q[101] == 7.0).any()
    offsets = solver.offsets.clone()
    offsets[257] = solver.E + 5                                 # the last list runs past the neighbours: it is never read
    solver.offsets, solver.nbr = offsets, good_nbr
    q, partial, bad = gpu_matvec(solver, p, 1.0)
    assert bad.tolist() == [1] and (q[256] == 7.0).all() and not (q[255] == 7.0).any()


# ---- warp -------------------------------------------------------------------------------------------------------------------------------
HANDLES = (np.array([0, 84, 168]), (dist.widen(wr.template()[0])[[0, 84, 168]] + np.array([[0.0, 0.0, 0.3], [0.1, 0.0, -0.3], [0.0, -0.1, 0.2]])).astype(np.float32),
           np.array([50.0, 5.0, 0.5]))
SHORT = dict(stiffness=(1.0, 0.1), iterations=2)
SETTINGS = (("patch", dict(metric="plane")), ("patch", dict(metric="point")), ("crop", dict(metric="plane", **SHORT)),
            ("crop", dict(metric="point", reject_border=False, **SHORT)), ("crop", dict(metric="plane", reject_border=False, max_distance=0.08, **SHORT)),
            ("patch", dict(metric="plane", handles=HANDLES, cg_iterations=30, **SHORT)), ("patch", dict(metric="point", max_distance=0.12, tol=5e-3, iterations=4, stiffness=(1.0, 0.1))))


def gpu_warp(scene, **kw):
    tv, tf, pv, pf = wr.scene(scene)
    if "handles" in kw:
        kw = dict(kw, handles=tuple(dev(h) for h in kw["handles"]))
    return host(mesh.warp(dev(tv), dev(tf), dev(pv), dev(pf), **kw))


@pytest.mark.parametrize("scene,kw", SETTINGS, ids=[f"{s}-{i}" for i, (s, _) in enumerate(SETTINGS)])
def test_warp_equals_the_restatement(scene, kw):
    want = reference(scene, **kw)
    got = gpu_warp(scene, **kw)
    assert not wr.mismatches(got, want), (kw, wr.mismatches(got, want), got["status"], want["status"])
    assert got["verts"].dtype == np.float32 and got["displacement"].dtype == np.float64 and len(got["grid"]) == 3


def test_the_grid_changes_no_byte_and_two_runs_agree():
    kw = dict(metric="plane", **SHORT)
    runs = [gpu_warp("crop", grid=g, **kw) for g in (1, 7, None, None)]
    assert runs[0]["grid"] == (1, 1, 1) and runs[1]["grid"] == (7, 7, 7)
    for r in runs[1:]:
        assert not wr.mismatches(r, runs[0])
    timed = gpu_warp("crop", timing=True, **kw)
    assert not wr.mismatches(timed, runs[0]) and set(timed["times"]) == {"bin", "query", "system", "solve"} and all(v >= 0 for v in timed["times"].values())


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_it_warps_on_the_gpu(metric):
    """The CPU test's condition on the GPU's own result: the template -> target rms surface distance at most halves (measured by
    mesh.surface_distance at the same spacing)."""
    tv, tf, pv, pf = (dev(a) for a in wr.scene("patch"))
    out = mesh.warp(tv, tf, pv, pf, metric=metric)
    before = mesh.surface_distance(tv, tf, pv, pf, 0.05)["a_to_b"]["rms"]
    after = mesh.surface_distance(out["verts"], tf, pv, pf, 0.05)["a_to_b"]["rms"]
    print(metric, before, "->", after, after / before)
    assert out["status"] == "iterations" and out["iterations"] == 15 and after <= 0.5 * before


def test_statuses_on_the_gpu():
    tv, tf, pv, pf = wr.scene("patch")
    out = gpu_warp("patch", iterations=0)
    assert out["status"] == "iterations" and out["iterations"] == 0 and same(out["verts"], tv) and not out["displacement"].any()
    out = host(mesh.warp(dev(tv[:0]), dev(tf[:0]), dev(pv), dev(pf)))
    assert out["status"] == "empty" and out["verts"].shape == (0, 3) and out["history"] == []
    out = host(mesh.warp(dev(tv), dev(tf), dev(pv), dev(pf[:0])))
    assert out["status"] == "no_correspondences" and same(out["verts"], tv)
    flat = dist.square(4)
    side = (tv * np.float32(0.25) + np.array([3.0, 0.5, 0.0], dtype=np.float32)).astype(np.float32)
    for kw in ({}, {"max_distance": 0.5}):
        want = wr.warp(side, tf, *flat, **kw)
        got = host(mesh.warp(dev(side), dev(tf), dev(flat[0]), dev(flat[1]), **kw))
        assert got["status"] == "no_correspondences" and not wr.mismatches(got, want)
    init = 0.02 * np.sin(np.arange(3 * len(tv), dtype=np.float64)).reshape(-1, 3)
    want = wr.warp(tv, tf, pv, pf, init=init, **SHORT)
    got = host(mesh.warp(dev(tv), dev(tf), dev(pv), dev(pf), init=dev(init), **SHORT))
    assert not wr.mismatches(got, want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_on_device_tensors_raise():
    tv, tf, pv, pf = (dev(a) for a in wr.scene("patch"))
    V = tv.shape[0]
    bad_faces = tf.clone()
    bad_faces[3, 1] = V
    nan_verts = tv.clone()
    nan_verts[5, 2] = float("nan")
    w = torch.ones(V, dtype=torch.float64, device=DEV)
    idx, pos = torch.tensor([1, 2], device=DEV), tv[:2].clone()
    for call, match in ((lambda: mesh.warp(tv, bad_faces, pv, pf), "outside"), (lambda: mesh.warp(nan_verts, tf, pv, pf), "non-finite"),
                        (lambda: mesh.warp(tv, tf, nan_verts, tf), "not finite"), (lambda: mesh.warp(tv, tf, pv, bad_faces[:, :2]), "faces"),
                        (lambda: mesh.warp(tv.double(), tf, pv, pf), "float32"), (lambda: mesh.warp(tv, tf.long(), pv, pf), "int32"),
                        (lambda: mesh.warp(tv, tf, pv, pf, weight=-w), ">= 0"), (lambda: mesh.warp(tv, tf, pv, pf, weight=w[:5]), "weight"),
                        (lambda: mesh.warp(tv, tf, pv, pf, weight=w.float()), "float64"), (lambda: mesh.warp(tv, tf, pv, pf, init=w), "init"),
                        (lambda: mesh.warp(tv, tf, pv, pf, init=torch.full((V, 3), float("inf"), dtype=torch.float64, device=DEV)), "finite"),
                        (lambda: mesh.warp(tv, tf, pv, pf, handles=(torch.tensor([1, V], device=DEV), pos, 1.0)), "outside"),
                        (lambda: mesh.warp(tv, tf, pv, pf, handles=(torch.tensor([1, 1], device=DEV), pos, 1.0)), "repeated"),
                        (lambda: mesh.warp(tv, tf, pv, pf, handles=(idx, pos * float("nan"), 1.0)), "finite"),
                        (lambda: mesh.warp(tv, tf, pv, pf, handles=(idx, pos, -1.0)), "finite"),
                        (lambda: mesh.warp(tv, tf, pv, pf, handles=(idx.cpu(), pos, 1.0)), "on the GPU"),
                        (lambda: mesh.warp(tv, tf, pv, pf, handles=(idx, pos[:1], 1.0)), "positions"),
                        (lambda: mesh.warp(tv, tf, pv, pf, grid=300), "grid"), (lambda: mesh.warp(tv, tf, pv, pf, stiffness=()), "stiffness"),
                        (lambda: mesh.warp_to(tv, tf, pv), "targets"), (lambda: mesh.warp_to(tv, tf, tv, metric="plane"), "normals"),
                        (lambda: mesh.warp_to(tv, tf, tv, normals=pv, metric="plane"), "normals"), (lambda: mesh.warp_to(tv, bad_faces, tv), "outside"),
                        (lambda: mesh.warp_to(tv, tf, tv, weight=-w), ">= 0"), (lambda: mesh.warp_to(tv, tf, tv.cpu()), "on the GPU")):
        with pytest.raises(lib.MofaError, match=match):
            call()

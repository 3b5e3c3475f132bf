"""The as-rigid-as-possible stiffness on the GPU (``mofa_warp_rotations`` / ``mofa_warp_arap_rhs``, ``mesh.warp(stiffness_model="arap")``,
``mesh.deform``) against the NumPy restatement (tests/arap_reference.py; tests/test_arap_reference_cpu.py shows what it catches), everything
bit for bit (``dist_reference._same``):

* the rotations, the fit, both counters and the amended right-hand side on the whole neighbourhood catalogue (rest poses, exact rigid
  motions up to 180 degrees, flat and one-edge neighbourhoods, the vertex without neighbours, mirrored neighbourhoods, coordinates scaled by
  1e-6 and 1e6, non-finite displacements, noisy fields) and on strips sized at every boundary of the launch and of the two-level sum
  (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049), with ``arap_energy`` at those sizes;
* an index out of range is counted and writes the identity / leaves b alone;
* ``deform`` on the patch with its ring of border handles and with five handles, and ``warp(stiffness_model="arap")`` on the patch and the
  cropped patch: vertices, displacement, rotations and every history entry, for both metrics, with and without handles, the border rule
  and ``max_distance``; the grid changes no byte, two runs give equal bytes, and the CPU test's two conditions hold on the GPU's own result;
* ``warp`` without the new argument equals ``stiffness_model="displacement"`` byte for byte; bad arguments raise ``MofaError``.
"""
import numpy as np
import pytest
import torch

import arap_reference as ar
import dist_reference as dist
import icp_reference as icp
import warp_reference as wr
from mofanerf_amd import lib, mesh

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = icp.CHUNK
SIZES = (1, 2, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
KINDS = ("rest", "noisy", "rigid", "mirrored", "scaled", "non_finite")
_refs = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return dist._same(got, np.asarray(want))


def host(res):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def gpu_arap(verts, faces):
    """mesh._WarpArap on a mesh: (the buffers, the device tensors that must stay alive)."""
    V = len(verts)
    adj = mesh.vertex_adjacency(dev(faces), V) if len(faces) else None
    graph = (adj["offsets"], adj["neighbours"], int(adj["neighbours"].shape[0])) if adj is not None else mesh._warp_graph(None, V, torch.device(DEV, 0))
    arap = mesh._WarpArap(V, graph, torch.device(DEV, 0))
    arap.R.fill_(7.0), arap.fit.fill_(7.0), arap.bad_fit.fill_(-1), arap.bad_rhs.fill_(-1)
    return arap, [dev(verts)]


def check_kernels(verts, faces, d, alpha=0.7):
    V = len(verts)
    adj = wr.adjacency(faces, V)
    R, fit, odd = ar.rotations(verts, d, adj)
    arap, keep = gpu_arap(verts, faces)
    fit_sum = arap.rotations(keep[0], dev(d))
    assert same(arap.R, R), "R"
    assert same(arap.fit, fit), "fit"
    assert arap.bad_fit.sum(0).tolist() == [0, odd], ("counters", arap.bad_fit.sum(0).tolist(), odd)
    b = np.random.default_rng(V).standard_normal((V, 3)) * 10.0 ** np.random.default_rng(V + 1).integers(-3, 4, (V, 1))
    gb = dev(b)
    arap.amend(keep[0], alpha, gb)
    assert same(gb, ar.arap_rhs(verts, R, adj, alpha, b)) and int(arap.bad_rhs.sum()) == 0, "right-hand side"
    assert arap.energy("test", arap.tail(fit_sum).cpu().numpy()) == ar.energy(fit), "arap_energy"
    return arap


# ---- the two kernels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_rotations_and_right_hand_side_equal_the_restatement_on_the_catalogue(kind):
    names = [n for n in ar.catalogue() if n.split("/")[0] == kind]
    assert names
    for name in names:
        verts, faces, d, _ = ar.catalogue()[name]
        try:
            arap = check_kernels(verts, faces, d)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None
        if kind == "rest":                                       # the exact-identity property on the GPU's own bytes
            assert same(arap.R, np.tile(ar.IDENTITY, (len(verts), 1))) and not arap.fit.cpu().numpy().any()


@pytest.mark.parametrize("V", SIZES)
def test_rotations_energy_and_right_hand_side_at_every_boundary(V):
    verts, faces, targets, _, _ = wr.solver_case(wr.strip(V))
    check_kernels(verts, faces, dist.widen(targets) - dist.widen(verts))
    check_kernels(verts, faces, np.zeros((V, 3)), alpha=0.0)


def test_an_index_out_of_range_is_counted_and_writes_the_identity():
    verts, faces, targets, _, _ = wr.solver_case("strip257")
    d = dist.widen(targets) - dist.widen(verts)
    adj = wr.adjacency(faces, 257)
    R, fit, _ = ar.rotations(verts, d, adj)
    arap, keep = gpu_arap(verts, faces)
    good_nbr, good_offsets = arap.nbr, arap.offsets
    nbr = good_nbr.clone()
    nbr[int(arap.offsets[100]) + 1] = 257                       # vertex 100's second neighbour lies one past the mesh
    arap.nbr = nbr
    arap.rotations(keep[0], dev(d))
    got = arap.R.cpu().numpy()
    assert arap.bad_fit.tolist() == [[1, 0], [0, 0]] and np.array_equal(got[100], ar.IDENTITY) and float(arap.fit[100]) == 0.0
    assert same(np.delete(got, 100, 0), np.delete(R, 100, 0)) and same(np.delete(arap.fit.cpu().numpy(), 100), np.delete(fit, 100))
    b = np.random.default_rng(3).standard_normal((257, 3))
    want = ar.arap_rhs(verts, got, adj, 2.0, b)
    gb = dev(b)
    arap.amend(keep[0], 2.0, gb)
    assert arap.bad_rhs.tolist() == [1, 0] and same(gb[100], b[100]) and same(np.delete(gb.cpu().numpy(), 100, 0), np.delete(want, 100, 0))
    offsets = good_offsets.clone()
    offsets[257] = arap.E + 5                                   # the last list runs past the neighbours: it is never read
    arap.offsets, arap.nbr = offsets, good_nbr
    arap.rotations(keep[0], dev(d))
    assert arap.bad_fit.tolist() == [[0, 0], [1, 0]] and np.array_equal(arap.R[256].cpu().numpy(), ar.IDENTITY) and same(arap.R[:256], R[:256])
    gb = dev(b)
    arap.amend(keep[0], 2.0, gb)
    assert arap.bad_rhs.tolist() == [0, 1] and same(gb[256], b[256])


# ---- deform -----------------------------------------------------------------------------------------------------------------------------
def gpu_handles(handles):
    index, pos, hw = handles
    return dev(index), dev(pos), (hw if np.isscalar(hw) else dev(hw))


DEFORMS = (("border", {}), ("five", dict(iterations=6, stiffness=2.5, cg_iterations=25)), ("five", dict(iterations=8, tol=0.05)),
           ("five", dict(iterations=3, cg_tol=0.0, cg_iterations=12, init=True)))


@pytest.mark.parametrize("which,kw", DEFORMS, ids=[f"{w}-{i}" for i, (w, _) in enumerate(DEFORMS)])
def test_deform_equals_the_restatement(which, kw):
    verts, faces, handles, truth = ar.deform_scene(which)
    if which == "five":
        handles = (handles[0], handles[1], np.array([4.0, 1.0, 0.5, 2.0, 0.0]))
    gkw = dict(kw)
    if kw.get("init"):
        kw = dict(kw, init=0.01 * np.sin(np.arange(3 * len(verts), dtype=np.float64)).reshape(-1, 3))
        gkw = dict(kw, init=dev(kw["init"]))
    want = ar.deform(verts, faces, handles, **kw)
    got = host(mesh.deform(dev(verts), dev(faces), gpu_handles(handles), **gkw))
    assert not ar.mismatches(got, want), (kw, ar.mismatches(got, want), got["status"], want["status"])
    assert got["verts"].dtype == np.float32 and got["rotations"].shape == (len(verts), 3, 3) and got["rotations"].dtype == np.float64
    if "tol" in kw:
        assert got["status"] == "converged" and 1 < got["iterations"] < 8
    if which == "border":                                       # the CPU test's condition on the GPU's own result
        base = mesh.warp_to(dev(verts), dev(faces), dev(truth.astype(np.float32)), dev(np.isin(np.arange(len(verts)), handles[0]).astype(np.float64)), stiffness=1.0)[0]
        assert ar.deform_condition(got, verts, faces, handles, truth, base.cpu().numpy())
        again = host(mesh.deform(dev(verts), dev(faces), gpu_handles(handles)))
        assert not ar.mismatches(again, got)
    else:
        energies = [h["arap_energy"] for h in got["history"]]
        assert all(b <= a for a, b in zip(energies[1:], energies[2:])) or "init" in kw


def test_deform_statuses_on_the_gpu():
    verts, faces, handles, _ = ar.deform_scene("five")
    out = host(mesh.deform(dev(verts), dev(faces), gpu_handles(handles), iterations=0))
    assert out["status"] == "iterations" and out["iterations"] == 0 and np.array_equal(out["verts"], verts) and out["history"] == []
    assert np.array_equal(out["rotations"], np.tile(np.eye(3), (81, 1, 1)))
    empty = (dev(np.zeros(0, dtype=np.int64)), dev(np.zeros((0, 3), dtype=np.float32)), 1.0)
    out = host(mesh.deform(dev(verts[:0]), dev(faces[:0]), empty))
    assert out["status"] == "empty" and out["rotations"].shape == (0, 3, 3) and out["verts"].shape == (0, 3)
    rest = (handles[0], verts[handles[0]], 1.0)
    out = host(mesh.deform(dev(verts), dev(faces), gpu_handles(rest), iterations=2))
    assert not out["displacement"].any() and all(h["arap_energy"] == 0.0 for h in out["history"])
    verts, faces = wr.isolated()                                # the vertex without neighbours or handle keeps its start
    want = ar.deform(verts, faces, (np.array([0, 2]), (verts[[0, 2]] + np.float32(0.5)), 1.0), iterations=3)
    got = host(mesh.deform(dev(verts), dev(faces), (dev(np.array([0, 2])), dev(verts[[0, 2]] + np.float32(0.5)), 1.0), iterations=3))
    assert not ar.mismatches(got, want) and not got["displacement"][4].any()


# ---- warp -------------------------------------------------------------------------------------------------------------------------------
HANDLES = (np.array([0, 84, 168]), (dist.widen(wr.template()[0])[[0, 84, 168]] + np.array([[0.0, 0.0, 0.3], [0.1, 0.0, -0.3], [0.0, -0.1, 0.2]])).astype(np.float32),
           np.array([50.0, 5.0, 0.5]))
SHORT = dict(stiffness=(1.0, 0.1), iterations=2)
SETTINGS = (("patch", dict(metric="plane")), ("patch", dict(metric="point", **SHORT)), ("crop", dict(metric="plane", **SHORT)),
            ("crop", dict(metric="point", reject_border=False, **SHORT)), ("crop", dict(metric="plane", reject_border=False, max_distance=0.08, **SHORT)),
            ("patch", dict(metric="plane", handles=HANDLES, cg_iterations=30, **SHORT)), ("patch", dict(metric="point", max_distance=0.12, tol=5e-3, iterations=4, stiffness=(1.0, 0.1))))


def reference(scene, **kw):
    key = (scene,) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _refs:
        _refs[key] = ar.warp(*wr.scene(scene), stiffness_model="arap", **kw)
    return _refs[key]


def gpu_warp(scene, **kw):
    tv, tf, pv, pf = wr.scene(scene)
    if "handles" in kw:
        kw = dict(kw, handles=tuple(dev(h) for h in kw["handles"]))
    return host(mesh.warp(dev(tv), dev(tf), dev(pv), dev(pf), **kw))


@pytest.mark.parametrize("scene,kw", SETTINGS, ids=[f"{s}-{i}" for i, (s, _) in enumerate(SETTINGS)])
def test_warp_with_arap_equals_the_restatement(scene, kw):
    want = reference(scene, **kw)
    got = gpu_warp(scene, stiffness_model="arap", **kw)
    assert not ar.mismatches(got, want), (kw, ar.mismatches(got, want), got["status"], want["status"])
    assert got["rotations"].shape == (169, 3, 3) and got["rotations"].dtype == np.float64 and all("arap_energy" in h for h in got["history"])
    assert got["history"][0]["arap_energy"] == 0.0 and got["history"][-1]["arap_energy"] > 0.0


def test_the_grid_changes_no_byte_and_two_runs_agree():
    kw = dict(metric="plane", stiffness_model="arap", **SHORT)
    runs = [gpu_warp("crop", grid=g, **kw) for g in (1, 7, None, None)]
    assert runs[0]["grid"] == (1, 1, 1) and runs[1]["grid"] == (7, 7, 7)
    for r in runs[1:]:
        assert not ar.mismatches(r, runs[0])
    timed = gpu_warp("crop", timing=True, **kw)
    assert not ar.mismatches(timed, runs[0]) and set(timed["times"]) == {"bin", "query", "system", "arap", "solve"} and all(v >= 0 for v in timed["times"].values())


def test_the_default_model_is_the_displacement_model_byte_for_byte():
    for scene, kw in (("patch", dict(metric="plane", **SHORT)), ("crop", dict(metric="point", handles=HANDLES, **SHORT))):
        plain, named = gpu_warp(scene, **kw), gpu_warp(scene, stiffness_model="displacement", **kw)
        assert set(plain) == set(named) == {"verts", "displacement", "history", "iterations", "status", "grid"}
        assert not wr.mismatches(plain, named) and not wr.mismatches(plain, wr.warp(*wr.scene(scene), **kw))
        assert all(set(h) == {"stiffness", "rms", "used", "rejected", "cg_steps", "rho", "stop", "step"} for h in plain["history"])
        assert set(gpu_warp(scene, timing=True, **kw)["times"]) == {"bin", "query", "system", "solve"}


def test_arap_keeps_the_edge_lengths_on_the_gpu():
    """The CPU test's warp condition on the GPU's own results."""
    verts, faces, pv, pf = ar.rotated_template()
    results = {m: host(mesh.warp(dev(verts), dev(faces), dev(pv), dev(pf), stiffness_model=m)) for m in ("displacement", "arap")}
    assert results["arap"]["status"] == "iterations" and results["arap"]["iterations"] == 15
    assert ar.warp_condition(results, verts, faces)


def test_warp_statuses_with_arap():
    tv, tf, pv, pf = wr.scene("patch")
    out = gpu_warp("patch", iterations=0, stiffness_model="arap")
    assert out["status"] == "iterations" and out["iterations"] == 0 and np.array_equal(out["rotations"], np.tile(np.eye(3), (169, 1, 1)))
    out = host(mesh.warp(dev(tv[:0]), dev(tf[:0]), dev(pv), dev(pf), stiffness_model="arap"))
    assert out["status"] == "empty" and out["rotations"].shape == (0, 3, 3)
    out = host(mesh.warp(dev(tv), dev(tf), dev(pv), dev(pf[:0]), stiffness_model="arap"))
    assert out["status"] == "no_correspondences" and np.array_equal(out["rotations"], np.tile(np.eye(3), (169, 1, 1)))
    flat = dist.square(4)
    side = (tv * np.float32(0.25) + np.array([3.0, 0.5, 0.0], dtype=np.float32)).astype(np.float32)
    want = ar.warp(side, tf, *flat, stiffness_model="arap")
    got = host(mesh.warp(dev(side), dev(tf), dev(flat[0]), dev(flat[1]), stiffness_model="arap"))
    assert got["status"] == "no_correspondences" and not ar.mismatches(got, want) and got["history"][0]["arap_energy"] == 0.0
    init = 0.02 * np.sin(np.arange(3 * len(tv), dtype=np.float64)).reshape(-1, 3)
    want = ar.warp(tv, tf, pv, pf, init=init, stiffness_model="arap", **SHORT)
    got = host(mesh.warp(dev(tv), dev(tf), dev(pv), dev(pf), init=dev(init), stiffness_model="arap", **SHORT))
    assert not ar.mismatches(got, want) and got["history"][0]["arap_energy"] > 0.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise():
    tv, tf, pv, pf = (dev(a) for a in wr.scene("patch"))
    V = tv.shape[0]
    idx, pos = torch.tensor([1, 2], device=DEV), tv[:2].clone()
    bad_faces = tf.clone()
    bad_faces[3, 1] = V
    for call, match in ((lambda: mesh.warp(tv, tf, pv, pf, stiffness_model="rigid"), "stiffness_model"),
                        (lambda: mesh.warp(tv, tf, pv, pf, stiffness_model="ARAP"), "stiffness_model"),
                        (lambda: mesh.warp(tv.cpu(), tf.cpu(), pv, pf, stiffness_model="arap"), "on the GPU"),
                        (lambda: mesh.deform(tv, tf, None), "handles"), (lambda: mesh.deform(tv, tf, (idx, pos, 0.0)), "positive weight"),
                        (lambda: mesh.deform(tv.cpu(), tf.cpu(), (idx, pos, 1.0)), "on the GPU"), (lambda: mesh.deform(tv, tf, (idx.cpu(), pos, 1.0)), "on the GPU"),
                        (lambda: mesh.deform(tv, bad_faces, (idx, pos, 1.0)), "outside"), (lambda: mesh.deform(tv, tf, (torch.tensor([1, V], device=DEV), pos, 1.0)), "outside"),
                        (lambda: mesh.deform(tv, tf, (torch.tensor([1, 1], device=DEV), pos, 1.0)), "repeated"),
                        (lambda: mesh.deform(tv, tf, (idx, pos, 1.0), stiffness=(1.0, 2.0)), "one value"),
                        (lambda: mesh.deform(tv, tf, (idx, pos, 1.0), init=torch.zeros(V, 3, device=DEV)), "init"),
                        (lambda: mesh.deform(tv.double(), tf, (idx, pos, 1.0)), "float32")):
        with pytest.raises(lib.MofaError, match=match):
            call()

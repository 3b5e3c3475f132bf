"""The restatement of the mesh smoothing (tests/smooth_reference.py) judged on the CPU: exact values on an octahedron, a regular
tetrahedron and an open patch; on the staircase mesh of a thresholded ball, Taubin smoothing lowers the radial noise without shrinking the
volume while plain Laplacian smoothing shrinks it; every injected fault changes an output bit on a mesh the GPU tests use
(tests/test_gpu_smooth.py); and mesh.smooth refuses bad parameters before it touches a GPU."""
import os

import numpy as np
import pytest
import torch

import mt_reference as mt
import smooth_reference as sr
from mofanerf_amd import lib, mesh

SMOOTH_NAMES = ("mofa_smooth_corner_cots", "mofa_smooth_edge_weights", "mofa_smooth_step")
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mofanerf_hip.h")


@pytest.fixture(autouse=True)
def the_feature_exists():
    for name in ("smooth", "vertex_adjacency"):
        assert callable(getattr(mesh, name, None)) and name in mesh.__all__, name
    assert all(n in lib.SIGNATURES for n in SMOOTH_NAMES)
    with open(HEADER) as fh:
        header = fh.read()
    assert all(f"int {n}(" in header for n in SMOOTH_NAMES) and "MOFA_SMOOTH_COUNTS" in header
    assert lib.ABI_VERSION == 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_octahedron_one_laplacian_pass_halves_it():
    verts, faces = sr.octahedron()
    adj = sr.adjacency(faces, 6)
    assert adj["offsets"].tolist() == [0, 4, 8, 12, 16, 20, 24] and adj["degree_max"] == 4
    assert adj["neighbours"].tolist() == [2, 3, 4, 5, 2, 3, 4, 5, 0, 1, 4, 5, 0, 1, 4, 5, 0, 1, 2, 3, 0, 1, 2, 3]
    assert not adj["boundary"].any() and adj["edges_nonmanifold"] == 0
    for weights in ("uniform", "cotangent"):
        out, stats = sr.smooth(verts, faces, iterations=1, lam=0.5, mu=None, weights=weights)
        assert np.array_equal(bits(out), bits(np.float32(0.5) * verts)), weights
        assert stats["passes"] == 1 and stats["max_displacement"] == 0.5 and np.array_equal(stats["displacement"], np.full(6, 0.5, np.float32))


def test_regular_tetrahedron_weights_are_equal_and_symmetric():
    verts, faces = sr.tetrahedron()
    adj = sr.adjacency(faces, 4)
    cots, flat = sr.corner_cots(verts, faces)
    w, negative = sr.edge_weights(cots, adj)
    assert flat == 0 and negative == 0 and len(w) == 12 and len(set(w.tolist())) == 1
    assert abs(w[0] - 1 / np.sqrt(3)) < 1e-15                                   # two angles of 60 degrees: 2 * 0.5 * cot(60)
    verts, faces = sr.mt_sphere(9, False)                                        # symmetric bit for bit on a mesh with unequal weights too
    adj = sr.adjacency(faces, len(verts))
    w, _ = sr.edge_weights(sr.corner_cots(verts, faces)[0], adj)
    i = np.repeat(np.arange(len(verts)), np.diff(adj["offsets"]))
    table = {(int(a), int(b)): x for a, b, x in zip(i, adj["neighbours"], w)}
    assert len(set(w.tolist())) > 10 and all(table[b, a] == x for (a, b), x in table.items())


def test_grid_patch_boundary_fixed_and_free():
    verts, faces = sr.grid_patch(9, 9)
    adj = sr.adjacency(faces, 81)
    I, J = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    edge = ((I == 0) | (I == 8) | (J == 0) | (J == 8)).reshape(-1)
    assert np.array_equal(adj["boundary"], edge) and edge.sum() == 32
    for weights in ("uniform", "cotangent"):
        fixed, fs = sr.smooth(verts, faces, iterations=3, weights=weights, boundary="fixed")
        free, rs = sr.smooth(verts, faces, iterations=3, weights=weights, boundary="free")
        assert np.array_equal(bits(fixed)[edge], bits(verts)[edge]) and (bits(fixed)[~edge] != bits(verts)[~edge]).any(1).all()
        assert (bits(free)[edge] != bits(verts)[edge]).any(1).all()
        assert fs["n_pinned"] == 32 and rs["n_pinned"] == 0 and fs["n_boundary"] == rs["n_boundary"] == 32
        assert (fs["displacement"][edge] == 0).all() and (rs["displacement"][edge] > 0).all()
    pinned = np.zeros(81, dtype=bool)
    pinned[40] = True
    out, stats = sr.smooth(verts, faces, iterations=2, boundary="free", pinned=pinned)
    assert np.array_equal(bits(out)[40], bits(verts)[40]) and stats["n_pinned"] == 1


def test_the_odd_mesh_keeps_what_has_no_neighbours():
    verts, faces = sr.odd_mesh()
    adj = sr.adjacency(faces, 7)
    assert np.diff(adj["offsets"]).tolist() == [4, 3, 3, 3, 0, 1, 0] and adj["edges_nonmanifold"] == 3 and not adj["boundary"].any()
    assert adj["neighbours"][:4].tolist() == [1, 2, 3, 5] and adj["neighbours"][-1] == 0
    out, stats = sr.smooth(verts, faces, iterations=2, weights="cotangent")
    assert np.array_equal(bits(out)[[4, 6]], bits(verts)[[4, 6]]) and stats["n_isolated"] == 2
    assert stats["flat_corners"] == 6                                            # the three corners of (0, 0, 5) and of (6, 6, 6)
    assert stats["zero_weight"] == 1 and np.array_equal(bits(out)[5], bits(verts)[5])       # vertex 5: its only weight is that of a flat face


def test_taubin_smooths_the_staircase_without_shrinking_it():
    """Measured with this restatement: radial std 0.03056 -> 0.01951 uniform (0.638 x), -> 0.02328 cotangent (0.762 x); volume ratio
    1.0062 / 1.0041; plain Laplacian 0.9001; 240 of 7,560 directed weights negative before the clamp."""
    verts, faces = sr.mt_sphere(17, binary=True)
    adj = sr.adjacency(faces, len(verts))
    assert (len(verts), len(faces), adj["degree_max"], len(adj["neighbours"])) == (1262, 2520, 8, 7560)
    assert mt.is_closed_oriented_manifold(faces) and not adj["boundary"].any() and adj["edges_nonmanifold"] == 0
    std0, vol0 = sr.radial_std(verts), mt.signed_volume(verts, faces)
    for weights, bound in (("uniform", 0.70), ("cotangent", 0.85)):
        out, stats = sr.smooth(verts, faces, iterations=10, lam=0.5, mu=-0.53, weights=weights)
        std, vol = sr.radial_std(out), mt.signed_volume(out, faces)
        print(f"{weights}: radial std {std0:.5f} -> {std:.5f} ({std / std0:.3f} x), volume ratio {vol / vol0:.4f}, "
              f"{stats['negative_weights']} of {len(adj['neighbours'])} weights negative, max displacement {stats['max_displacement']:.4f}")
        assert std < bound * std0
        assert 0.99 <= vol / vol0 <= 1.02
        assert stats["flat_corners"] == 0 and stats["zero_weight"] == 0 and stats["passes"] == 20
        assert stats["negative_weights"] == (240 if weights == "cotangent" else 0)
    out, stats = sr.smooth(verts, faces, iterations=10, lam=0.5, mu=None)
    vol = mt.signed_volume(out, faces)
    print(f"laplacian: volume ratio {vol / vol0:.4f}, radial std {sr.radial_std(out):.5f}")
    assert vol < 0.92 * vol0 and stats["passes"] == 10


# the mesh of sr.MESHES on which each fault shows, and the call it shows in
FAULT_SHOWS = {
    # an interior edge is listed twice, a border edge once: a free border vertex weighs its inner neighbours double.  (Where every edge
    # of a vertex is listed twice the mean is the same up to rounding: with the border fixed no fp32 bit of this patch changes.)
    "no_dedup": ("grid_patch", dict(weights="uniform", boundary="free")),
    # fp64 sums of fp32 differences are exact on ordinary meshes (29 spare bits) and the weighted ones differ by an fp64 ulp that the
    # rounding to fp32 hides: on no other mesh here, with either weights, does the order change a bit.  Heights that span 2^40 show it.
    "reversed_order": ("wide_fan", dict(weights="uniform")),
    "self_loops": ("odd_mesh", dict(weights="uniform")),              # (0, 0, 5): vertex 0 becomes its own neighbour, deg 5 instead of 4
    "no_division": ("octahedron", dict(weights="uniform")),
    "skip_mu": ("octahedron", dict(weights="uniform")),
    "in_place": ("grid_patch", dict(weights="uniform")),
    "fp32_accumulate": ("mt_sphere_binary", dict(weights="uniform")),
    "wrong_corner": ("grid_patch", dict(weights="cotangent")),
    "no_clamp": ("mt_sphere_binary", dict(weights="cotangent")),      # 240 of its 7,560 directed weights are negative before the clamp
    "boundary_free": ("grid_patch", dict(weights="uniform")),         # the patch's 32 border vertices move
}


@pytest.mark.parametrize("fault", sr.FAULTS)
def test_every_injected_fault_changes_an_output_bit(fault):
    name, kw = FAULT_SHOWS[fault]
    verts, faces = dict(sr.MESHES)[name]()
    good, _ = sr.smooth(verts, faces, iterations=2, **kw)
    bad, _ = sr.smooth(verts, faces, iterations=2, fault=fault, **kw)
    changed = int((bits(good) != bits(bad)).any(1).sum())
    print(f"{fault} on {name}: {changed} of {len(verts)} vertices change")
    assert changed > 0
    if fault in ("no_clamp", "boundary_free"):                        # where they cannot show: no negative weight, no boundary
        verts, faces = sr.octahedron()
        assert np.array_equal(bits(sr.smooth(verts, faces, 2, fault=fault, **kw)[0]), bits(sr.smooth(verts, faces, 2, **kw)[0]))


def test_the_set_of_faults_is_the_one_the_table_names():
    assert set(FAULT_SHOWS) == set(sr.FAULTS) and all(n in dict(sr.MESHES) for n, _ in FAULT_SHOWS.values())


@pytest.mark.parametrize("kw, match", [
    (dict(lam=0.0), "lam"), (dict(lam=-0.5), "lam"), (dict(lam=1.5), "lam"), (dict(lam=float("nan")), "lam"), (dict(lam="a"), "lam"),
    (dict(mu=-0.5), "mu"), (dict(mu=0.2), "mu"), (dict(mu=-0.3), "mu"), (dict(mu=float("-inf")), "mu"), (dict(mu=float("nan")), "mu"),
    (dict(lam=1.0, mu=-1.5), "top frequency"), (dict(lam=0.9, mu=-0.95), "top frequency"),
    (dict(weights="cot"), "weights"), (dict(weights=None), "weights"), (dict(boundary="pinned"), "boundary"), (dict(boundary=True), "boundary"),
    (dict(iterations=-1), "iterations"), (dict(iterations=1001), "iterations"), (dict(iterations=2.0), "iterations"),
    (dict(iterations=True), "iterations"), (dict(iterations="3"), "iterations"),
])
def test_bad_parameters_are_refused_before_anything_touches_a_gpu(monkeypatch, kw, match):
    def no_load():
        raise AssertionError("the library was loaded before the parameters were checked")

    monkeypatch.setattr(lib, "load", no_load)
    verts, faces = sr.octahedron()
    with pytest.raises(lib.MofaError, match=match):
        mesh.smooth(torch.from_numpy(verts), torch.from_numpy(faces), **kw)


def test_accepted_parameters_then_cpu_tensors_are_refused(monkeypatch):
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded for CPU tensors")))
    verts, faces = sr.octahedron()
    for kw in (dict(), dict(lam=1.0, mu=None), dict(lam=0.5, mu=-1.0), dict(lam=0.6307, mu=-0.6732), dict(iterations=0), dict(iterations=1000),
               dict(weights="cotangent", boundary="free")):
        with pytest.raises(lib.MofaError, match="GPU"):
            mesh.smooth(torch.from_numpy(verts), torch.from_numpy(faces), **kw)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.vertex_adjacency(torch.from_numpy(faces), 6)

"""The NumPy restatement of the mesh components (tests/cc_reference.py) against scipy's connected components, the pass count of the
emulated hook / compress loop, and — the point of this file — that the comparisons the GPU tests use (``mismatches``,
``compaction_mismatches``) see every plausible wrong kernel: each injected fault below is one a GPU implementation could have."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import cc_reference as cc
import mt_reference as mt


def scipy_labels(V, faces):
    e = cc.edges_of(faces)
    g = sp.coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V))
    return connected_components(g, directed=False)[1]


def referenced_partition(V, faces, labels):
    """scipy gives every unreferenced vertex a component of its own: mark them -1 as the restatement does."""
    ref = np.zeros(V, dtype=bool)
    ref[np.asarray(faces).reshape(-1)] = True
    return np.where(ref, labels, -1)


def check_against_scipy(verts, faces):
    V = len(verts)
    want = cc.components(verts, faces)
    assert cc.same_partition(want["vertex_labels"], referenced_partition(V, faces, scipy_labels(V, faces)))
    parent, passes = cc.emulate(V, faces)
    assert passes <= 16
    assert cc.mismatches(cc.components(verts, faces, root=parent), want) == []        # the emulation's fixed point is the union-find's
    first = [np.flatnonzero(want["vertex_labels"] == c)[0] for c in range(want["n_components"])]
    assert first == sorted(first)                                                     # numbered by smallest vertex index
    return want, passes


@pytest.mark.parametrize("name,res,n_c", [(n, r, c) for (n, r), c in zip(cc.FIELDS, (1, 2, 1))])
def test_fields_equal_scipy(name, res, n_c):
    verts, faces, _, _ = cc.field_mesh(name, res)
    want, passes = check_against_scipy(verts, faces)
    assert want["n_components"] == n_c and want["unreferenced"] == 0 and want["n_faces"].sum() == len(faces)
    pv, pf, _ = cc.permuted(verts, faces, 3)
    _, permuted_passes = check_against_scipy(pv, pf)
    print(f"{name} {res}: {len(verts)} vertices, {n_c} components, {passes} passes in lattice order, {permuted_passes} permuted")
    if name == "two_spheres":
        assert want["n_verts"].tolist() == [3522, 3522]
        assert cc.select(want, "largest").tolist() == [True, False]                   # the tie keeps label 0
        assert (want["volume"] > 0).all()
    total = mt.signed_volume(verts, faces)
    assert abs(want["volume"].sum() - total) <= (len(faces) + 8) * cc.EPS * want["abs_volume"].sum()


@pytest.mark.parametrize("V", cc.STRIPS)
def test_permuted_strips_equal_scipy(V):
    verts, faces = cc.strip(V, V)
    want, passes = check_against_scipy(verts, faces)
    assert want["n_components"] == 1 and want["n_verts"].tolist() == [V]
    print(f"strip of {V}: {passes} passes")
    if V == 100003:
        for numbering in ("identity", "reversed", "zigzag"):
            _, f = cc.strip(V, V, numbering)
            assert cc.emulate(V, f)[1] <= 4, numbering


def test_small_meshes():
    verts, faces = cc.bow_tie()
    want, _ = check_against_scipy(verts, faces)
    assert want["n_components"] == 1
    verts, faces = cc.odd_mesh()
    want, _ = check_against_scipy(verts, faces)
    assert want["n_components"] == 3 and want["unreferenced"] == 4
    assert want["vertex_labels"].tolist() == [-1, 0, -1, 1, 1, 2, 1, 2, 0, 0, -1, 2, 2, -1]
    assert want["face_labels"].tolist() == [0, 1, 2, 0, 2, 1, 2] and want["n_faces"].tolist() == [2, 2, 3]
    assert (want["area"][0] == 0) and (want["area"][1:] > 0).all()
    empty = cc.components(verts, np.zeros((0, 3), dtype=np.int32))
    assert empty["n_components"] == 0 and empty["unreferenced"] == 14 and (empty["vertex_labels"] == -1).all()


def test_hollow_ball_has_a_solid_and_a_cavity():
    grid, lo, step = cc.shell_field((41, 41, 41))
    verts, faces = mt.marching_tets(grid, 0.0, lo, step)
    want, _ = check_against_scipy(verts, faces)
    assert want["n_components"] == 2 and want["volume"][0] > 0 > want["volume"][1]
    shell = 4 / 3 * np.pi * (0.7 ** 3 - 0.35 ** 3)
    assert abs(want["volume"].sum() - shell) < 0.02 * shell


# ---- every injected fault is seen -------------------------------------------------------------------------------------------------------
def two_spheres():
    verts, faces, _, _ = cc.field_mesh(*cc.FIELDS[1])
    return verts, faces


def test_fault_only_the_first_edge_is_hooked():
    verts, faces = cc.bow_tie()
    got = cc.components(verts, faces, root=cc.emulate(len(verts), faces, only_ab=True)[0])
    assert "vertex_labels" in cc.mismatches(got, cc.components(verts, faces))
    verts, faces = two_spheres()                                  # (a closed surface stays connected through its first edges alone:
    got = cc.components(verts, faces, root=cc.emulate(len(verts), faces, only_ab=True)[0])      # the bow-tie is the case that tells)
    assert cc.mismatches(got, cc.components(verts, faces)) == []


def test_fault_one_pass_without_iterating():
    verts, faces = cc.strip(1025, 1025)
    parent, passes = cc.emulate(len(verts), faces, max_passes=1)
    assert passes == 1
    assert "n_components" in cc.mismatches(cc.components(verts, faces, root=parent), cc.components(verts, faces))


def test_fault_hooking_toward_the_larger_root():
    verts, faces = cc.odd_mesh()
    parent, _ = cc.emulate(len(verts), faces, toward_larger=True)
    want = cc.components(verts, faces)
    got = cc.components(verts, faces, root=parent)
    assert cc.same_partition(got["vertex_labels"], want["vertex_labels"])             # the partition is right, the numbering is not
    assert "vertex_labels" in cc.mismatches(got, want)


def test_fault_face_label_from_an_unhooked_copy():
    verts, faces = two_spheres()
    want = cc.components(verts, faces)
    got = dict(want, face_labels=cc.dense_labels(len(verts), faces, np.arange(len(verts)))[1])
    assert cc.mismatches(got, want) == ["face_labels"]


def test_fault_numbering_by_root_value():
    verts, faces = two_spheres()
    want = cc.components(verts, faces)
    root = cc.union_find(len(verts), cc.edges_of(faces))
    got = dict(want, vertex_labels=root.astype(np.int32))
    assert cc.mismatches(got, want) == ["vertex_labels"]


def test_fault_unreferenced_vertices_labelled_zero():
    verts, faces = cc.odd_mesh()
    want = cc.components(verts, faces)
    got = dict(want, vertex_labels=np.maximum(want["vertex_labels"], 0))
    assert cc.mismatches(got, want) == ["vertex_labels"]


def test_fault_volume_without_the_sign_and_area_without_the_half():
    grid, lo, step = cc.shell_field((41, 41, 41))
    verts, faces = mt.marching_tets(grid, 0.0, lo, step)
    want = cc.components(verts, faces)
    assert cc.mismatches(dict(want, volume=want["abs_volume"]), want) == ["volume"]
    assert cc.mismatches(dict(want, area=2 * want["area"]), want) == ["area"]
    # one ulp of a single large term away is still inside the bound; one part in 10^9 of the sum is not
    assert cc.mismatches(dict(want, area=want["area"] * (1 + 2.0 ** -50)), want) == []
    assert cc.mismatches(dict(want, area=want["area"] * (1 + 1e-9)), want) == ["area"]


def test_faults_of_the_compaction():
    verts, faces = cc.odd_mesh()
    stats = cc.components(verts, faces)
    ids = np.arange(len(verts), dtype=np.int64) * 7
    mask = np.array([False, True, True])
    want = cc.compact(verts, faces, stats, mask, ids)
    assert want[1].tolist() == [[1, 3, 0], [6, 2, 4], [5, 4, 6], [3, 1, 0], [4, 4, 4]] and want[2].tolist() == [21, 28, 35, 42, 49, 77, 84]
    assert cc.compaction_mismatches(want, want) == []
    kept = faces[mask[stats["face_labels"]]]
    assert cc.compaction_mismatches((want[0], kept, want[2]), want) == [1]                          # no index remap
    order = np.argsort(stats["vertex_labels"][stats["vertex_labels"] >= 1], kind="stable")          # vertices grouped by component
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    assert cc.compaction_mismatches((want[0][order], inv[want[1]].astype(np.int32), want[2][order]), want) == [0, 1, 2]
    flipped = want[0].copy()
    flipped[2, 1] = -flipped[2, 1] * 0.0 if flipped[2, 1] == 0 else np.nextafter(flipped[2, 1], np.float32(np.inf))
    assert cc.compaction_mismatches((flipped, want[1], want[2]), want) == [0]                       # one bit of one coordinate
    everything = cc.compact(verts, faces, stats, np.ones(3, dtype=bool), ids)
    assert len(everything[0]) == 10                                                                 # unreferenced vertices are dropped
    sv, sf = two_spheres()
    st = cc.components(sv, sf)
    assert cc.compaction_mismatches(cc.compact(sv, sf, st, np.ones(2, dtype=bool)), (sv, sf)) == []  # keeping everything is the identity
    one = cc.compact(sv, sf, st, cc.select(st, "largest"))
    assert len(one[0]) == 3522 and mt.is_closed_oriented_manifold(one[1]) and cc.components(*one)["n_components"] == 1


def test_selection_rules():
    verts, faces = cc.odd_mesh()
    stats = cc.components(verts, faces)
    assert cc.select(stats, "largest").tolist() == [False, False, True]
    assert cc.select(stats, 3).tolist() == [False, False, True] and cc.select(stats, 2).tolist() == [True, True, True]
    assert cc.select(stats, lambda s: s["area"] > 0).tolist() == [False, True, True]
    assert cc.select(stats, [True, False, True]).tolist() == [True, False, True]

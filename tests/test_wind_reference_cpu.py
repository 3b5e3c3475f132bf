"""The restatement of the mesh winding number (tests/wind_reference.py) judged on the CPU: on cubes its integers are the exact half-space
answers, also where rays pass through vertices and edges; on marching-tetrahedra meshes queried at their own lattice points (rays through
mesh vertices and along mesh edges) they are the field's sign; the column walk equals brute force at every grid; every injected fault
changes a winding number on the inputs the GPU tests use (tests/test_gpu_winding.py); the open-edge count and the signed statistics take
their known values."""
import numpy as np
import pytest

import wind_reference as wr
from mofanerf_amd import lib, mesh

WIND_NAMES = ("mofa_wind_bin_count", "mofa_wind_bin_emit", "mofa_wind_query")
GRIDS = (1, 2, 7, 32, (5, 9))
FIELD_NAMES = ("sphere", "two_spheres", "torus", "shell")
N_QUERIES = 600


@pytest.fixture(autouse=True)
def the_feature_exists():
    for name in ("winding_number", "signed_distance", "inside_grid"):
        assert callable(getattr(mesh, name, None)) and name in mesh.__all__, name
    assert all(n in lib.SIGNATURES for n in WIND_NAMES)
    assert lib.ABI_VERSION == 5


@pytest.fixture(scope="module")
def fields():
    """The four analytic meshes with their lattice queries, the field's sign and the pair table of axis 2 (computed once)."""
    out = {}
    for name in FIELD_NAMES:
        verts, faces, queries, truth = wr.field_case(name, N_QUERIES)
        out[name] = dict(verts=verts, faces=faces, queries=queries, truth=truth, pairs=wr.pair_w(queries, verts, faces, 2))
    return out


def test_unit_cube_lattice_on_three_axes():
    verts, faces = wr.cube()
    p, on_surface, inside = wr.cube_queries()
    assert len(p) == 216 and on_surface.sum() == 4 ** 3 - 2 ** 3 and inside.sum() == 8
    for axis in range(3):
        res = wr.brute_force(p, verts, faces, axis)
        assert np.array_equal(res["winding"][~on_surface], inside[~on_surface].astype(np.int32)), axis
        assert res["winding"].dtype == np.int32 and res["crossings"].dtype == np.int32
        assert (res["crossings"][inside] == 1).all() and set(res["crossings"][~on_surface & ~inside]) == {0, 2}      # past the cube, or through it
        assert np.array_equal(res["inside"], res["winding"] != 0)
        assert res["counts"] == {"non_finite_queries": 0, "flat_faces": 8}                 # the four sides parallel to the ray, two faces each


def test_inverted_nested_and_cavity_cubes():
    unit, big = wr.cube(), wr.cube(-0.25, 1.25)
    q = np.array([(0.5, 0.5, 0.5), (0.25, 0.75, 0.5), (-0.125, 0.5, 0.5), (0.5, 1.125, 0.25), (0.5, 0.5, 1.125), (2, 2, 2), (0.5, 0.5, -1),
                  (-0.25, -0.25, -3), (1.0, 1.0, -0.125)], dtype=np.float32)
    for axis in range(3):
        assert wr.brute_force(q, *wr.cube(inward=True), axis)["winding"].tolist() == [-1, -1, 0, 0, 0, 0, 0, 0, 0], axis
        assert wr.brute_force(q, *wr.merged(big, unit), axis)["winding"].tolist() == [2, 2, 1, 1, 1, 0, 0, 0, 1], axis
        assert wr.brute_force(q, *wr.merged(big, wr.cube(inward=True)), axis)["winding"].tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 1], axis
    cavity = wr.brute_force(q, *wr.merged(big, wr.cube(inward=True)), 2)
    assert cavity["crossings"][:2].tolist() == [2, 2] and cavity["inside"][:2].tolist() == [False, False]


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_lattice_queries_take_the_sign_of_the_field(fields, name):
    c = fields[name]
    assert len(c["queries"]) == N_QUERIES and 10 < c["truth"].sum() < N_QUERIES - 10
    assert wr.open_edges(c["faces"]) == 0
    for axis in range(3):
        pairs = c["pairs"] if axis == 2 else None
        res = wr.brute_force(c["queries"], c["verts"], c["faces"], axis, pairs=pairs)
        wrong = int((res["winding"] != c["truth"]).sum())
        print(f"{name}: {len(c['faces'])} faces, axis {axis}: {wrong} of {N_QUERIES} differ from grid > 0")
        assert wrong == 0


def test_the_cavity_of_the_shell_has_winding_zero(fields):
    c = fields["shell"]
    r = np.linalg.norm(c["queries"].astype(np.float64), axis=1)
    res = wr.brute_force(c["queries"], c["verts"], c["faces"], 2, pairs=c["pairs"])
    cavity = r < 0.35
    assert cavity.sum() > 0 and not c["truth"][cavity].any()
    assert (res["winding"][cavity] == 0).all() and (res["crossings"][cavity] >= 2).all() and (res["crossings"][cavity] % 2 == 0).all()


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_every_grid_equals_brute_force(fields, name):
    c = fields[name]
    brute = wr.brute_force(c["queries"], c["verts"], c["faces"], 2, pairs=c["pairs"])
    for g in GRIDS:
        walk = wr.column_walk(c["queries"], c["verts"], c["faces"], g, 2, pairs=c["pairs"])
        assert wr.mismatches(walk, brute) == [], g
        if g == 1:
            assert walk["counts"]["face_tests"] == N_QUERIES * (len(c["faces"]) - brute["counts"]["flat_faces"])
            assert walk["counts"]["max_column"] == len(c["faces"]) - brute["counts"]["flat_faces"]
        else:
            assert 0 < walk["counts"]["face_tests"] < N_QUERIES * len(c["faces"]) // 2


def test_grids_on_the_cubes_with_queries_outside_the_box_and_not_finite():
    verts, faces = wr.merged(wr.cube(-0.25, 1.25), wr.cube(inward=True))
    p = np.concatenate([wr.cube_queries()[0], np.array([(np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (9, 9, 9), (0.5, 0.5, -9)],
                                                       dtype=np.float32)])
    for axis in range(3):
        pairs = wr.pair_w(p, verts, faces, axis)
        brute = wr.brute_force(p, verts, faces, axis, pairs=pairs)
        assert brute["counts"]["non_finite_queries"] == 3 and (brute["winding"][-5:-2] == 0).all() and (brute["crossings"][-5:-2] == 0).all()
        for g in GRIDS:
            assert wr.mismatches(wr.column_walk(p, verts, faces, g, axis, pairs=pairs), brute) == [], (axis, g)


@pytest.mark.parametrize("fault", [f for f in wr.FAULTS if f != "no_range_clamp"])
def test_injected_faults_change_winding_numbers(fields, fault):
    """Each fault is seen on the unit cube's lattice (off the surface), on the inverted cube or on a field's lattice queries."""
    assert fault in wr.FAULTS
    verts, faces = wr.cube()
    p, on_surface, _ = wr.cube_queries()
    seen = {}
    honest = wr.brute_force(p, verts, faces, 2)
    seen["cube"] = int((wr.brute_force(p, verts, faces, 2, faults={fault})["winding"] != honest["winding"])[~on_surface].sum())
    inv = wr.cube(inward=True)
    seen["inverted"] = int((wr.brute_force(p, *inv, 2, faults={fault})["winding"] != wr.brute_force(p, *inv, 2)["winding"])[~on_surface].sum())
    c = fields["two_spheres"]
    got = wr.brute_force(c["queries"], c["verts"], c["faces"], 2, faults={fault})
    seen["two_spheres"] = int((got["winding"] != c["truth"]).sum())
    print(fault, seen)
    assert seen["cube"] + seen["inverted"] > 0 and seen["two_spheres"] > 0
    assert "winding" in wr.mismatches(got, wr.brute_force(c["queries"], c["verts"], c["faces"], 2, pairs=c["pairs"]))


def test_the_range_clamp_decides_a_query_beyond_an_edges_extent():
    verts, faces, q, want = wr.sliver()
    assert np.array_equal(verts.astype(np.float64), [(-2.0 ** 40, 2.0 ** 40, 5), (-2.0 ** 40, -2.0 ** 41, 5), (1 + 2.0 ** -23, 1 + 2.0 ** -23, 5)])
    honest = wr.brute_force(q, verts, faces, 2)
    assert np.array_equal(honest["winding"], want) and honest["crossings"].tolist() == [1, 0]
    # exactly: at u = 1 the upper edge is at v = (1 + e) + e (2^40 - 1 - e) / (2^40 + 1 + e) > 1 and the lower edge at
    # v = (1 + e) - e (2^41 + 1 + e) / (2^40 + 1 + e) < 1, so (1, 1) is inside the face's projection and the ray from z = 0 crosses it
    from fractions import Fraction as Fr
    e, big = Fr(1, 2 ** 23), Fr(2 ** 40)
    upper = (1 + e) - e * ((1 + e) - big) / ((1 + e) + big)
    lower = (1 + e) - e * ((1 + e) + 2 * big) / ((1 + e) + big)
    assert lower < 1 < upper
    faulty = wr.brute_force(q, verts, faces, 2, faults={"no_range_clamp"})
    assert faulty["winding"].tolist() == [0, 0] and "winding" in wr.mismatches(faulty, honest)
    for g in GRIDS:
        assert wr.mismatches(wr.column_walk(q, verts, faces, g, 2), honest) == []


def test_open_edges():
    verts, faces = wr.cube()
    assert wr.open_edges(faces) == 0 and wr.open_edges(wr.merged(wr.cube(-1, 2), wr.cube(inward=True))[1]) == 0
    assert wr.open_edges(faces[1:]) == 3 and wr.open_edges(faces[2:]) == 4          # one triangle gone: its 3 edges; one side gone: its 4
    assert wr.open_edges(np.zeros((0, 3), dtype=np.int32)) == 0
    flipped = faces.copy()
    flipped[0] = flipped[0, ::-1]
    assert wr.open_edges(flipped) == 3                                                # each of its edges twice one way, never the other
    assert wr.open_edges(np.concatenate([faces, faces[:1]])) == 6                     # a doubled face: 2 against 1, seen from both directions


def test_signed_statistics():
    d = np.array([0.25, 0.25, 0.5, 1.0, 2.0, 4.0])
    weight = np.array([1.0, 3.0, 0.0, 4.0, 0.0, 1.0])
    found = np.array([True, True, True, True, True, False])
    inside = np.array([True, True, True, False, False, True])
    st = wr.signed_stats(d, weight, found, inside)
    assert st == {"signed_mean": (4 * -0.25 + 4 * 1.0) / 8, "inside_fraction": 0.5, "max_inside": 0.5, "max_outside": 2.0}
    none = wr.signed_stats(d, weight, found, np.zeros(6, dtype=bool))
    assert np.isnan(none["max_inside"]) and none["max_outside"] == 2.0 and none["inside_fraction"] == 0.0
    assert none["signed_mean"] == (0.25 * 4 + 4.0) / 8

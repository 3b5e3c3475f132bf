"""Mesh winding numbers on the GPU (``mofa_wind_*``, ``mesh.winding_number`` / ``signed_distance`` / ``inside_grid`` /
``surface_distance(signed=True)``) against the NumPy restatement (tests/wind_reference.py):

* ``winding``, ``crossings`` and the grid-independent counters are brute force's, integer for integer (``wind_reference.mismatches``;
  tests/test_wind_reference_cpu.py shows what it catches) on hand-made cubes and on four analytic iso-surfaces queried at their own lattice
  points, on every grid and axis; at one grid the walk's own counters are the restated walk's;
* the same input gives the same bytes, also on another stream;
* ``inside_grid`` of an extraction on its own lattice is ``grid > 0`` wherever ``grid != 0`` and the point is no mesh vertex;
* ``signed_distance`` keeps ``closest_points``' bits and takes its sign from ``inside``; the signed surface distance takes its exact values
  on two cubes, and ``signed=False`` is the dict it always was;
* bad input raises ``MofaError``, a bad index before any other kernel runs.
"""
import numpy as np
import pytest
import torch

import cc_reference as cc
import dist_reference as dr
import mt_reference as mt
import wind_reference as wr
from mofanerf_amd import lib, mesh

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRIDS = (1, 2, 7, 32, None, (5, 9))
WALK_GRID = 7
FIELD_NAMES = ("sphere", "two_spheres", "torus", "shell")
N_QUERIES = 600


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(host(v) for v in x)
    return x.cpu().numpy() if torch.is_tensor(x) else x


def winding(points, verts, faces, **kw):
    return host(mesh.winding_number(dev(np.asarray(points, dtype=np.float32)), dev(verts), dev(faces), **kw))


def check(points, verts, faces, axes=(0, 1, 2), grids=GRIDS, **kw):
    """winding_number equals brute force integer for integer on every axis of ``axes`` and grid of ``grids``, and the restated walk's
    counters at WALK_GRID; returns brute force's records by axis."""
    out = {}
    for axis in axes:
        pairs = wr.pair_w(points, verts, faces, axis)
        want = out[axis] = wr.brute_force(points, verts, faces, axis, pairs=pairs)
        for g in grids:
            got = winding(points, verts, faces, axis=axis, grid=g, **kw)
            assert wr.mismatches(got, want) == [], (axis, g, wr.mismatches(got, want))
        walk = wr.column_walk(points, verts, faces, WALK_GRID, axis, pairs=pairs)
        got = winding(points, verts, faces, axis=axis, grid=WALK_GRID, **kw)
        assert wr.mismatches(got, walk, wr.WALK_COUNTERS) == [], (axis, got["counts"], walk["counts"])
        assert got["grid"] == (WALK_GRID, WALK_GRID)
    return out


# ---- hand-made meshes ------------------------------------------------------------------------------------------------------------------
ODD = np.array([(np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (0.5, 0.5, -np.inf), (9, 9, 9), (0.5, 0.5, -9), (-9, 0.5, 0.5), (0.5, -9, 0.5)],
               dtype=np.float32)


def test_the_unit_cube_on_its_lattice():
    verts, faces = wr.cube()
    p, on_surface, inside = wr.cube_queries()
    want = check(np.concatenate([p, ODD]), verts, faces)
    for axis in range(3):
        assert np.array_equal(want[axis]["winding"][:216][~on_surface], inside[~on_surface].astype(np.int32))
        assert want[axis]["counts"] == {"non_finite_queries": 3, "flat_faces": 8}
    got = winding(p, verts, faces)
    assert got["winding"].dtype == np.int32 and got["crossings"].dtype == np.int32 and got["inside"].dtype == np.bool_
    assert np.array_equal(got["inside"], got["winding"] != 0) and got["open_edges"] == 0 and got["grid"] == (1, 1)


def test_inverted_nested_and_cavity_cubes():
    unit, big = wr.cube(), wr.cube(-0.25, 1.25)
    p = np.concatenate([wr.cube_queries()[0], ODD, np.array([(0.25, 0.75, 0.5), (-0.125, 0.5, 0.5), (1.0, 1.0, -0.125)], dtype=np.float32)])
    for name, (verts, faces), tail in (("inverted", wr.cube(inward=True), [-1, 0, 0]), ("nested", wr.merged(big, unit), [2, 1, 1]),
                                       ("cavity", wr.merged(big, wr.cube(inward=True)), [0, 1, 1])):
        want = check(p, verts, faces)
        for axis in range(3):
            assert want[axis]["winding"][-3:].tolist() == tail, (name, axis)


def test_the_range_clamp_on_the_huge_face():
    verts, faces, q, want = wr.sliver()
    for g in (1, 3, None):
        got = winding(q, verts, faces, grid=g, require_closed=False)
        assert np.array_equal(got["winding"], want) and got["crossings"].tolist() == [1, 0] and got["open_edges"] == 3
    check(q, verts, faces, axes=(2,), require_closed=False)


def test_empty_inputs_launch_nothing(monkeypatch):
    verts, faces = wr.cube()
    monkeypatch.setattr(lib, "check", lambda rc, what: pytest.fail(f"{what} was launched"))
    none = mesh.winding_number(torch.zeros(0, 3, device=DEV), dev(verts), dev(faces))
    assert none["winding"].shape == (0,) and none["winding"].dtype == torch.int32 and none["inside"].dtype == torch.bool
    q = dev(np.concatenate([wr.cube_queries()[0][:10], ODD]))
    for v, f in ((dev(verts), torch.zeros(0, 3, dtype=torch.int32, device=DEV)), (torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV))):
        got = host(mesh.winding_number(q, v, f))
        assert not got["winding"].any() and not got["crossings"].any() and not got["inside"].any() and got["open_edges"] == 0
        assert got["counts"] == {"non_finite_queries": 3, "flat_faces": 0, "face_tests": 0, "max_column": 0}
        assert not mesh.inside_grid(v, f, (3, 4, 5), (0, 0, 0), (1, 1, 1)).any()


# ---- analytic iso-surfaces -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELD_NAMES)
def test_lattice_queries_equal_the_restatement_and_the_field(name):
    verts, faces, queries, truth = wr.field_case(name, N_QUERIES)
    want = check(queries, verts, faces)
    for axis in range(3):
        assert np.array_equal(want[axis]["winding"], truth.astype(np.int32)), axis
    got = winding(queries, verts, faces)
    print(f"{name}: {len(faces)} faces, {len(queries)} queries, default grid {got['grid']}: "
          f"{got['counts']['face_tests'] / len(queries):.1f} faces per query, longest column {got['counts']['max_column']}")
    brute = winding(queries, verts, faces, grid=1)
    n_listed = len(faces) - want[2]["counts"]["flat_faces"]
    assert brute["counts"]["face_tests"] == len(queries) * n_listed and brute["counts"]["max_column"] == n_listed


def test_the_same_input_gives_the_same_bytes():
    verts, faces, queries, _ = wr.field_case("torus", N_QUERIES)
    v, f, q = dev(verts), dev(faces), dev(queries)
    first = host(mesh.winding_number(q, v, f))
    for _ in range(2):
        assert wr.mismatches(host(mesh.winding_number(q, v, f)), first, wr.WALK_COUNTERS) == []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = mesh.winding_number(q, v, f)
    side.synchronize()
    assert wr.mismatches(host(other), first, wr.WALK_COUNTERS) == []


@pytest.mark.parametrize("name", FIELD_NAMES)
def test_inside_grid_round_trip(name):
    """Mesh back to volume at the full lattice: the truth is the field."""
    if name == "shell":
        grid, lo, step = cc.shell_field((21, 21, 21))
        verts, faces = mt.marching_tets(grid, 0.0, lo, step)
    else:
        res = dict(dr.CASES)[name]
        verts, faces, lo, step = cc.field_mesh(name, res)
        grid = mt.field(name, res, lo, step)
    _, keep = wr.lattice_queries(grid, lo, step, verts)
    truth = np.asarray(grid).reshape(-1) > 0
    for axis in range(3):
        inside = mesh.inside_grid(dev(verts), dev(faces), grid.shape, lo, step, axis=axis)
        assert inside.dtype == torch.bool and tuple(inside.shape) == tuple(grid.shape)
        got = inside.cpu().numpy().reshape(-1)
        assert np.array_equal(got[keep], truth[keep]), (axis, int((got[keep] != truth[keep]).sum()))
    chunked = mesh.inside_grid(dev(verts), dev(faces), grid.shape, lo, step, chunk=1000)
    assert torch.equal(chunked, inside)
    print(f"{name}: {grid.size} lattice points, {len(keep)} judged, {int(truth[keep].sum())} inside")


# ---- the signed distance ---------------------------------------------------------------------------------------------------------------
def test_signed_distance_keeps_the_bits_and_follows_inside():
    verts, faces, queries, truth = wr.field_case("sphere", N_QUERIES)
    q = np.concatenate([queries, ODD])
    v, f, p = dev(verts), dev(faces), dev(q)
    plain = host(mesh.closest_points(p, v, f))
    got = host(mesh.signed_distance(p, v, f))
    assert set(got) == set(plain) | {"winding", "inside", "signed_distance"}
    assert dr.mismatches(got, plain, mesh._DIST_COUNTS) == [] and got["grid"] == plain["grid"]
    wind = winding(q, verts, faces)
    assert np.array_equal(got["winding"], wind["winding"]) and np.array_equal(got["inside"], wind["inside"])
    assert np.array_equal(got["inside"][:len(queries)], truth) and got["signed_distance"].dtype == np.float32
    assert got["counts"]["non_finite_queries"] == 3 and np.isnan(got["signed_distance"][len(queries):len(queries) + 3]).all()
    ok = np.isfinite(got["distance"])
    assert np.array_equal(got["signed_distance"][ok], np.where(got["inside"], -got["distance"], got["distance"])[ok]) and ok.sum() == len(q) - 3
    assert (got["signed_distance"][ok][got["inside"][ok]] < 0).all() and (got["signed_distance"][ok][~got["inside"][ok]] > 0).all()
    by_x = host(mesh.signed_distance(p, v, f, axis=0, grid=3))
    assert np.array_equal(by_x["inside"], got["inside"]) and dr.mismatches(by_x, plain) == []
    # a bound: the sphere of radius 0.6 has points deeper than 0.2 and points farther out than 0.2
    bound = host(mesh.signed_distance(p, v, f, max_distance=0.2))
    assert dr.mismatches(bound, host(mesh.closest_points(p, v, f, max_distance=0.2)), mesh._DIST_COUNTS) == []
    far = np.isinf(bound["distance"])
    assert (far & bound["inside"]).sum() > 3 and (far & ~bound["inside"]).sum() > 3
    assert np.isneginf(bound["signed_distance"][far & bound["inside"]]).all() and np.isposinf(bound["signed_distance"][far & ~bound["inside"]]).all()
    assert np.array_equal(bound["signed_distance"][~far & ok], got["signed_distance"][~far & ok])


def distance(a, b, spacing, **kw):
    return host(mesh.surface_distance(dev(a[0]), dev(a[1]), dev(b[0]), dev(b[1]), spacing, **kw))


UNSIGNED_KEYS = {"mean", "rms", "max", "p50", "p95", "n_samples", "n_beyond", "counts", "grid"}
SIGNED_KEYS = {"signed_mean", "inside_fraction", "max_inside", "max_outside", "open_edges"}


def same_value(x, y):
    if isinstance(x, dict):
        return isinstance(y, dict) and set(x) == set(y) and all(same_value(x[k], y[k]) for k in x)
    if isinstance(x, np.ndarray):
        return isinstance(y, np.ndarray) and dr._same(x, y)
    if isinstance(x, float):
        return isinstance(y, float) and (x == y or (np.isnan(x) and np.isnan(y)))
    return type(x) is type(y) and x == y


def test_signed_surface_distance_of_two_cubes(monkeypatch):
    unit, big = wr.cube(), wr.cube(-0.25, 1.25)
    res = distance(unit, big, 0.25, signed=True, samples=True)
    a, b = res["a_to_b"], res["b_to_a"]
    assert set(a) == UNSIGNED_KEYS | SIGNED_KEYS | {"points", "weight", "distance", "face", "inside"}
    print({k: a[k] for k in sorted(SIGNED_KEYS)}, {k: b[k] for k in sorted(SIGNED_KEYS)})
    assert a["inside_fraction"] == 1.0 and a["signed_mean"] == -0.25 and a["max_inside"] == 0.25 and np.isnan(a["max_outside"])
    assert a["mean"] == 0.25 and a["inside"].all() and a["open_edges"] == 0
    assert b["inside_fraction"] == 0.0 and b["signed_mean"] == b["mean"] and np.isnan(b["max_inside"]) and b["max_outside"] == b["max"]
    assert not b["inside"].any() and b["open_edges"] == 0
    want = wr.signed_stats(a["distance"], a["weight"], a["face"] >= 0, a["inside"])
    assert want["signed_mean"] == -0.25 and want["inside_fraction"] == 1.0 and want["max_inside"] == 0.25
    # the default launches nothing new and is the dict it always was: the unsigned keys, the values of the signed call
    seen, real = [], lib.check

    def spy(rc, what):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(lib, "check", spy)
    plain, default = distance(unit, big, 0.25, signed=False), distance(unit, big, 0.25)
    assert seen and not [w for w in seen if w.startswith("mofa_wind")]
    monkeypatch.setattr(lib, "check", real)
    assert set(plain) == {"a_to_b", "b_to_a", "hausdorff", "chamfer"} and same_value(plain, default)
    for name in ("a_to_b", "b_to_a"):
        assert set(plain[name]) == UNSIGNED_KEYS
        assert same_value(plain[name], {k: res[name][k] for k in UNSIGNED_KEYS})
    assert plain["hausdorff"] == res["hausdorff"] and plain["chamfer"] == res["chamfer"]
    ref = dr.surface_distance(unit[0], unit[1], big[0], big[1], 0.25)
    for name in ("a_to_b", "b_to_a"):
        assert all(same_value(float(plain[name][k]), float(ref[name][k])) for k in ("max", "p50", "p95")) and plain[name]["n_samples"] == ref[name]["n_samples"]
    timed = distance(unit, big, 0.25, signed=True, timing=True)
    assert {"a_to_b.winding", "b_to_a.winding"} <= set(timed["times"])
    # an open target is refused by name
    with pytest.raises(lib.MofaError, match="not closed: 3 directed edges"):
        distance(unit, (big[0], big[1][1:].copy()), 0.25, signed=True)
    assert same_value(distance(unit, (big[0], big[1][1:].copy()), 0.25)["a_to_b"]["n_samples"], plain["a_to_b"]["n_samples"])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_a_bad_face_index_is_refused_before_anything_else_runs(monkeypatch):
    verts, faces, queries, _ = wr.field_case("two_spheres", N_QUERIES)
    bad = faces.copy()
    bad[len(bad) // 2, 1] = len(verts)
    seen, real = [], lib.check

    def spy(rc, what):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(lib, "check", spy)
    v, f, q = dev(verts), dev(bad), dev(queries)
    for call in (lambda: mesh.winding_number(q, v, f), lambda: mesh.winding_number(q, v, f, require_closed=False),
                 lambda: mesh.signed_distance(q, v, f), lambda: mesh.inside_grid(v, f, (4, 4, 4), (-1, -1, -1), (0.5, 0.5, 0.5)),
                 lambda: mesh.surface_distance(v, dev(faces), v, f, 0.2, signed=True)):
        del seen[:]
        with pytest.raises(lib.MofaError, match=f"1 of the {3 * len(bad)} face indices lie outside"):
            call()
        assert seen[-1] == "mofa_cc_validate" and not [w for w in seen if w.startswith("mofa_wind")]
    del seen[:]
    with pytest.raises(lib.MofaError):
        mesh.winding_number(q, v, f)
    assert seen == ["mofa_cc_validate"]


def test_bad_input_is_refused(monkeypatch):
    verts, faces, queries, _ = wr.field_case("two_spheres", N_QUERIES)
    v, f, q = dev(verts), dev(faces), dev(queries[:64])
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.winding_number(q.cpu(), v, f)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.winding_number(q, v.cpu(), f)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.winding_number(q, v, f.cpu())
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.inside_grid(v, f.cpu(), (4, 4, 4), (-1, -1, -1), (0.5, 0.5, 0.5))
    with pytest.raises(lib.MofaError, match="int32"):
        mesh.winding_number(q, v, f.long())
    with pytest.raises(lib.MofaError, match="float32"):
        mesh.winding_number(q.double(), v, f)
    with pytest.raises(lib.MofaError, match=r"points \[N,3\]"):
        mesh.winding_number(q[:, :2].contiguous(), v, f)
    bad = verts.copy()
    bad[11, 1] = np.nan
    seen, real = [], lib.check

    def spy(rc, what):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(lib, "check", spy)
    with pytest.raises(lib.MofaError, match="1 of the .* coordinates of the mesh are not finite"):
        mesh.winding_number(q, dev(bad), f)
    assert seen == ["mofa_cc_validate", "mofa_dist_validate"]
    del seen[:]
    opened = dev(faces[3:].copy())
    with pytest.raises(lib.MofaError, match=f"not closed: {wr.open_edges(faces[3:])} directed edges"):
        mesh.winding_number(q, v, opened)
    assert seen == ["mofa_cc_validate", "mofa_dist_validate"]
    monkeypatch.setattr(lib, "check", real)
    with pytest.raises(lib.MofaError, match="not closed"):
        mesh.signed_distance(q, v, opened)
    with pytest.raises(lib.MofaError, match="not closed"):
        mesh.inside_grid(v, opened, (4, 4, 4), (-1, -1, -1), (0.5, 0.5, 0.5))
    got = host(mesh.winding_number(q, v, opened, require_closed=False))
    assert got["open_edges"] == wr.open_edges(faces[3:]) > 0
    assert wr.mismatches(got, wr.brute_force(queries[:64], verts, faces[3:])) == []
    for a in (-1, 3, 1.0, "2", None, True):
        with pytest.raises(lib.MofaError, match="axis"):
            mesh.winding_number(q, v, f, axis=a)
    with pytest.raises(lib.MofaError, match="axis"):
        mesh.signed_distance(q, v, f, axis=3)
    with pytest.raises(lib.MofaError, match="axis"):
        mesh.inside_grid(v, f, (4, 4, 4), (-1, -1, -1), (0.5, 0.5, 0.5), axis=5)
    for g in (0, -3, mesh.WIND_GRID_CAP + 1, (4, 4, 4), (4, 0), 2.5, "7"):
        with pytest.raises(lib.MofaError, match="grid"):
            mesh.winding_number(q, v, f, grid=g)
    with pytest.raises(lib.MofaError, match="resolution"):
        mesh.inside_grid(v, f, (4, 4), (-1, -1, -1), (0.5, 0.5, 0.5))


def test_the_library_refuses_what_mesh_py_never_sends():
    verts, faces = wr.cube()
    v, f, q = dev(verts), dev(faces), dev(wr.cube_queries()[0])
    L = lib.load()
    two = lambda *x: (lib.C.c_double * 2)(*x)
    n_ok, n_big, n_zero = (lib.C.c_int32 * 2)(2, 2), (lib.C.c_int32 * 2)(2, 4097), (lib.C.c_int32 * 2)(0, 2)
    out, crossed = torch.zeros(len(q), dtype=torch.int32, device=DEV), torch.zeros(len(q), dtype=torch.int32, device=DEV)
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    start = torch.zeros(5, dtype=torch.int32, device=DEV)
    per_face = torch.zeros(12, dtype=torch.int64, device=DEV)

    def query(axis=2, n=n_ok, cell=two(1, 1), points=lib.ptr(q), P=0):
        return L.mofa_wind_query(points, len(q), None, lib.ptr(v), 8, f.data_ptr(), 12, axis, two(0, 0), cell, n, start.data_ptr(), None, P,
                                 out.data_ptr(), crossed.data_ptr(), counts.data_ptr(), lib.stream())

    assert query() == 0                                                                # P = 0 with null lists: nothing is read
    torch.cuda.synchronize()
    assert not out.any() and counts.cpu().tolist() == [0, 0, 0, 0]
    for bad in (dict(axis=3), dict(axis=-1), dict(n=n_big), dict(n=n_zero), dict(cell=two(1, 0)), dict(cell=two(np.nan, 1)), dict(points=None),
                dict(P=5)):
        assert query(**bad) != 0 and L.mofa_last_error().decode().startswith("wind_query"), bad
    assert L.mofa_wind_bin_count(lib.ptr(v), f.data_ptr(), 12, 8, 3, two(0, 0), two(1, 1), n_ok, per_face.data_ptr(), counts.data_ptr(), lib.stream()) != 0
    assert L.mofa_wind_bin_count(lib.ptr(v), f.data_ptr(), 12, 8, 2, two(0, 0), two(1, 1), n_ok, None, counts.data_ptr(), lib.stream()) != 0
    assert L.mofa_wind_bin_emit(lib.ptr(v), f.data_ptr(), 12, 8, 2, two(0, 0), two(1, 1), n_big, per_face.data_ptr(), 4, out.data_ptr(), crossed.data_ptr(),
                                lib.stream()) != 0

"""Mesh surface distance on the GPU (``mofa_dist_*``, ``mesh.closest_points`` / ``sample_faces`` / ``surface_distance``,
``Renderer.extract_mesh(simplify_error=)``) against the NumPy restatement (tests/dist_reference.py):

* every output and every grid-independent counter of ``closest_points`` is brute force's bit for bit (``dist_reference.mismatches``;
  tests/test_dist_reference_cpu.py shows what it catches) on hand-made meshes and on three analytic iso-surfaces, at grids 1, 2, 7, 32, the
  default and an anisotropic triple; at one grid the walk's own counters (candidate tests, largest ring) are the restated walk's;
* ``max_distance`` keeps the bits within the bound and gives -1 / inf beyond it;
* ``sample_faces`` is the restatement bit for bit, the metric takes its exact values, and both directions are each other's mirror;
* the same input gives the same bytes, also on another stream; bad input raises ``MofaError``, a bad index before any other kernel runs;
* through the seeded 10 x 1024 network ``simplify_error=True`` fills ``mesh_stats["simplify_error"]`` and its absence changes nothing.
"""
import numpy as np
import pytest
import torch

import dist_reference as dr
import mt_reference as mt
from mofanerf_amd import lib, mesh, synth
from mofanerf_amd.model import NeRF
from mofanerf_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRIDS = (1, 2, 7, 32, None, (5, 1, 9))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(host(v) for v in x)
    return x.cpu().numpy() if torch.is_tensor(x) else x


def closest(points, verts, faces, **kw):
    return host(mesh.closest_points(dev(np.asarray(points, dtype=np.float32)), dev(verts), dev(faces), **kw))


def check(points, verts, faces, grids=(1, 3, None), **kw):
    """closest_points equals brute force bit for bit at every grid of ``grids``; returns brute force's record."""
    want = dr.brute_force(points, verts, faces, **{k: v for k, v in kw.items() if k == "max_distance"})
    for g in grids:
        got = closest(points, verts, faces, grid=g, **kw)
        assert dr.mismatches(got, want) == [], (g, dr.mismatches(got, want))
    return want


@pytest.fixture(scope="module")
def cases():
    """The three analytic iso-surfaces with their queries and brute force's answer (computed once)."""
    out = {}
    for name, _ in dr.CASES:
        verts, faces, queries, _ = dr.case(name)
        pairs = dr.pair_d2(queries, verts, faces)
        out[name] = dict(verts=verts, faces=faces, queries=queries, pairs=pairs, brute=dr.brute_force(queries, verts, faces, pairs=pairs))
    return out


# ---- hand-made meshes ------------------------------------------------------------------------------------------------------------------
TRI = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], dtype=np.float32)


def test_one_triangle_in_all_seven_regions():
    faces = np.array([(0, 1, 2)], dtype=np.int32)
    flat = [(-0.5, -0.5), (1.5, -0.25), (0.5, -0.5), (-0.25, 1.5), (-0.5, 0.5), (1.0, 1.0), (0.25, 0.25),          # A B AB C AC BC inside
            (0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.125, 0.5)]                                 # on vertices, edges, the plane
    q = np.array([(x, y, z) for z in (0.0, 0.75, -0.75) for x, y in flat], dtype=np.float32)
    want = check(q, TRI, faces)
    assert (want["face"] == 0).all()
    n = len(flat)
    assert np.array_equal(want["closest"][:n], want["closest"][n:2 * n]) and np.array_equal(want["d2"][n:2 * n], want["d2"][2 * n:])      # mirrored
    assert want["bary"][:7].tolist() == [[1, 0, 0], [0, 1, 0], [0.5, 0.5, 0], [0, 0, 1], [0.5, 0, 0.5], [0, 0.5, 0.5], [0.5, 0.25, 0.25]]
    assert want["d2"][:7].tolist() == [0.5, 0.3125, 0.25, 0.3125, 0.25, 0.5, 0.0] and (want["d2"][7:n] == 0).all()
    assert np.array_equal(want["distance"][n:n + 7], np.sqrt(np.array([0.5, 0.3125, 0.25, 0.3125, 0.25, 0.5, 0.0]) + 0.5625).astype(np.float32))


def test_ties_go_to_the_lower_index():
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], dtype=np.float32)
    faces = np.array([(0, 1, 2), (1, 3, 2)], dtype=np.int32)
    q = np.array([(0.5, 0.5, 0.5), (0.25, 0.75, -2.0), (0.75, 0.25, 0.0), (1, 0, 0.25), (2.0, -1.0, 0.0)], dtype=np.float32)     # above the shared edge
    assert (check(q, verts, faces, grids=(1, 2, 5, None))["face"] == 0).all()
    assert (check(q, verts, faces[::-1].copy(), grids=(1, 2, 5, None))["face"] == 0).all()
    dup = np.array([(1, 3, 2), (0, 1, 2), (1, 3, 2), (0, 1, 2), (0, 1, 2)], dtype=np.int32)
    want = check(np.array([(0.2, 0.2, 1), (0.9, 0.9, 1), (0.5, 0.5, 0)], dtype=np.float32), verts, dup, grids=(1, 4, None))
    assert want["face"].tolist() == [1, 0, 0]


def test_degenerate_faces_are_skipped_and_counted():
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0.2, 0.2, 0.5), (0.4, 0.4, 0.5), (0.8, 0.8, 0.5)], dtype=np.float32)
    faces = np.array([(3, 4, 5), (0, 1, 2), (3, 3, 4)], dtype=np.int32)
    q = np.array([(0.3, 0.3, 0.45), (0.2, 0.2, 0.5), (5, 5, 5)], dtype=np.float32)
    want = check(q, verts, faces)
    assert (want["face"] == 1).all() and want["counts"]["degenerate_faces"] == 2
    only = closest(q, verts, faces[[0, 2]].copy(), grid=3)
    assert dr.mismatches(only, dr.brute_force(q, verts, faces[[0, 2]])) == []
    assert (only["face"] == -1).all() and np.isposinf(only["distance"]).all() and np.isposinf(only["d2"]).all() and np.isnan(only["closest"]).all()
    assert only["counts"]["degenerate_faces"] == 2 and only["counts"]["candidate_tests"] == 0
    none = closest(q, verts, np.zeros((0, 3), dtype=np.int32))
    assert (none["face"] == -1).all() and np.isposinf(none["distance"]).all()
    empty = mesh.closest_points(torch.zeros(0, 3, device=DEV), dev(verts), dev(faces))
    assert empty["distance"].shape == (0,) and empty["closest"].shape == (0, 3) and empty["face"].dtype == torch.int32


def test_one_huge_triangle_over_many_tiny_ones():
    rng = np.random.default_rng(3)
    c = rng.uniform(-0.9, 0.9, (200, 1, 3))
    tiny = (c + rng.uniform(-0.02, 0.02, (200, 3, 3))).reshape(-1, 3)
    verts = np.concatenate([tiny, [(-2, -2, -1.5), (2.5, -2, 1.0), (-2, 2.5, 1.0)]]).astype(np.float32)
    faces = np.concatenate([[(600, 601, 602)], np.arange(600).reshape(200, 3)]).astype(np.int32)
    q = np.concatenate([rng.uniform(-1.2, 1.2, (300, 3)), c[:50, 0]]).astype(np.float32)
    want = check(q, verts, faces, grids=(1, 8, 32, None))
    assert 30 < (want["face"] == 0).sum() < 330
    got = closest(q, verts, faces, grid=8)
    assert got["counts"]["candidate_tests"] >= len(q)                # the huge face sits in every cell a query starts in


def test_a_single_face():
    q = dr.queries_for(TRI, np.array([(0, 1, 2)], dtype=np.int32), 3, n_random=100, n_each=30)
    check(q, TRI, np.array([(0, 1, 2)], dtype=np.int32), grids=(1, 3, (4, 2, 1), None))


# ---- analytic iso-surfaces -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in dr.CASES])
def test_every_grid_equals_brute_force(cases, name):
    c = cases[name]
    v, f, q = dev(c["verts"]), dev(c["faces"]), dev(c["queries"])
    results = {}
    for g in GRIDS:
        got = host(mesh.closest_points(q, v, f, grid=g))
        results[g] = got
        print(f"{name}: {len(c['faces'])} faces, {len(c['queries'])} queries, grid {got['grid']}: "
              f"{got['counts']['candidate_tests'] / len(c['queries']):.1f} tests per query, largest ring {got['counts']['max_ring']}")
        assert dr.mismatches(got, c["brute"]) == [], (g, dr.mismatches(got, c["brute"]))
    for g in GRIDS[1:]:
        assert dr.mismatches(results[g], results[1]) == []
    assert results[1]["counts"]["candidate_tests"] == len(c["queries"]) * (len(c["faces"]) - 2) and results[1]["counts"]["max_ring"] == 0
    assert results[None]["grid"] == mesh.default_dist_grid(c["verts"].min(0), c["verts"].max(0), len(c["faces"])) != (1, 1, 1)
    b = c["brute"]
    assert (b["d2"] == 0).sum() >= 100 and b["counts"]["degenerate_faces"] == 2 and b["face"].min() >= 2
    assert dr.barycentric_violations(c["verts"], c["faces"], results[None]) == 0


def test_the_walks_own_counters_are_the_restatements(cases):
    c = cases["torus"]
    for g in (7, (5, 1, 9)):
        got = closest(c["queries"], c["verts"], c["faces"], grid=g)
        want = dr.grid_walk(c["queries"], c["verts"], c["faces"], g, pairs=c["pairs"])
        assert dr.mismatches(got, want, dr.WALK_COUNTERS) == []
        assert got["counts"]["skipped_tests"] == 0


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_query_counts(cases, n):
    c = cases["sphere"]
    idx = np.arange(n) * 3 % len(c["queries"])
    want = {k: (v[idx] if k != "counts" else v) for k, v in c["brute"].items()}
    for g in (1, 7, None):
        assert dr.mismatches(closest(c["queries"][idx], c["verts"], c["faces"], grid=g), want) == []


def test_max_distance(cases):
    c = cases["two_spheres"]
    bound = 0.3
    want = dr.brute_force(c["queries"], c["verts"], c["faces"], max_distance=bound, pairs=c["pairs"])
    inside = np.sqrt(c["brute"]["d2"]) <= bound
    assert 50 < inside.sum() < len(inside) - 50
    free = closest(c["queries"], c["verts"], c["faces"], grid=7)
    for g in (1, 7, 32, None):
        got = closest(c["queries"], c["verts"], c["faces"], grid=g, max_distance=bound)
        assert dr.mismatches(got, want) == []
        for k in ("distance", "d2", "face", "closest", "bary"):
            assert dr._same(got[k][inside], c["brute"][k][inside])
        assert (got["face"][~inside] == -1).all() and np.isposinf(got["distance"][~inside]).all()
    got = closest(c["queries"], c["verts"], c["faces"], grid=7, max_distance=bound)
    assert got["counts"]["candidate_tests"] < free["counts"]["candidate_tests"]
    exact = float(np.sqrt(c["brute"]["d2"][inside]).max())            # a bound that equals a distance keeps it
    assert dr.mismatches(closest(c["queries"], c["verts"], c["faces"], max_distance=exact),
                         dr.brute_force(c["queries"], c["verts"], c["faces"], max_distance=exact, pairs=c["pairs"])) == []


# ---- the quadrature and the metric -------------------------------------------------------------------------------------------------------
def test_sample_faces_equals_the_restatement(cases):
    verts, faces = dr.sample_mesh()
    got = host(mesh.sample_faces(dev(verts), dev(faces), 0.25, 8))
    want = dr.sample_faces(verts, faces, 0.25, 8)
    assert dr.sample_mismatches(got, want) == [] and np.bincount(got[1], minlength=5).tolist() == [4, 4, 64, 64, 0]
    assert abs(got[2].sum() - want[3].sum()) <= 1e-14 * want[3].sum()
    assert len(host(mesh.sample_faces(dev(verts[3:6]), dev(faces[:1]), 0.28, 8))[0]) == 1
    c = cases["torus"]
    for spacing, cap in ((0.05, 64), (0.01, 3), (10.0, 1)):
        got = host(mesh.sample_faces(dev(c["verts"]), dev(c["faces"]), spacing, cap))
        want = dr.sample_faces(c["verts"], c["faces"], spacing, cap)
        assert dr.sample_mismatches(got, want) == []
        assert abs(got[2].sum() - want[3].sum()) <= 1e-14 * want[3].sum()
    none = mesh.sample_faces(dev(verts), dev(faces[4:]), 0.25)
    assert none[0].shape == (0, 3) and none[1].shape == (0,) and none[2].dtype == torch.float64


def distance(a, b, spacing, **kw):
    return mesh.surface_distance(dev(a[0]), dev(a[1]), dev(b[0]), dev(b[1]), spacing, **kw)


@pytest.mark.parametrize("n", (1, 3, 8))
def test_parallel_squares(n):
    out = distance(dr.square(n), dr.square(n, z=0.25), 0.1)
    for d in ("a_to_b", "b_to_a"):
        for k in ("mean", "rms", "max", "p50", "p95"):
            assert abs(out[d][k] - 0.25) <= 0.25e-15, (d, k, out[d][k])
        assert out[d]["n_beyond"] == 0
    assert out["hausdorff"] == 0.25 and abs(out["chamfer"] - 0.5) <= 1e-15


def test_a_shifted_square_needs_its_vertices_and_a_mesh_is_at_zero_from_itself():
    a, b = dr.square(2), dr.square(2, shift=(0.125, 0.0))
    full = distance(a, b, 1.0)
    assert full["hausdorff"] == 0.125 == full["a_to_b"]["max"] == full["b_to_a"]["max"]
    blind = distance(a, b, 1.0, vertices=False)
    assert blind["hausdorff"] < 0.125 and full["a_to_b"]["mean"] == blind["a_to_b"]["mean"]
    want = dr.surface_distance(*a, *b, 1.0)
    for d in ("a_to_b", "b_to_a"):
        assert full[d]["n_samples"] == want[d]["n_samples"]
        for k in ("mean", "rms", "max", "p50", "p95"):
            assert abs(full[d][k] - want[d][k]) <= 1e-14 * want[d][k]
    sq = dr.square(4)                                                # exact arithmetic: tests/test_dist_reference_cpu.py says why
    out = distance(sq, sq, 0.1)
    for d in ("a_to_b", "b_to_a"):
        assert all(out[d][k] == 0.0 for k in ("mean", "rms", "max", "p50", "p95")), out[d]
    assert out["hausdorff"] == 0.0 and out["chamfer"] == 0.0


def test_the_two_directions_mirror_each_other_and_the_bound_is_counted(cases):
    a, b = cases["sphere"], cases["torus"]
    A, B = (a["verts"], a["faces"][2:]), (b["verts"], b["faces"][2:])
    ab, ba = distance(A, B, 0.08, samples=True, timing=True), distance(B, A, 0.08, samples=True)
    for k in ("points", "weight", "distance", "face"):
        assert torch.equal(ab["a_to_b"][k], ba["b_to_a"][k]) and torch.equal(ab["b_to_a"][k], ba["a_to_b"][k])
    for k in ("mean", "rms", "max", "p50", "p95", "n_samples", "n_beyond"):
        assert ab["a_to_b"][k] == ba["b_to_a"][k] and ab["b_to_a"][k] == ba["a_to_b"][k]
    assert ab["hausdorff"] == ba["hausdorff"] >= max(ab["a_to_b"]["mean"], ab["b_to_a"]["mean"]) and ab["chamfer"] == ba["chamfer"]
    assert sorted(ab["times"]) == sorted(f"{d}.{p}" for d in ("a_to_b", "b_to_a") for p in ("sample", "query", "stats"))
    d = host(ab["a_to_b"]["distance"])
    bound = float(np.median(d))
    cut = distance(A, B, 0.08, max_distance=bound)
    assert cut["a_to_b"]["n_beyond"] == int((d > bound).sum()) > 0 and cut["a_to_b"]["max"] == d[d <= bound].max()
    assert cut["a_to_b"]["n_samples"] == len(d)


def test_quadric_placement_is_closer_to_the_input_than_the_mean():
    """On a sphere of radius 0.6 sampled at 33 per axis, simplified on cells of 4 steps: the surface distance to the input, in the mean
    and both ways, is smaller with the quadric placement than with the cells' means (the ordering DESIGN 3.16 reports against the
    analytic sphere).  The ordering alone is asserted; the numbers are printed."""
    res = (33, 33, 33)
    lo, step = mt.cube_grid(res)
    verts, faces = mesh.iso_surface(dev(mt.field("sphere", res, lo, step)), 0.0, lo, step)
    cell = (np.float32(4) * step).astype(np.float32)
    out = {}
    for placement in ("quadric", "mean"):
        sv, sf, _ = mesh.simplify(verts, faces, cell, origin=lo, placement=placement)
        out[placement] = mesh.surface_distance(verts, faces, sv, sf, float(step.min()))
        o = out[placement]
        print(f"{placement}: {sv.shape[0]} vertices / {sf.shape[0]} faces; input -> simplified mean {o['a_to_b']['mean']:.6f} max {o['a_to_b']['max']:.6f}; "
              f"simplified -> input mean {o['b_to_a']['mean']:.6f} max {o['b_to_a']['max']:.6f}; chamfer {o['chamfer']:.6f} hausdorff {o['hausdorff']:.6f}")
    for d in ("a_to_b", "b_to_a"):
        assert out["quadric"][d]["mean"] < out["mean"][d]["mean"]


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def test_the_same_input_gives_the_same_bytes(cases):
    c = cases["two_spheres"]
    v, f, q = dev(c["verts"]), dev(c["faces"]), dev(c["queries"])
    first = host(mesh.closest_points(q, v, f))
    s_first = host(mesh.sample_faces(v, f, 0.05))
    for _ in range(2):
        assert dr.mismatches(host(mesh.closest_points(q, v, f)), first, mesh._DIST_COUNTS) == []
        assert dr.sample_mismatches(host(mesh.sample_faces(v, f, 0.05)), s_first) == []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other, s_other = mesh.closest_points(q, v, f), mesh.sample_faces(v, f, 0.05)
    side.synchronize()
    assert dr.mismatches(host(other), first, mesh._DIST_COUNTS) == [] and dr.sample_mismatches(host(s_other), s_first) == []


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_a_bad_face_index_is_refused_before_anything_else_runs(cases, monkeypatch):
    c = cases["sphere"]
    faces = c["faces"].copy()
    faces[len(faces) // 2, 1] = len(c["verts"])
    seen, real = [], lib.check

    def spy(rc, what):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(lib, "check", spy)
    v, f, q = dev(c["verts"]), dev(faces), dev(c["queries"])
    for call in (lambda: mesh.closest_points(q, v, f), lambda: mesh.sample_faces(v, f, 0.1),
                 lambda: mesh.surface_distance(v, f, v, dev(c["faces"]), 0.1)):
        del seen[:]
        with pytest.raises(lib.MofaError, match=f"1 of the {3 * len(faces)} face indices lie outside"):
            call()
        assert seen == ["mofa_cc_validate"]


def test_bad_input_is_refused(cases, monkeypatch):
    c = cases["sphere"]
    v, f, q = dev(c["verts"]), dev(c["faces"]), dev(c["queries"][:64])
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.closest_points(q.cpu(), v, f)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.closest_points(q, v.cpu(), f)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.closest_points(q, v, f.cpu())
    with pytest.raises(lib.MofaError, match="int32"):
        mesh.closest_points(q, v, f.long())
    with pytest.raises(lib.MofaError, match="float32"):
        mesh.closest_points(q.double(), v, f)
    with pytest.raises(lib.MofaError, match=r"points \[N,3\]"):
        mesh.closest_points(q[:, :2].contiguous(), v, f)
    bad = c["verts"].copy()
    bad[11, 1] = np.nan
    seen, real = [], lib.check

    def spy(rc, what):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(lib, "check", spy)
    with pytest.raises(lib.MofaError, match="1 of the .* coordinates of the target mesh are not finite"):
        mesh.closest_points(q, dev(bad), f)
    assert seen == ["mofa_cc_validate", "mofa_dist_validate"]
    monkeypatch.setattr(lib, "check", real)
    for m in (0.0, -1.0, np.nan):
        with pytest.raises(lib.MofaError, match="max_distance"):
            mesh.closest_points(q, v, f, max_distance=m)
        with pytest.raises(lib.MofaError, match="max_distance"):
            mesh.surface_distance(v, f, v, f, 0.1, max_distance=m)
    for g in (0, -3, mesh.DIST_GRID_CAP + 1, (4, 4), (4, 0, 4), 2.5, "7"):
        with pytest.raises(lib.MofaError, match="grid"):
            mesh.closest_points(q, v, f, grid=g)
    for s in (0.0, -0.1, np.nan, np.inf):
        with pytest.raises(lib.MofaError, match="spacing"):
            mesh.sample_faces(v, f, s)
        with pytest.raises(lib.MofaError, match="spacing"):
            mesh.surface_distance(v, f, v, f, s)
    for k in (0, -1, 1.5, mesh.DIST_MAX_SUBDIV + 1):
        with pytest.raises(lib.MofaError, match="max_subdiv"):
            mesh.sample_faces(v, f, 0.1, k)
    nanq = c["queries"][:64].copy()
    nanq[5, 0], nanq[40, 2] = np.nan, -np.inf                        # counted, not refused
    want = dr.brute_force(nanq, c["verts"], c["faces"])
    for g in (1, None):
        got = closest(nanq, c["verts"], c["faces"], grid=g)
        assert dr.mismatches(got, want) == [] and got["counts"]["non_finite_queries"] == 2
        assert np.isnan(got["distance"][[5, 40]]).all() and got["face"][[5, 40]].tolist() == [-1, -1]


# ---- through the network ---------------------------------------------------------------------------------------------------------------
BOUNDS, RES = ((-1.0, -1.1, -0.9), (1.1, 0.9, 1.0)), (33, 33, 33)


@pytest.fixture(scope="module")
def face():
    render = Renderer(netchunk=1024 * 64, expCodesLen=30)
    render.idSpecificMod.load_state_dict(synth.style_state(0))
    for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(0)):
        dst.data[:] = src
    render = render.to(DEV).eval()
    net = NeRF(D=10, W=1024, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(10, 1024, 1))
    net = net.to(DEV)
    bm, tex, e = [t.to(DEV) for t in synth.codes(3)]
    grid = render.query_density(net, bounds=BOUNDS, resolution=RES, shapeCodes=bm, expCodes=e)
    return dict(render=render, net=net, kw=dict(bounds=BOUNDS, resolution=RES, level=float(grid.median()), shapeCodes=bm, expCodes=e))


def test_simplify_error_through_the_network(face):
    render, net = face["render"], face["net"]
    kw = dict(face["kw"], components="largest", refine=2)
    plain = host(render.extract_mesh(net, simplify=4, **kw))
    plain_stats = host(dict(render.mesh_stats["simplify"]))
    assert "simplify_error" not in render.mesh_stats
    measured = host(render.extract_mesh(net, simplify=4, simplify_error=True, **kw))
    stats = render.mesh_stats
    assert np.array_equal(measured[0].view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(measured[1], plain[1])
    got = host(dict(stats["simplify"]))
    assert got.keys() == plain_stats.keys()
    assert all(np.array_equal(got[k], plain_stats[k]) for k in got)
    err = stats["simplify_error"]
    print(f"simplify=4 on {RES}: hausdorff {err['hausdorff']:.5f}, chamfer {err['chamfer']:.5f}, mean {err['a_to_b']['mean']:.5f} / "
          f"{err['b_to_a']['mean']:.5f} (grid step {2.1 / 32:.5f}; seeded weights: this says nothing about a trained face)")
    for d in ("a_to_b", "b_to_a"):
        assert all(np.isfinite(err[d][k]) for k in ("mean", "rms", "max", "p50", "p95")) and err[d]["n_samples"] > 0 and err[d]["n_beyond"] == 0
    assert err["hausdorff"] >= max(err["a_to_b"]["mean"], err["b_to_a"]["mean"]) > 0 and np.isfinite(err["chamfer"])
    with pytest.raises(lib.MofaError, match="simplify_error"):
        render.extract_mesh(net, simplify_error=True, **kw)

"""Mesh simplification on the GPU (``mofa_simp_*``, ``mesh.simplify``, ``Renderer.extract_mesh(simplify=)``) against the NumPy restatement
(tests/simp_reference.py):

* ``verts'``, ``faces'``, ``cluster_of`` and every counter are the restatement's bit for bit (``simp_reference.mismatches``;
  tests/test_simp_reference_cpu.py shows what it catches) on iso-surfaces at lattice cells of 2, 4 and 7 steps and a non-lattice cell and
  origin, a hollow shell, randomly permuted numbering, hand-made meshes (one vertex per cell, one cell for everything, vertices on cell
  boundaries, fins far apart, duplicates, degenerate faces, a bow-tie) and clusters whose corners straddle the reduction's chunk seams;
* bad indices, vertices without a cell, bad parameters and CPU tensors raise ``MofaError``; a bad index before any other kernel runs;
* the same mesh gives the same bytes;
* through the seeded 10 x 1024 network: ``simplify=None`` changes nothing, ``simplify=4`` after ``components=`` and ``refine=`` and before
  normals and colours gives consistent shapes and a closed mesh, and the network is asked at the simplified vertices only.
"""
import numpy as np
import pytest
import torch

import cc_reference as cc
import mt_reference as mt
import simp_reference as sr
from mofanerf_amd import lib, mesh, synth
from mofanerf_amd.model import NeRF
from mofanerf_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(host(v) for v in x)
    return x.cpu().numpy() if torch.is_tensor(x) else x


def check(verts, faces, cell, origin=None, **kw):
    """mesh.simplify equals the restatement bit for bit; returns (the GPU result on the host, the restatement's)."""
    got = host(mesh.simplify(dev(verts), dev(faces), cell, origin, **kw))
    want = sr.simplify(verts, faces, cell, origin, **kw)
    st = got[2]
    print(f"V = {len(verts)}, F = {len(faces)}, cell {np.asarray(cell).tolist()}: {st['n_clusters']} clusters -> {st['verts_out']} vertices, "
          f"{st['faces_out']} faces ({st['faces_degenerate']} degenerate, {st['faces_cancelled']} cancelled); placed "
          f"{st['placed_quadric']} / {st['placed_mean']} / {st['placed_first']}; {st['edges_multiple']} directed edges used twice")
    assert sr.mismatches(got, want) == []
    assert st["placed_quadric"] + st["placed_mean"] + st["placed_first"] == st["n_clusters"]
    return got, want


@pytest.fixture(scope="module")
def fields():
    """The three analytic iso-surfaces through mesh.iso_surface, on the host, with their lattice (computed once)."""
    out = {}
    for name, res in cc.FIELDS:
        lo, step = mt.cube_grid(res)
        out[name] = host(mesh.iso_surface(dev(mt.field(name, res, lo, step)), 0.0, lo, step)) + (lo, step)
    return out


# ---- bit for bit against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (2, 4, 7, "free"))
@pytest.mark.parametrize("name", [n for n, _ in cc.FIELDS])
def test_iso_surfaces_equal_the_restatement(fields, name, m):
    verts, faces, lo, step = fields[name]
    if m == "free":                                                  # a cell and an origin that are no multiples of the lattice
        cell, origin = np.array([0.11, 0.07, 0.13], dtype=np.float32), np.array([-1.03, -1.01, -1.07], dtype=np.float32)
    else:
        cell, origin = sr.lattice_cell(step, m), lo
    for placement in ("quadric", "mean"):
        (ov, of, st), _ = check(verts, faces, cell, origin, placement=placement)
        assert not sr.edge_balance(of).any()                          # closed in, closed out
        assert sr.cell_violations(ov, sr.keys(ov, origin, cell)[0], origin, cell) == 0
        assert (np.diff(sr.keys(ov, origin, cell)[0]) > 0).all()      # one vertex per cell, by ascending key
        assert st["mean_requested"] == (st["n_clusters"] if placement == "mean" else 0)
    assert 0 < st["faces_out"] < len(faces) and st["verts_out"] < len(verts)


def test_the_default_origin_and_a_scalar_cell(fields):
    verts, faces, _, _ = fields["torus"]
    check(verts, faces, 0.09)
    check(verts, faces, 0.09, regularize=0.25)


def test_hollow_shell():
    grid, lo, step = cc.shell_field((41, 41, 41))
    verts, faces = host(mesh.iso_surface(dev(grid), 0.0, lo, step))
    (ov, of, st), _ = check(verts, faces, sr.lattice_cell(step, 3), lo)
    assert not sr.edge_balance(of).any() and cc.components(ov, of)["n_components"] == 2


def test_permuted_numbering(fields):
    """The permuted mesh equals the restatement on the permuted mesh bit for bit.  Against the unpermuted result: the cells are the same,
    so the output has the same vertices (one per key, in key order) and, as a set, the same faces; the positions come from sums taken in
    another order: the fp64 sums differ by rounding, far below an fp32 ulp, so after the rounding to fp32 a coordinate differs by at most
    one ulp of a number below 2, 2^-23 (the largest difference is printed)."""
    verts, faces, lo, step = fields["two_spheres"]
    cell = sr.lattice_cell(step, 4)
    (ov, of, _), _ = check(verts, faces, cell, lo)
    pv, pf, perm = cc.permuted(verts, faces, 3)
    (qv, qf, st), _ = check(pv, pf, cell, lo)
    assert np.array_equal(sr.keys(qv, lo, cell)[0], sr.keys(ov, lo, cell)[0])
    assert np.array_equal(np.unique(qf, axis=0), np.unique(of, axis=0)) and len(qf) == len(of)
    print(f"largest |position difference| between the two numberings: {np.abs(qv - ov).max():.3e}")
    assert np.abs(qv - ov).max() <= 2.0 ** -23
    back = host(mesh.simplify(dev(verts), dev(faces), cell, lo))[2]["cluster_of"]
    assert np.array_equal(st["cluster_of"][perm], back)


# ---- hand-made meshes ------------------------------------------------------------------------------------------------------------------
def test_one_vertex_per_cell_returns_the_input():
    """Three planes meet in each vertex of a tetrahedron, and the vertex is its cluster's mean: the regularised minimiser is the vertex
    itself, up to an fp64 rounding that the rounding to fp32 removes.  The output is the input up to the vertex order (by key)."""
    verts, faces = sr.tetrahedron()
    (ov, of, st), _ = check(verts, faces, 1.0, (0, 0, 0))
    order = np.argsort(sr.keys(verts, np.zeros(3), 1.0)[0])
    rank = np.argsort(order)
    assert np.array_equal(ov, verts[order]) and st["placed_quadric"] == 4
    assert of.tolist() == sr.canonical(rank[faces]).tolist()          # the faces in their order, renumbered, smallest index first
    assert st["cluster_of"].tolist() == rank.tolist() and not sr.edge_balance(of).any() and mt.is_closed_oriented_manifold(of)


def test_everything_in_one_cell_leaves_nothing():
    verts, faces = sr.tetrahedron()
    (ov, of, st), _ = check(verts, faces, 4.0, (0, 0, 0))
    assert ov.shape == (0, 3) and of.shape == (0, 3) and st["n_clusters"] == 1 and st["faces_degenerate"] == 4
    assert st["cluster_of"].tolist() == [-1] * 4


def test_vertices_on_cell_boundaries_and_at_the_origin():
    verts, faces, origin, cell = sr.boundary_mesh()
    (ov, of, st), want = check(verts, faces, cell, origin)
    k = sr.keys(verts, origin, cell)[0]
    assert k[0] == 0 and k[1] == 2 << 42 and k[2] == 1 << 42         # at the origin; on a boundary: the upper cell; one ulp below: the lower
    check(verts, faces, cell, origin, placement="mean")


def test_a_fin_pair_far_apart_cancels():
    verts, faces = sr.fin_mesh()
    (ov, of, st), _ = check(verts, faces, 1.0, (0, 0, 0))
    assert st["faces_cancelled"] == 2 and st["faces_out"] == len(faces) - 2 and st["faces_degenerate"] == 0
    gone = sorted(st["cluster_of"][[1, 2, 3]].tolist())
    assert len(ov) == 4 and not any(sorted(r) == gone for r in of.tolist())          # both copies of the face went, everything else stayed


def test_three_copies_and_one_opposite_keep_two():
    verts, faces = sr.three_and_one()
    (ov, of, st), _ = check(verts, faces, 1.0, (0, 0, 0))
    assert st["faces_out"] == 2 and st["faces_cancelled"] == 2 and st["edges_multiple"] == 3
    assert of.tolist() == sr.canonical(st["cluster_of"][faces[:2]]).tolist()          # the first two of the majority orientation


def test_degenerate_faces_unreferenced_vertices_and_a_bow_tie():
    verts, faces = cc.odd_mesh()
    for cell in (0.5, 1.5, 50.0):
        (_, _, st), _ = check(verts, faces, cell)
        assert (st["cluster_of"][[0, 2, 10, 13]] == -1).all()
    (_, _, st), _ = check(*sr.tetrahedron_with_stray(), 1.0, (0, 0, 0))          # an unreferenced vertex in a used cell joins no mean
    assert st["cluster_of"][4] == -1 and st["verts_out"] == 4
    check(*sr.tetrahedron_with_stray(), 1.0, (0, 0, 0), placement="mean")
    check(*cc.bow_tie(), 0.75)
    check(*cc.bow_tie(), 0.75, placement="mean")
    empty = mesh.simplify(dev(verts), torch.zeros(0, 3, dtype=torch.int32, device=DEV), 1.0)
    assert sr.mismatches(host(empty), sr.simplify(verts, np.zeros((0, 3), dtype=np.int32), 1.0)) == []
    none = mesh.simplify(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV), 1.0)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3) and none[2]["verts_in"] == 0


# ---- reduction seams -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (1025, 100003))
def test_strips_squeezed_into_two_cells(V):
    verts, faces, origin, cell = sr.two_cell_strip(V, V)
    (ov, of, st), _ = check(verts, faces, cell, origin)
    # each of the two big clusters' 3 V / 2 corners span many chunks of mesh.CC_CHUNK, and both representatives are in the output
    assert st["n_clusters"] == 4 and len(ov) == 4 and len(of) == 2 and st["faces_degenerate"] == V - 2
    check(verts, faces, cell, origin, placement="mean")


@pytest.mark.parametrize("n", (1023, 1024, 1025))
def test_clusters_of_exactly_n_corners(n):
    verts, faces, origin, cell = sr.fan_of_corners(n, n)
    _, (_, _, want) = check(verts, faces, cell, origin)
    assert np.bincount(want["cluster"][faces.astype(np.int64)].reshape(-1))[0] == n and mesh.CC_CHUNK == sr.CHUNK == 1024


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ("V", -1, 2 ** 31 - 1))
def test_a_bad_face_index_is_refused_before_anything_else_runs(fields, monkeypatch, bad):
    verts, faces, lo, step = fields["sphere"]
    faces = faces.copy()
    faces[len(faces) // 2, 1] = len(verts) if bad == "V" else bad
    seen, real = [], lib.check

    def spy(rc, what):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(lib, "check", spy)
    with pytest.raises(lib.MofaError, match=f"1 of the {3 * len(faces)} face indices lie outside"):
        mesh.simplify(dev(verts), dev(faces), 0.1, lo)
    assert seen == ["mofa_cc_validate"]
    with pytest.raises(sr.Refused, match="1 of the"):
        sr.simplify(verts, faces, 0.1, lo)


def test_vertices_without_a_cell_are_refused(fields, monkeypatch):
    verts, faces, lo, step = fields["sphere"]
    seen, real = [], lib.check

    def spy(rc, what):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(lib, "check", spy)
    for value, cell, origin in ((np.nan, 0.1, lo), (np.inf, 0.1, lo), (1.0, 1e-7, lo), (-1.5, 0.1, lo)):
        v = verts.copy()
        v[7, 2] = value                                               # NaN / infinite / beyond 2^21 cells of 1e-7 / below the origin
        del seen[:]
        with pytest.raises(lib.MofaError, match="vertices are not finite or lie outside"):
            mesh.simplify(dev(v), dev(faces), cell, origin)
        assert seen == ["mofa_cc_validate", "mofa_simp_keys"]
        with pytest.raises(sr.Refused):
            sr.simplify(v, faces, cell, origin)
    v = verts.copy()
    v[7, 2] = np.nan
    with pytest.raises(lib.MofaError, match="origin"):                # the default origin of a mesh with a NaN is no origin
        mesh.simplify(dev(v), dev(faces), 0.1)


def test_bad_parameters_and_cpu_tensors_are_refused(fields):
    verts, faces, lo, step = fields["sphere"]
    v, f = dev(verts), dev(faces)
    for cell in (0.0, -0.1, np.nan, np.inf, (0.1, 0.0, 0.1), (0.1, 0.1)):
        with pytest.raises(lib.MofaError, match="cell"):
            mesh.simplify(v, f, cell, lo)
    for reg in (0.0, -1e-3, np.nan, np.inf):
        with pytest.raises(lib.MofaError, match="regularize"):
            mesh.simplify(v, f, 0.1, lo, regularize=reg)
    with pytest.raises(lib.MofaError, match="placement"):
        mesh.simplify(v, f, 0.1, lo, placement="median")
    with pytest.raises(lib.MofaError, match="origin"):
        mesh.simplify(v, f, 0.1, (0.0, np.nan, 0.0))
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.simplify(torch.from_numpy(verts), f, 0.1)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.simplify(v, torch.from_numpy(faces), 0.1)
    with pytest.raises(lib.MofaError, match="int32"):
        mesh.simplify(v, f.long(), 0.1)


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def test_the_same_mesh_gives_the_same_bytes(fields):
    verts, faces, lo, step = fields["torus"]
    pv, pf, _ = cc.permuted(verts, faces, 3)
    v, f = dev(pv), dev(pf)
    first = host(mesh.simplify(v, f, sr.lattice_cell(step, 2), lo))
    for _ in range(3):
        assert sr.mismatches(host(mesh.simplify(v, f, sr.lattice_cell(step, 2), lo)), first) == []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = mesh.simplify(v, f, sr.lattice_cell(step, 2), lo, timing=True)
    side.synchronize()
    assert sr.mismatches(host(other), first) == []
    assert list(other[2]["times"]) == ["validate", "keys", "clusters", "sums", "place", "faces", "compact"]


# ---- through the network ---------------------------------------------------------------------------------------------------------------
BOUNDS, RES, BRICK = ((-1.0, -1.1, -0.9), (1.1, 0.9, 1.0)), (33, 33, 33), 8
QUANTILE = 0.5


def make(D=10, W=1024, seed=1, netchunk=1024 * 64):
    render = Renderer(netchunk=netchunk, expCodesLen=30)
    render.idSpecificMod.load_state_dict(synth.style_state(0))
    for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(0)):
        dst.data[:] = src
    render = render.to(DEV).eval()
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, seed))
    return render, net.to(DEV)


@pytest.fixture(scope="module")
def face():
    render, net = make()
    bm, tex, e = [t.to(DEV) for t in synth.codes(3)]
    grid = render.query_density(net, bounds=BOUNDS, resolution=RES, shapeCodes=bm, expCodes=e)
    return dict(render=render, net=net, tex=tex, kw=dict(bounds=BOUNDS, resolution=RES, level=float(grid.median()), shapeCodes=bm, expCodes=e))


def face_normals_fp64(verts, faces):
    """(area-weighted unit vertex normals in fp64, a bound on what mesh.vertex_normals may differ from them by): mesh.vertex_normals sums
    k fp32 cross products per vertex in no fixed order and normalises.  Each product carries a few 2^-24 |u| |w| of rounding and the sum
    (k - 1) 2^-24 of the absolute sum, so the direction's error is below (k + 8) 2^-24 sum(|u| |w|) / |sum|; the bound takes 8 times that."""
    v, f = verts.astype(np.float64), faces.astype(np.int64)
    u, w = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    t, mag = np.cross(u, w), np.linalg.norm(u, axis=1) * np.linalg.norm(w, axis=1)
    total, absolute, k = np.zeros((len(v), 3)), np.zeros(len(v)), np.bincount(f.reshape(-1), minlength=len(v))
    for c in range(3):
        np.add.at(total, f[:, c], t)
        np.add.at(absolute, f[:, c], mag)
    norm = np.linalg.norm(total, axis=1)
    with np.errstate(all="ignore"):
        return total / norm[:, None], np.where(norm > 0, (k + 8) * 2.0 ** -21 * absolute / norm, np.inf)


@pytest.mark.parametrize("brick", (None, BRICK))
def test_simplify_none_changes_nothing(face, brick):
    render, net = face["render"], face["net"]
    kw = dict(face["kw"], brick=brick, refine=2, normals="density", colors=True, uvCodes=face["tex"])
    plain = host(render.extract_mesh(net, **kw))
    same = host(render.extract_mesh(net, simplify=None, **kw))
    assert "simplify" not in render.mesh_stats and "edge_ids" in render.mesh_stats
    assert cc.compaction_mismatches(same, plain) == []
    bare = host(render.extract_mesh(net, **face["kw"], brick=brick))
    assert cc.compaction_mismatches(host(render.extract_mesh(net, simplify=None, **face["kw"], brick=brick)), bare) == []
    for bad in (1, 0, -4, 2.0, True, "4"):
        with pytest.raises(lib.MofaError, match="simplify"):
            render.extract_mesh(net, simplify=bad, **face["kw"])
    with pytest.raises(lib.MofaError, match="placement"):
        render.extract_mesh(net, simplify=4, placement="median", **face["kw"])


@pytest.mark.parametrize("brick", (None, BRICK))
def test_simplified_extraction_runs_the_network_on_the_simplified_vertices(face, brick):
    render, net = face["render"], face["net"]
    kw = dict(face["kw"], brick=brick, components="largest", refine=3, normals="density", colors=True, uvCodes=face["tex"])
    fv, ff, frgb, fn = host(render.extract_mesh(net, **kw))
    full = dict(render.mesh_stats)
    verts, faces, rgb, nrm = host(render.extract_mesh(net, simplify=4, **kw))
    stats = dict(render.mesh_stats)
    st = host(stats["simplify"])
    print(f"brick {brick}: {len(fv)} vertices / {len(ff)} faces -> {len(verts)} / {len(faces)}; placed {st['placed_quadric']} / "
          f"{st['placed_mean']} / {st['placed_first']}; {st['edges_multiple']} directed edges used twice")
    V = len(verts)
    assert verts.shape == (V, 3) and rgb.shape == (V, 3) and nrm.shape == (V, 3) and faces.dtype == np.int32 and faces.shape[1] == 3
    assert 0 < V < len(fv) and 0 < len(faces) < len(ff) and faces.min() == 0 and faces.max() == V - 1
    assert st["verts_in"] == len(fv) and st["faces_in"] == len(ff) and st["verts_out"] == V and st["faces_out"] == len(faces)
    assert np.isfinite(verts).all() and np.isfinite(rgb).all() and np.isfinite(nrm).all()
    # closed where the unsimplified mesh is (a surface that leaves the grid is open at the border)
    assert not sr.edge_balance(faces).any() or sr.edge_balance(ff).any()
    # refinement ran before, on every unsimplified vertex; normals and colours after, on the simplified ones
    assert stats["refine"]["evaluations"] == full["refine"]["evaluations"] == 5 * len(fv)
    assert stats["normal_evaluations"] == 6 * V < full["normal_evaluations"] == 6 * len(fv)
    assert stats["color_evaluations"] == V < full["color_evaluations"] == len(fv)
    assert "edge_ids" not in stats and "edge_ids" in full
    # the simplification is mesh.simplify of the refined, filtered mesh on lattice-aligned cells: the restatement gives the same bytes
    res, lo, step = mesh.grid_spec(BOUNDS, RES)
    want = sr.simplify(fv, ff, sr.lattice_cell(step, 4), lo)
    assert sr.mismatches((verts, faces, st), want) == []
    # normals="faces" is computed on the simplified mesh
    kw["normals"] = "faces"
    v2, f2, _, n2 = render.extract_mesh(net, simplify=4, **kw)
    assert np.array_equal(host(v2), verts) and np.array_equal(host(f2), faces)
    ref, bound = face_normals_fp64(verts, faces)
    sure = bound < 0.1
    print(f"normals='faces': {int(sure.sum())} of {V} vertices with a bound below 0.1, largest error / bound "
          f"{(np.abs(host(n2) - ref).max(1) / bound)[sure].max():.3f}")
    assert n2.shape == (V, 3) and sure.sum() > 0.9 * V and (np.abs(host(n2) - ref).max(1) <= bound)[sure].all()
    mean = host(render.extract_mesh(net, simplify=4, placement="mean", **dict(kw, colors=False, normals=None)))
    assert sr.mismatches(mean + (host(render.mesh_stats["simplify"]),), sr.simplify(fv, ff, sr.lattice_cell(step, 4), lo, placement="mean")) == []

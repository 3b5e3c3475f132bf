"""Mesh components on the GPU (``mofa_cc_*``, ``mesh.components`` / ``select_components`` / ``keep_components``,
``Renderer.extract_mesh(components=)``) against the NumPy restatement (tests/cc_reference.py):

* labels, counts and boxes are exactly the restatement's, areas and volumes lie within ``(n_faces + 8) 2^-52 sum |term|`` of it, on
  iso-surfaces in lattice and in random numbering, a hollow ball, a bow-tie, degenerate faces with unreferenced vertices and randomly
  numbered strips up to 100,003 vertices (``cc_reference.mismatches``: tests/test_cc_reference_cpu.py shows what it catches);
* the same mesh gives the same bytes: across repeats and on a non-default stream;
* a face index outside [0, V) raises ``MofaError`` with the count after the validation kernel and before any other launch;
* ``keep_components`` equals the restatement bit for bit, companions included, and stays watertight;
* through the seeded 10 x 1024 network: ``components=None`` changes nothing, ``"largest"`` / ``8`` equal the restatement applied to the
  unfiltered mesh, and filtering before refinement, normals and colours equals filtering after them, on the dense and the brick path.
"""
import numpy as np
import pytest
import torch

import cc_reference as cc
import mt_reference as mt
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


def check(verts, faces, n_components=None):
    """mesh.components on (verts, faces) (NumPy) equals the restatement; returns (GPU stats, the restatement's)."""
    stats = mesh.components(dev(verts), dev(faces))
    want = cc.components(verts, faces)
    got = host(stats)
    print(f"V = {len(verts)}, F = {len(faces)}: {got['n_components']} components, {got['passes']} passes, "
          f"max |area - ref| / bound = {rel_err(got, want, 'area'):.3f}, volume {rel_err(got, want, 'volume'):.3f}")
    assert cc.mismatches(got, want) == []
    assert 1 <= got["passes"] < mesh.MAX_CC_PASSES
    assert n_components is None or got["n_components"] == n_components
    return stats, want


def rel_err(got, want, k):
    bound = (want["n_faces"] + 8) * cc.EPS * want["abs_" + k]
    if got[k].shape != want[k].shape or not len(bound):
        return float("nan")
    return float(np.max(np.abs(got[k] - want[k]) / np.where(bound > 0, bound, 1)))


@pytest.fixture(scope="module")
def fields():
    """The three analytic iso-surfaces through mesh.iso_surface, on the host (computed once)."""
    out = {}
    for name, res in cc.FIELDS:
        lo, step = mt.cube_grid(res)
        out[name] = host(mesh.iso_surface(dev(mt.field(name, res, lo, step)), 0.0, lo, step))
    return out


# ---- labels and statistics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_c", (("sphere", 1), ("two_spheres", 2), ("torus", 1)))
def test_iso_surfaces_in_lattice_and_random_numbering(fields, name, n_c):
    verts, faces = fields[name]
    stats, want = check(verts, faces, n_c)
    assert want["unreferenced"] == 0
    if name == "two_spheres":
        assert want["n_verts"].tolist() == [3522, 3522]
        assert host(mesh.select_components(stats, "largest")).tolist() == [True, False]       # the tie keeps label 0
    pv, pf, _ = cc.permuted(verts, faces, 3)
    check(pv, pf, n_c)


def test_hollow_ball_is_a_solid_and_a_cavity():
    grid, lo, step = cc.shell_field((41, 41, 41))
    verts, faces = host(mesh.iso_surface(dev(grid), 0.0, lo, step))
    stats, want = check(verts, faces, 2)
    volume = host(stats["volume"])
    assert volume[0] > 0 > volume[1]
    total = mt.signed_volume(verts, faces)                           # the shell's volume, summed in fp64 over all faces
    assert abs(volume.sum() - total) <= (len(faces) + 8) * cc.EPS * want["abs_volume"].sum()
    assert abs(total - 4 / 3 * np.pi * (0.7 ** 3 - 0.35 ** 3)) < 0.02 * total


def test_bow_tie_degenerate_faces_and_unreferenced_vertices():
    check(*cc.bow_tie(), 1)
    stats, want = check(*cc.odd_mesh(), 3)
    assert stats["unreferenced"] == 4 and host(stats["vertex_labels"]).tolist() == [-1, 0, -1, 1, 1, 2, 1, 2, 0, 0, -1, 2, 2, -1]
    empty = mesh.components(dev(cc.odd_mesh()[0]), torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    assert cc.mismatches(host(empty), cc.components(cc.odd_mesh()[0], np.zeros((0, 3), dtype=np.int32))) == [] and empty["passes"] == 0
    none = mesh.components(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    assert none["n_components"] == 0 and none["unreferenced"] == 0


@pytest.mark.parametrize("V", cc.STRIPS)
def test_randomly_numbered_strips(V):
    stats, _ = check(*cc.strip(V, V), 1)
    if V == 100003:
        assert stats["passes"] <= 16


def test_the_same_mesh_gives_the_same_bytes(fields):
    verts, faces, _ = cc.permuted(*fields["torus"], 3)
    v, f = dev(verts), dev(faces)
    keys = ("vertex_labels", "face_labels", "n_verts", "n_faces", "area", "volume", "bbox")
    first = host(mesh.components(v, f))
    for _ in range(4):                                            # plain repeats of a passing call
        again = host(mesh.components(v, f))
        assert all(np.array_equal(again[k].view(np.uint8), first[k].view(np.uint8)) for k in keys)
        assert again["n_components"] == first["n_components"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = mesh.components(v, f)
    side.synchronize()
    other = host(other)
    assert all(np.array_equal(other[k].view(np.uint8), first[k].view(np.uint8)) for k in keys)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ("V", -1, 2 ** 31 - 1))
def test_a_bad_face_index_is_refused_before_anything_else_runs(fields, monkeypatch, bad):
    verts, faces = fields["sphere"]
    faces = faces.copy()
    faces[len(faces) // 2, 1] = len(verts) if bad == "V" else bad
    seen, real = [], lib.check

    def spy(rc, what):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(lib, "check", spy)
    with pytest.raises(lib.MofaError, match=f"1 of the {3 * len(faces)} face indices lie outside"):
        mesh.components(dev(verts), dev(faces))
    assert seen == ["mofa_cc_validate"]
    faces[0, 0] = -7
    with pytest.raises(lib.MofaError, match="2 of the"):
        mesh.components(dev(verts), dev(faces))
    assert seen == ["mofa_cc_validate"] * 2


def test_cpu_tensors_and_wrong_layouts_are_refused(fields):
    verts, faces = fields["sphere"]
    v, f = dev(verts), dev(faces)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.components(torch.from_numpy(verts), f)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.components(v, torch.from_numpy(faces))
    with pytest.raises(lib.MofaError, match="int32"):
        mesh.components(v, f.long())
    with pytest.raises(lib.MofaError, match="contiguous"):
        mesh.components(dev(np.concatenate([verts, verts], 1))[:, :3], f)
    stats = mesh.components(v, f)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.keep_components(torch.from_numpy(verts), f, stats, mesh.select_components(stats, "largest"))
    with pytest.raises(lib.MofaError, match="mask"):
        mesh.keep_components(v, f, stats, torch.ones(2, dtype=torch.bool, device=DEV))
    with pytest.raises(lib.MofaError, match="per-vertex"):
        mesh.keep_components(v, f, stats, mesh.select_components(stats, 1), torch.zeros(3, device=DEV))
    for keep in ("smallest", -1, True, np.ones(3, dtype=bool)):
        with pytest.raises(lib.MofaError, match="select_components"):
            mesh.select_components(stats, keep)


# ---- selection and compaction --------------------------------------------------------------------------------------------------------
def compaction_case(verts, faces, keep):
    rng = np.random.default_rng(len(verts))
    ids = rng.integers(0, 2 ** 40, len(verts)).astype(np.int64)
    rgb = rng.random((len(verts), 3)).astype(np.float32)
    v, f = dev(verts), dev(faces)
    stats = mesh.components(v, f)
    want_stats = cc.components(verts, faces)
    mask = mesh.select_components(stats, keep)
    want_mask = cc.select(want_stats, keep)
    assert np.array_equal(host(mask), want_mask)
    got = host(mesh.keep_components(v, f, stats, mask, dev(ids), dev(rgb)))
    want = cc.compact(verts, faces, want_stats, want_mask, ids, rgb)
    assert cc.compaction_mismatches(got, want) == []
    return got, want_stats, want_mask


def test_keep_components_equals_the_restatement(fields):
    verts, faces = fields["two_spheres"]
    for keep in ("largest", 1, 10 ** 6, lambda s: s["bbox"][:, 0, 0] > 0, [False, True]):
        (kv, kf, _, _), st, mask = compaction_case(verts, faces, keep)
        vkeep = mask[st["vertex_labels"]]
        assert np.array_equal(kv.view(np.uint32), verts[vkeep].view(np.uint32))           # a bit-identical subset in the original order
        assert mt.is_closed_oriented_manifold(kf) and len(kf) == st["n_faces"][mask].sum()   # every directed edge has its reverse exactly once
        if mask.all():                                                                   # keeping everything returns the input bytes
            assert np.array_equal(kv.view(np.uint32), verts.view(np.uint32)) and np.array_equal(kf, faces)
    pv, pf, _ = cc.permuted(verts, faces, 11)
    (kv, kf, _, _), st, mask = compaction_case(pv, pf, "largest")
    assert mt.is_closed_oriented_manifold(kf) and len(kv) == 3522
    grid, lo, step = cc.shell_field((41, 41, 41))
    hv, hf = host(mesh.iso_surface(dev(grid), 0.0, lo, step))
    (kv, kf, _, _), st, mask = compaction_case(hv, hf, lambda s: s["volume"] < 0)          # the cavity alone
    assert mask.tolist() == [False, True] and mt.is_closed_oriented_manifold(kf) and mt.signed_volume(kv, kf) < 0
    ov, of = cc.odd_mesh()
    for keep in ([False, True, True], [True, True, True], [False, False, False], "largest", 3):
        (kv, kf, _, _), _, mask = compaction_case(ov, of, keep)
    assert len(kv) == 4 and kf.tolist() == [[3, 0, 1], [2, 1, 3], [1, 1, 1]]


# ---- through the network -------------------------------------------------------------------------------------------------------------
BOUNDS, RES = ((-1.0, -1.1, -0.9), (1.1, 0.9, 1.0)), (40, 48, 36)         # test_extract_mesh_end_to_end's
RES_B8 = (41, 49, 33)                                                     # bricks of 8 need (n - 1) % 8 == 0 on every axis
QUANTILE = 0.5                                                            # the level is the grid's median, as there


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
    """The seeded network, its level, and the unfiltered meshes with their restated components (computed once)."""
    render, net = make()
    bm, tex, e = [t.to(DEV) for t in synth.codes(3)]
    grid = render.query_density(net, bounds=BOUNDS, resolution=RES, shapeCodes=bm, expCodes=e)
    level = float(grid.median()) if QUANTILE == 0.5 else float(torch.quantile(grid.reshape(-1), QUANTILE))
    out = dict(render=render, net=net, tex=tex, kw=dict(bounds=BOUNDS, level=level, shapeCodes=bm, expCodes=e))
    for key, extra in (("dense", dict(resolution=RES)), ("brick", dict(resolution=RES_B8, brick=8))):
        render.mesh_stats = None
        verts, faces = render.extract_mesh(net, **out["kw"], **extra)
        if key == "dense":
            assert render.mesh_stats is None
            _, _, ids = mesh.iso_surface(grid, level, *mesh.grid_spec(BOUNDS, RES)[1:], edge_ids=True)
        else:
            ids = render.mesh_stats["edge_ids"]
        plain = host((verts, faces, ids))
        out[key] = dict(extra=extra, plain=plain, stats=cc.components(plain[0], plain[1]))
    return out


@pytest.mark.parametrize("path", ("dense", "brick"))
def test_the_seeded_mesh_has_floaters(face, path):
    st = face[path]["stats"]
    top = np.sort(st["n_faces"])[::-1][:5].tolist()
    print(f"{path}: {st['n_components']} components over {len(face[path]['plain'][1])} faces; the largest hold {top} faces; "
          f"{int((st['n_faces'] < 8).sum())} hold fewer than 8")
    assert st["n_components"] >= 2


def test_components_none_changes_nothing(face):
    render, net = face["render"], face["net"]
    render.mesh_stats = None
    verts, faces = render.extract_mesh(net, components=None, **face["kw"], **face["dense"]["extra"])
    assert render.mesh_stats is None
    assert cc.compaction_mismatches(host((verts, faces)), face["dense"]["plain"][:2]) == []
    for bad in ("biggest", 0, -3, 2.5, True):
        with pytest.raises(lib.MofaError, match="components"):
            render.extract_mesh(net, components=bad, **face["kw"], **face["dense"]["extra"])


@pytest.mark.parametrize("path", ("dense", "brick"))
@pytest.mark.parametrize("keep", ("largest", 8))
def test_filtered_extraction_equals_the_restatement_on_the_unfiltered_mesh(face, path, keep):
    render, net, case = face["render"], face["net"], face[path]
    verts, faces = render.extract_mesh(net, components=keep, **face["kw"], **case["extra"])
    stats = dict(render.mesh_stats)
    pv, pf, pids = case["plain"]
    mask = cc.select(case["stats"], keep)
    want = cc.compact(pv, pf, case["stats"], mask, pids)
    assert cc.compaction_mismatches(host((verts, faces, stats["edge_ids"])), want) == []
    assert cc.mismatches(host(stats["components"]), case["stats"]) == [] and np.array_equal(host(stats["components"]["kept"]), mask)
    # (a surface that leaves the grid is open at the border, so only a closed mesh has to stay closed)
    assert mt.is_closed_oriented_manifold(host(faces)) or not mt.is_closed_oriented_manifold(pf)
    assert len(faces) == case["stats"]["n_faces"][mask].sum() and 0 < len(faces) <= len(pf)
    if keep == "largest":
        assert len(faces) < len(pf) and cc.components(*host((verts, faces)))["n_components"] == 1


@pytest.mark.parametrize("path", ("dense", "brick"))
def test_filtering_before_refinement_normals_and_colours_equals_filtering_after(face, path):
    """Refinement, density normals and colours are per-vertex work on the network, so running them on the kept vertices only gives the
    bits of running them on all vertices and compacting afterwards.  One exception is read off the code, not met here unless the first
    assertion says so: a vertex whose density gradient vanishes looks along ``mesh.vertex_normals`` for its colour, a float
    ``index_add_`` over its faces with no fixed order; such vertices' colours are compared to 1e-5 instead."""
    render, net, case = face["render"], face["net"], face[path]
    kw = dict(face["kw"], refine=2, normals="density", colors=True, uvCodes=face["tex"], **case["extra"])
    all_v, all_f, all_rgb, all_n = host(render.extract_mesh(net, **kw))
    assert np.array_equal(all_f, case["plain"][1])
    mask = cc.select(case["stats"], "largest")
    want = cc.compact(all_v, all_f, case["stats"], mask, all_rgb, all_n)
    got = host(render.extract_mesh(net, components="largest", **kw))
    stats = dict(render.mesh_stats)
    assert stats["refine"]["evaluations"] == 4 * len(got[0]) and len(got[0]) == case["stats"]["n_verts"][mask].sum()
    zero = ~want[3].any(1)
    print(f"{path}: {len(got[0])} of {len(all_v)} vertices kept; {int(zero.sum())} of them without a density normal")
    assert cc.compaction_mismatches((got[0], got[1], got[3]), (want[0], want[1], want[3])) == []
    assert cc.compaction_mismatches((got[2][~zero],), (want[2][~zero],)) == []
    assert got[2].shape == want[2].shape and (np.abs(got[2][zero] - want[2][zero]) <= 1e-5).all()

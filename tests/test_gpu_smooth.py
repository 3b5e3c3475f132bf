"""Mesh smoothing on the GPU (``mofa_smooth_*``, ``mesh.vertex_adjacency``, ``mesh.smooth``, ``Renderer.extract_mesh(smooth=)``) against the
NumPy restatement (tests/smooth_reference.py; tests/test_smooth_reference_cpu.py shows what it catches):

* the adjacency is the restatement's integer for integer on every mesh of ``smooth_reference.MESHES``;
* the smoothed vertices are the restatement's bit for bit, every counter is equal and the displacement is within 1 ulp, for uniform and
  cotangent weights, a fixed and a free boundary, Taubin and plain Laplacian steps, 1, 2 and 7 iterations, with and without a pinned mask;
* the same call gives the same bytes, the inputs are not written, ``iterations=0`` returns the input's bits;
* a bad face index (before any other kernel), a NaN vertex and CPU tensors raise ``MofaError``;
* through the seeded 10 x 1024 network: ``smooth=3`` equals ``mesh.smooth`` of the unsmoothed extraction, alone and after ``components=``
  and ``simplify=``; normals and colours are evaluated at the smoothed vertices; ``smooth=None`` changes nothing.
"""
import itertools

import numpy as np
import pytest
import torch

import smooth_reference as sr
from mofanerf_amd import lib, mesh, synth
from mofanerf_amd.model import NeRF
from mofanerf_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
DEV = "cuda"
MESH_NAMES = [n for n, _ in sr.MESHES]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(x):
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(host(v) for v in x)
    return x.cpu().numpy() if torch.is_tensor(x) else x


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pinned_mask(V):
    """Every fifth vertex from vertex 2, fixed."""
    m = np.zeros(V, dtype=bool)
    m[2::5] = True
    return m


@pytest.mark.parametrize("name", MESH_NAMES)
def test_the_adjacency_equals_the_restatement(name):
    verts, faces = dict(sr.MESHES)[name]()
    V = len(verts)
    got, want = host(mesh.vertex_adjacency(dev(faces), V)), sr.adjacency(faces, V)
    print(f"{name}: V = {V}, F = {len(faces)}, E = {len(want['neighbours'])}, degree_max {want['degree_max']}, "
          f"{int(want['boundary'].sum())} boundary vertices, {want['edges_nonmanifold']} non-manifold edges")
    assert sorted(got) == ["boundary", "degree_max", "edges_nonmanifold", "neighbours", "offsets"]
    assert got["offsets"].dtype == np.int64 and got["neighbours"].dtype == np.int32 and got["boundary"].dtype == np.bool_
    for k in ("offsets", "neighbours", "boundary"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert got["degree_max"] == want["degree_max"] and got["edges_nonmanifold"] == want["edges_nonmanifold"]
    assert type(got["degree_max"]) is int and type(got["edges_nonmanifold"]) is int


@pytest.mark.parametrize("name", MESH_NAMES)
def test_smoothing_equals_the_restatement_bit_for_bit(name):
    verts, faces = dict(sr.MESHES)[name]()
    v, f, V = dev(verts), dev(faces), len(verts)
    keep_v, keep_f = v.clone(), f.clone()
    moved = 0
    for weights, boundary, mu, iterations, pin in itertools.product(("uniform", "cotangent"), ("fixed", "free"), (-0.53, None), (1, 2, 7),
                                                                    (False, True)):
        mask = pinned_mask(V) if pin else None
        got = host(mesh.smooth(v, f, iterations=iterations, lam=0.5, mu=mu, weights=weights, boundary=boundary,
                               pinned=None if mask is None else dev(mask)))
        want = sr.smooth(verts, faces, iterations=iterations, lam=0.5, mu=mu, weights=weights, boundary=boundary, pinned=mask)
        assert sr.mismatches(got, want) == [], (weights, boundary, mu, iterations, pin)
        assert sorted(got[1]) == sorted(want[1])
        assert np.isfinite(want[0][np.isfinite(verts).all(1)]).all()
        moved = max(moved, int((bits(got[0]) != bits(verts)).any(1).sum()))
    print(f"{name}: 48 calls equal the restatement; at most {moved} of {V} vertices moved")
    assert moved > 0
    assert torch.equal(v, keep_v) and torch.equal(f, keep_f)                    # the inputs are never written


def test_the_same_call_gives_the_same_bytes_and_the_phases_are_timed():
    verts, faces = sr.mt_sphere(17, True)
    v, f = dev(verts), dev(faces)
    first = host(mesh.smooth(v, f, weights="cotangent"))
    for _ in range(3):
        assert sr.mismatches(host(mesh.smooth(v, f, weights="cotangent")), first) == []
    timed = host(mesh.smooth(v, f, weights="cotangent", timing=True))
    assert sr.mismatches(timed, first) == [] and list(timed[1]["times"]) == ["adjacency", "weights", "passes", "stats"]
    assert first[1]["negative_weights"] == 240 and first[1]["flat_corners"] == 0 and first[1]["zero_weight"] == 0 and first[1]["passes"] == 20


def test_zero_iterations_and_empty_meshes_return_the_input(monkeypatch):
    verts, faces = sr.grid_patch(9, 9)
    v, f = dev(verts), dev(faces)
    monkeypatch.setattr(lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was asked for")))
    for vv, ff, kw in ((v, f, dict(iterations=0)), (v, f[:0], dict()), (v[:0], f[:0], dict())):
        out, stats = mesh.smooth(vv, ff, **kw)
        assert out.data_ptr() != vv.data_ptr() or vv.numel() == 0
        assert np.array_equal(bits(host(out)), bits(host(vv))) and stats["passes"] == 0 and stats["max_displacement"] == 0.0
        assert stats["displacement"].shape == (vv.shape[0],) and not stats["displacement"].any()
        assert sr.mismatches(host((out, stats)), sr.smooth(host(vv), host(ff), **kw)) == []
    adj = mesh.vertex_adjacency(f[:0], 5)
    assert adj["offsets"].tolist() == [0] * 6 and adj["neighbours"].numel() == 0 and adj["degree_max"] == 0 and not adj["boundary"].any()


@pytest.mark.parametrize("bad", ("V", -1, 2 ** 31 - 1))
def test_a_bad_face_index_is_refused_before_anything_else_runs(monkeypatch, bad):
    verts, faces = sr.mt_sphere(9, False)
    faces = faces.copy()
    faces[len(faces) // 2, 1] = len(verts) if bad == "V" else bad
    seen, real = [], lib.check

    def spy(rc, what):
        seen.append(what)
        return real(rc, what)

    monkeypatch.setattr(lib, "check", spy)
    for call in (lambda: mesh.smooth(dev(verts), dev(faces), weights="cotangent"), lambda: mesh.vertex_adjacency(dev(faces), len(verts))):
        del seen[:]
        with pytest.raises(lib.MofaError, match=f"1 of the {3 * len(faces)} face indices lie outside"):
            call()
        assert seen == ["mofa_cc_validate"]


def test_non_finite_vertices_cpu_tensors_and_bad_masks_are_refused():
    verts, faces = sr.odd_mesh()
    for value in (np.nan, np.inf):
        v = verts.copy()
        v[2, 1] = value
        with pytest.raises(lib.MofaError, match="non-finite"):
            mesh.smooth(dev(v), dev(faces))
    v = verts.copy()
    v[4] = np.nan                                                               # no face references vertex 4: it keeps its NaN
    got = host(mesh.smooth(dev(v), dev(faces), iterations=2))
    assert np.array_equal(bits(got[0]), bits(sr.smooth(v, faces, iterations=2)[0])) and np.isnan(got[0][4]).all()
    v, f = dev(verts), dev(faces)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.smooth(torch.from_numpy(verts), f)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.smooth(v, torch.from_numpy(faces))
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.vertex_adjacency(torch.from_numpy(faces), 7)
    with pytest.raises(lib.MofaError, match="int32"):
        mesh.smooth(v, f.long())
    with pytest.raises(lib.MofaError, match="int32"):
        mesh.vertex_adjacency(f.long(), 7)
    for V in (-1, 2 ** 31, 7.0, True):
        with pytest.raises(lib.MofaError, match="V ="):
            mesh.vertex_adjacency(f, V)
    for pinned in (torch.zeros(6, dtype=torch.bool, device=DEV), torch.zeros(7, dtype=torch.uint8, device=DEV), torch.zeros(7, dtype=torch.bool),
                   np.zeros(7, dtype=bool)):
        with pytest.raises(lib.MofaError, match="pinned"):
            mesh.smooth(v, f, pinned=pinned)
    with pytest.raises(lib.MofaError, match="lam"):
        mesh.smooth(v, f, lam=0.0)


# ---- through the network ---------------------------------------------------------------------------------------------------------------
BOUNDS, RES = ((-1.0, -1.1, -0.9), (1.1, 0.9, 1.0)), (33, 33, 33)          # the extraction of tests/test_gpu_simplify.py


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


@pytest.mark.parametrize("extra", (dict(), dict(components="largest", simplify=2)), ids=("alone", "after_components_and_simplify"))
def test_extract_mesh_smooth_is_mesh_smooth_of_the_extraction(face, extra):
    render, net = face["render"], face["net"]
    v0, f0 = render.extract_mesh(net, **face["kw"], **extra)
    before = dict(render.mesh_stats) if extra else {}
    for weights in ("uniform", "cotangent"):
        v1, f1 = render.extract_mesh(net, smooth=3, smooth_weights=weights, **face["kw"], **extra)
        stats = dict(render.mesh_stats)
        want_v, want_s = mesh.smooth(v0.contiguous(), f0.contiguous(), iterations=3, weights=weights)
        assert torch.equal(f1, f0) and np.array_equal(bits(host(v1)), bits(host(want_v)))
        assert sr.mismatches(host((v1, stats["smooth"])), host((want_v, want_s))) == []
        assert sr.mismatches(host((v1, stats["smooth"])), sr.smooth(host(v0), host(f0), iterations=3, weights=weights)) == []
        assert stats["smooth"]["passes"] == 6 and stats["smooth"]["max_displacement"] > 0 and "edge_ids" not in stats
        assert set(stats) - {"smooth"} == set(before) - {"edge_ids"}
        print(f"{weights}: {v0.shape[0]} vertices, {stats['smooth']['n_pinned']} pinned, max displacement {stats['smooth']['max_displacement']:.5f}")


def test_normals_and_colours_are_evaluated_at_the_smoothed_vertices(face):
    render, net = face["render"], face["net"]
    kw = dict(face["kw"], refine=2, colors=True, uvCodes=face["tex"])
    v0, f0, rgb0, n0 = host(render.extract_mesh(net, normals="faces", **kw))
    verts, faces, rgb, nrm = host(render.extract_mesh(net, normals="faces", smooth=3, **kw))
    stats = dict(render.mesh_stats)
    V = len(verts)
    assert np.array_equal(faces, f0) and verts.shape == v0.shape and (bits(verts) != bits(v0)).any()
    assert np.array_equal(bits(verts), bits(sr.smooth(v0, f0, iterations=3)[0]))           # refinement ran first, on the lattice edges
    assert stats["refine"]["evaluations"] == 4 * V and stats["color_evaluations"] == V and "edge_ids" not in stats
    ref, bound = face_normals_fp64(verts, faces)
    sure = bound < 0.1
    err, err0 = np.abs(nrm - ref).max(1), np.abs(n0 - ref).max(1)
    print(f"normals='faces': {int(sure.sum())} of {V} vertices with a bound below 0.1, largest error / bound {(err / bound)[sure].max():.3f}; "
          f"the unsmoothed normals are off by up to {err0[sure].max():.3f}")
    assert sure.sum() > 0.9 * V and (err <= bound)[sure].all() and (err0 > bound)[sure].any()
    assert rgb.shape == (V, 3) and np.isfinite(rgb).all() and (rgb != rgb0).any()
    # with density normals the view directions are a function of the positions alone: the colours are the same bytes every time, and
    # the normals are those of the density field at the smoothed positions
    a = host(render.extract_mesh(net, normals="density", smooth=3, **kw))
    assert render.mesh_stats["refine"]["evaluations"] == 4 * V and render.mesh_stats["normal_evaluations"] == 6 * V
    b = host(render.extract_mesh(net, normals="density", smooth=3, **kw))
    plain = host(render.extract_mesh(net, normals="density", **kw))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.array_equal(bits(a[0]), bits(verts))
    assert (a[3] != plain[3]).any() and (a[2] != plain[2]).any()


@pytest.mark.parametrize("brick", (None, 8))
def test_smooth_none_changes_nothing(face, brick):
    render, net = face["render"], face["net"]
    kw = dict(face["kw"], brick=brick, refine=2, normals="density", colors=True, uvCodes=face["tex"])
    plain = host(render.extract_mesh(net, **kw))
    keys = set(render.mesh_stats)
    same = host(render.extract_mesh(net, smooth=None, **kw))
    assert set(render.mesh_stats) == keys and "smooth" not in keys and "edge_ids" in keys
    if brick is None:
        assert keys == {"edge_ids", "refine", "zero_normals", "normal_evaluations", "color_evaluations"}
    assert len(same) == len(plain) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(same, plain))
    render.mesh_stats = None
    bare = host(render.extract_mesh(net, **face["kw"], brick=brick))
    stats = render.mesh_stats
    again = host(render.extract_mesh(net, smooth=None, **face["kw"], brick=brick))
    assert all(np.array_equal(x, y) for x, y in zip(again, bare)) and (stats is None) == (brick is None)
    for bad in (0, -4, 2.0, True, "4"):
        with pytest.raises(lib.MofaError, match="smooth"):
            render.extract_mesh(net, smooth=bad, **face["kw"])
    with pytest.raises(lib.MofaError, match="smooth_weights"):
        render.extract_mesh(net, smooth=2, smooth_weights="cot", **face["kw"])

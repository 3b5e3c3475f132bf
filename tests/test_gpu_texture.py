"""UV texture baking on the GPU (``mofa_uv_locate`` / ``_surface`` / ``_dilate`` / ``_sample``, ``mesh.uv_locate`` / ``texel_map`` /
``texel_surface`` / ``texture_image`` / ``dilate_texture`` / ``sample_texture``, ``Renderer.bake_texture``, ``render_mesh(texture=...)``)
against the NumPy restatement (tests/uv_reference.py; tests/test_uv_reference_cpu.py shows what the comparison catches):

* ``uv_locate`` and ``texel_map`` are the restatement's — ``face`` integer for integer, ``bary`` bit for bit, the counts equal — on the whole
  catalogue for ``grid = None``, ``1`` and ``(3, 5)``, and for 1,000 seeded queries per layout (NaN, points on vertices and on edges);
* ``texel_surface`` bit for bit with and without normals, ``dilate_texture`` for 0, 1 and 5 steps, ``sample_texture`` on rasterised views;
* ``texture_image`` after streaming the sphere scene's ten frames in one call and in calls of 3 + 3 + 4: the same bytes, the restatement's;
* quality on the sphere scene and texture against vertex colours (the measured values are in the tests' docstrings);
* ``Renderer.bake_texture`` equals the hand-made sequence bit for bit; ``render_mesh`` without the new arguments is unchanged;
* every entry point and call refuses bad arguments.
"""
import numpy as np
import pytest
import torch

import bake_reference as br
import uv_reference as uvr
from harness import make_product
from mofanerf_amd import lib, mesh, synth
from mofanerf_amd.rays import pose_spherical

pytestmark = pytest.mark.gpu
DEV = "cuda"
CATALOGUE = uvr.catalogue()
NAMES = [c["name"] for c in CATALOGUE]
GRIDS = (None, 1, (3, 5))
WANT_MAPS = {(c["name"], s): uvr.texel_map(c["uvs"], c["uv_faces"], s, grid=1) for c in CATALOGUE for s in c["sizes"]}     # computed once, never modified
MAP_COUNTS = ("covered", "multi", "degenerate", "faces_without_texels")
SCENE = br.sphere_scene()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def case_of(name):
    (c,) = [c for c in CATALOGUE if c["name"] == name]
    return c


def gpu_map(c, size, grid=None):
    return mesh.texel_map(dev(c["uvs"]), dev(c["uv_faces"]), size, grid=grid)


def scene_cameras(sl=slice(None)):
    cams = SCENE["cams"][sl]
    K = np.zeros((len(cams), 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cams[:, 0], cams[:, 1], cams[:, 2], cams[:, 3], 1
    return K, cams[:, 4:].reshape(-1, 3, 4)


@pytest.mark.parametrize("name", NAMES)
def test_uv_locate_and_texel_map_equal_the_restatement(name):
    c = case_of(name)
    uvs, uv_faces = dev(c["uvs"]), dev(c["uv_faces"])
    q = uvr.random_queries(c, 1000)
    for grid in GRIDS:
        want = uvr.locate(q, c["uvs"], c["uv_faces"], grid=grid)
        got = mesh.uv_locate(dev(q), uvs, uv_faces, grid=grid)
        assert got["face"].dtype == torch.int32 and got["bary"].dtype == torch.float64 and got["grid"] == want["grid"]
        assert np.array_equal(host(got["face"]), want["face"]), (name, grid, int((host(got["face"]) != want["face"]).sum()))
        assert uvr.same_bits(host(got["bary"]), want["bary"]), (name, grid)
        assert got["counts"] == want["counts"], (name, grid, got["counts"], want["counts"])
        assert (want["face"] >= 0).any() and want["counts"]["non_finite_queries"] == 4
        for size in c["sizes"]:
            w = WANT_MAPS[name, size]
            m = mesh.texel_map(uvs, uv_faces, size if size[0] != size[1] or grid is None else size[0], grid=grid)
            assert m["size"] == size and m["n_faces"] == len(c["uv_faces"])
            assert np.array_equal(host(m["face"]), w["face"]) and uvr.same_bits(host(m["bary"]), w["bary"]), (name, size, grid)
            assert np.array_equal(host(m["covered"]), w["covered"]) and np.array_equal(host(m["index"]), w["index"]) and m["index"].dtype == torch.int64
            assert {k: m["counts"][k] for k in MAP_COUNTS} == {k: w["counts"][k] for k in MAP_COUNTS}, (name, size, grid, m["counts"])
            if grid == 1:
                assert m["counts"]["face_tests"] == w["counts"]["face_tests"]


@pytest.mark.parametrize("name", NAMES)
def test_texel_surface_equals_the_restatement(name):
    c = case_of(name)
    verts, faces = dev(c["verts"]), dev(c["faces"])
    rng = np.random.default_rng(4)
    normals = c["normals"].copy() if c["normals"] is not None else rng.normal(size=c["verts"].shape).astype(np.float32)
    normals[: len(normals) // 7] = 0                                             # normals without length: (0, 0, 0) where they meet
    for size in c["sizes"]:
        w = WANT_MAPS[name, size]
        m = gpu_map(c, size)
        for nrm in (None, normals):
            want_p, want_n = uvr.texel_surface(w, c["verts"], c["faces"], nrm)
            got_p, got_n = mesh.texel_surface(m, verts, faces, None if nrm is None else dev(nrm))
            assert got_p.dtype == got_n.dtype == torch.float32 and tuple(got_p.shape) == (w["counts"]["covered"], 3)
            assert uvr.same_bits(host(got_p), want_p) and uvr.same_bits(host(got_n), want_n), (name, size, nrm is None)


@pytest.mark.parametrize("name", ["quad", "sphere", "atlas_octahedron", "sliver"])
def test_dilate_texture_equals_the_restatement(name):
    c = case_of(name)
    size = c["sizes"][0]
    w = WANT_MAPS[name, size]
    rng = np.random.default_rng(6)
    for C in (1, 3, 5):
        texture = rng.uniform(-1, 2, size + (C,)).astype(np.float32)
        valid = w["covered"] & (rng.uniform(0, 1, size) < 0.5)
        for steps in (0, 1, 5):
            want_t, want_v, want_left = uvr.dilate(texture, valid, steps)
            got_t, got_v, left = mesh.dilate_texture(dev(texture), dev(valid), steps)
            assert uvr.same_bits(host(got_t), want_t) and np.array_equal(host(got_v), want_v) and left == want_left, (name, C, steps)
    none = mesh.dilate_texture(dev(texture), dev(np.zeros(size, bool)), 3)
    assert uvr.same_bits(host(none[0]), texture) and none[2] == size[0] * size[1]


@pytest.mark.parametrize("name", ["quad", "sphere"])
def test_sample_texture_on_rasterised_views_equals_the_restatement(name):
    c = case_of(name)
    H, W = 23, 31
    K = np.array([[1.3 * W, 0, W / 2 - 1.25], [0, 1.1 * W, H / 2 + 0.75], [0, 0, 1]], np.float32)
    centre = (0.5, 0.5, 0.0) if name == "quad" else br.SPHERE["centre"]
    poses = [np.asarray(br.pose_spherical(az, el, r, roll, shift=centre), np.float32)[:3, :4]
             for az, el, r, roll in ((90.0, -80.0, 1.6, 12.0), (35.0, -20.0, 3.0, -17.0), (-120.0, 60.0, 3.5, 40.0))]
    verts, faces, uvs, uv_faces = dev(c["verts"]), dev(c["faces"]), dev(c["uvs"]), dev(c["uv_faces"])
    rng = np.random.default_rng(8)
    hits = 0
    for C, size in ((3, (16, 32)), (1, (5, 3)), (16, (2, 2)), (4, (1, 1))):
        texture = rng.uniform(-1, 2, size + (C,)).astype(np.float32)
        for pose in poses:
            r = mesh.rasterize(verts, faces, H, W, K, pose, bary=True)
            got = mesh.sample_texture(dev(texture), r["face"], r["bary"], uvs, uv_faces, background=-0.5)
            want = uvr.sample(texture, host(r["face"]), host(r["bary"]), c["uvs"], c["uv_faces"], background=-0.5)
            assert tuple(got.shape) == (H, W, C) and uvr.same_bits(host(got), want), (name, C, size)
            hits += int((host(r["face"]) >= 0).sum())
            assert (host(got)[host(r["face"]) < 0] == -0.5).all()
    assert hits > 400, hits


def stream_texels(points, normals, batches):
    state = mesh.bake_state(points.shape[0], 3, DEV)
    first = 0
    for b in batches:
        sl = slice(first, first + b)
        K, pose = scene_cameras(sl)
        mesh.bake_integrate(state, points, dev(SCENE["images"][sl]), dev(SCENE["depth"][sl]), K, pose, normals, depth_tol=SCENE["depth_tol"],
                            cos_min=SCENE["cos_min"], power=SCENE["power"])
        first += b
    return state


def test_texture_image_streamed_equals_the_restatement():
    """The sphere scene's ten 40 x 56 frames into a 16 x 32 texture of the sphere's layout, in one call and in calls of 3 + 3 + 4."""
    c = case_of("sphere")
    size = (16, 32)
    w = WANT_MAPS["sphere", size]
    m = gpu_map(c, size)
    want_p, want_n = uvr.texel_surface(w, c["verts"], c["faces"], c["normals"])
    want_state = br.bake(dict(SCENE, verts=want_p, normals=want_n))
    points, normals = mesh.texel_surface(m, dev(c["verts"]), dev(c["faces"]), dev(c["normals"]))
    one, three = stream_texels(points, normals, [10]), stream_texels(points, normals, [3, 3, 4])
    for k in br.STATE_KEYS:
        assert uvr.same_bits(host(one[k]), want_state[k]) and uvr.same_bits(host(three[k]), want_state[k]), k
    state = mesh.texture_state(m)
    assert state["V"] == w["counts"]["covered"] and state["channels"] == 3
    for blend, fill, steps in (("mean", 0.0, 0), ("best", -1.0, 2), ("mean", 0.5, 8)):
        want = uvr.texture_image(want_state, w, blend, fill, steps)
        for st in (one, three):
            got = mesh.texture_image(st, m, blend, fill, steps)
            assert uvr.same_bits(host(got["texture"]), want["texture"]) and np.array_equal(host(got["valid"]), want["valid"]), (blend, steps)
            assert {k: got["counts"][k] for k in br.COUNTS} == want["counts"] and got["remaining"] == want["remaining"]
            assert got["counts"]["vertices"] == w["counts"]["covered"] and got["counts"]["frames"] == 10


def test_quality_on_the_sphere_scene():
    """The sphere scene (linear field, analytic normals interpolated) baked into a 64 x 128 texture through the GPU's own rasteriser.
    CONDITIONS: every covered texel is coloured, and | colour - (A x + b) | at the texel's own surface point <= the bound of DESIGN.md 3.27
    (``uv_reference.interior_bound``: 3.26's argument re-derived for face-interior points; 0.239 here).  The restatement on the CPU gives
    0.00191 (mean) / 0.00356 (best); measured on the MI355X through ``mesh.rasterize``: 0.00191 / 0.00356, all 8,192 texels coloured
    (profiles/mesh_texture.md)."""
    s = br.SPHERE
    c = case_of("sphere")
    verts, faces, normals = dev(c["verts"]), dev(c["faces"]), dev(c["normals"])
    m = gpu_map(c, (64, 128))
    assert m["counts"]["covered"] == 64 * 128
    points, pn = mesh.texel_surface(m, verts, faces, normals)
    K, poses = br.sphere_camera(), br.sphere_poses()
    attrs = dev(br.sphere_field(c["verts"]))
    state = mesh.texture_state(m)
    for pose in poses:
        r = mesh.rasterize(verts, faces, s["H"], s["W"], K, pose, attrs=attrs)
        mesh.bake_integrate(state, points, r["attr"], mesh.depth_frame(r["depth"], r["mask"]), K, pose, pn, depth_tol=s["depth_tol"],
                            cos_min=s["cos_min"], power=s["power"])
    bound, parts = uvr.interior_bound(c["verts"], c["faces"], c["normals"], br.cam_table(K, poses, len(poses)), s["depth_tol"], s["cos_min"], s["H"],
                                      s["W"])
    want = br.sphere_field(host(points)).astype(np.float64)
    for blend in ("mean", "best"):
        out = mesh.texture_image(state, m, blend)
        assert bool(out["valid"].all()) and out["counts"]["colored"] == 64 * 128 and out["remaining"] == 0, (blend, out["counts"])
        err = np.linalg.norm(host(out["texture"]).reshape(-1, 3).astype(np.float64) - want, axis=1)
        print(f"sphere texture 64 x 128, {blend}: max |colour - (A x + b)| = {err.max():.5f}, bound {bound:.5f} (slack {parts['slack']:.3f})")
        assert err.max() <= bound, (blend, err.max(), bound)


def test_the_entry_points_refuse_bad_arguments():
    L = lib.load()
    f = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
    N, T, F, V = 8, 4, 2, 4
    c = case_of("quad")
    uvs, uv_faces = dev(c["uvs"]), dev(c["uv_faces"])
    q, face, bary, counts = f(N, 2, dtype=torch.float64), f(N, dtype=torch.int32), f(N, 3, dtype=torch.float64), f(4, dtype=torch.int64)
    start, pairs = f(2, dtype=torch.int32), f(2, dtype=torch.int32)
    import ctypes as C
    o2, c2, n2 = (C.c_double * 2)(0.0, 0.0), (C.c_double * 2)(1.0, 1.0), (C.c_int32 * 2)(1, 1)
    locate = lambda q=q.data_ptr(), N=N, T=T, F=F, cell=c2, n=n2, P=0, counts=counts.data_ptr(): L.mofa_uv_locate(
        q, N, None, uvs.data_ptr(), T, uv_faces.data_ptr(), F, o2, cell, n, start.data_ptr(), pairs.data_ptr(), P, face.data_ptr(), bary.data_ptr(),
        counts, lib.stream())
    assert locate() == 0
    for kw in (dict(q=None), dict(counts=None), dict(N=0), dict(N=2 ** 31), dict(T=0), dict(F=0), dict(P=-1), dict(P=2 ** 31),
               dict(cell=(C.c_double * 2)(0.0, 1.0)), dict(cell=(C.c_double * 2)(float("nan"), 1.0)), dict(n=(C.c_int32 * 2)(0, 1)),
               dict(n=(C.c_int32 * 2)(1, 4097))):
        assert locate(**kw) != 0 and L.mofa_last_error(), kw
    verts, faces, points, normals = f(V, 3), dev(c["faces"]), f(N, 3), f(N, 3)
    surface = lambda face=face.data_ptr(), N=N, V=V, F=F, out=points.data_ptr(): L.mofa_uv_surface(
        face, bary.data_ptr(), N, verts.data_ptr(), V, faces.data_ptr(), F, None, out, normals.data_ptr(), counts.data_ptr(), lib.stream())
    assert surface() == 0
    for kw in (dict(face=None), dict(out=None), dict(N=0), dict(V=0), dict(F=0), dict(F=2 ** 31)):
        assert surface(**kw) != 0 and L.mofa_last_error(), kw
    tex, ok, tex2, ok2 = f(4, 5, 3), f(4, 5, dtype=torch.uint8), f(4, 5, 3), f(4, 5, dtype=torch.uint8)
    dilate = lambda Ht=4, Wt=5, C=3, out=tex2.data_ptr(), vout=ok2.data_ptr(): L.mofa_uv_dilate(tex.data_ptr(), ok.data_ptr(), Ht, Wt, C, out, vout,
                                                                                            lib.stream())
    assert dilate() == 0
    for kw in (dict(Ht=0), dict(Wt=0), dict(Ht=65536, Wt=32768), dict(C=0), dict(C=17), dict(out=tex.data_ptr()), dict(vout=ok.data_ptr()),
               dict(out=None)):
        assert dilate(**kw) != 0 and L.mofa_last_error(), kw
    pf, pb, out = f(N, dtype=torch.int32), f(N, 3), f(N, 3)
    sample = lambda N=N, T=T, F=F, Ht=4, Wt=5, C=3, out=out.data_ptr(), tex=tex.data_ptr(): L.mofa_uv_sample(
        pf.data_ptr(), pb.data_ptr(), N, uvs.data_ptr(), T, uv_faces.data_ptr(), F, tex, Ht, Wt, C, 0.0, out, counts.data_ptr(), lib.stream())
    assert sample() == 0
    for kw in (dict(N=0), dict(T=0), dict(F=0), dict(Ht=0), dict(Wt=0), dict(Ht=65536, Wt=32768), dict(C=0), dict(C=17), dict(out=None),
               dict(tex=None)):
        assert sample(**kw) != 0 and L.mofa_last_error(), kw
    torch.cuda.synchronize()


def test_the_kernels_skip_and_count_bad_indices():
    """What the Python layer refuses before a launch, the kernels themselves skip: a face or a vertex index outside the mesh is never
    dereferenced (``mofa_uv_surface``: NaN point, zero normal, counted; ``mofa_uv_sample``: background, counted)."""
    L = lib.load()
    c = case_of("quad")
    verts, faces, uvs = dev(c["verts"]), dev(np.array([(0, 1, 2), (0, 2, 99)], np.int32)), dev(c["uvs"])
    face = dev(np.array([0, 1, 2, -1, 0], np.int32))
    bary = dev(np.full((5, 3), 1.0 / 3.0))
    points, normals = torch.zeros(5, 3, device=DEV), torch.ones(5, 3, device=DEV)
    n = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert L.mofa_uv_surface(face.data_ptr(), bary.data_ptr(), 5, verts.data_ptr(), 4, faces.data_ptr(), 2, None, points.data_ptr(), normals.data_ptr(),
                             n.data_ptr(), lib.stream()) == 0
    assert int(n.cpu()[0]) == 3 and np.isnan(host(points)[1:4]).all() and np.isfinite(host(points)[[0, 4]]).all() and (host(normals)[1:4] == 0).all()
    out = torch.zeros(5, 3, device=DEV)
    tex = torch.ones(4, 4, 3, device=DEV)
    n.zero_()
    assert L.mofa_uv_sample(face.data_ptr(), bary.float().contiguous().data_ptr(), 5, uvs.data_ptr(), 4, faces.data_ptr(), 2, tex.data_ptr(), 4, 4, 3, 7.0,
                            out.data_ptr(), n.data_ptr(), lib.stream()) == 0
    assert int(n.cpu()[0]) == 3 and (host(out)[1:4] == 7.0).all() and (host(out)[[0, 4]] == 1.0).all()


def test_the_mesh_calls_refuse_bad_arguments():
    c = case_of("sphere")
    uvs, uv_faces, verts, faces = dev(c["uvs"]), dev(c["uv_faces"]), dev(c["verts"]), dev(c["faces"])
    q = dev(uvr.random_queries(c, 16))
    bad_index = uv_faces.clone()
    bad_index[3, 1] = len(c["uvs"])
    bad_uv = uvs.clone()
    bad_uv[5, 0] = float("nan")
    for args, kw, match in (((q.float(), uvs, uv_faces), {}, "float64"), ((q[:, :1].contiguous(), uvs, uv_faces), {}, "queries"),
                            ((q.cpu(), uvs, uv_faces), {}, "GPU"), ((q, uvs.double(), uv_faces), {}, "float32"), ((q, uvs[:, :1], uv_faces), {}, "contiguous"),
                            ((q, uvs, uv_faces.long()), {}, "int32"), ((q, uvs, uv_faces.cpu()), {}, "GPU"), ((q, uvs, bad_index), {}, "outside"),
                            ((q, bad_uv, uv_faces), {}, "not finite"), ((q, uvs, uv_faces), dict(grid=0), "grid"),
                            ((q, uvs, uv_faces), dict(grid=(1, 2, 3)), "grid"), ((q, uvs, uv_faces), dict(grid=4096), "grid"),
                            ((q, uvs, uv_faces), dict(grid=2.5), "grid")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.uv_locate(*args, **kw)
    for size, match in ((0, "size"), ((4, 4, 4), "size"), (2.5, "size"), ((65536, 32768), "2\\^31"), (True, "size")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.texel_map(uvs, uv_faces, size)
    with pytest.raises(lib.MofaError, match="outside"):
        mesh.texel_map(uvs, bad_index, 8)
    with pytest.raises(lib.MofaError, match="not finite"):
        mesh.texel_map(bad_uv, uv_faces, 8)
    empty = mesh.texel_map(uvs[:0], uv_faces[:0], (3, 4))                         # nothing to launch
    assert empty["counts"]["covered"] == 0 and tuple(empty["face"].shape) == (3, 4) and bool((empty["face"] == -1).all()) and empty["index"].numel() == 0
    none = mesh.uv_locate(q[:0], uvs, uv_faces)
    assert none["face"].numel() == 0 and none["counts"]["face_tests"] == 0
    m = mesh.texel_map(uvs, uv_faces, (8, 16))
    bad_faces = faces.clone()
    bad_faces[7, 2] = len(c["verts"])
    for args, match in (((m, verts, faces[:5]), "faces"), ((m, verts, bad_faces), "outside"), ((m, verts.double(), faces), "float32"),
                        ((m, verts, faces, verts[:5]), "normals"), ((m, verts.cpu(), faces), "GPU"), ((dict(m, face=m["face"].long()), verts, faces), "face"),
                        ((dict(m, size=(4, 4)), verts, faces), "face")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.texel_surface(*args)
    state = mesh.texture_state(m, 3)
    for args, kw, match in (((mesh.bake_state(5, 3, DEV), m), {}, "covered"), ((state, m, "median"), {}, "blend"), ((state, m), dict(fill="red"), "fill"),
                            ((state, m), dict(dilate=-1), "dilate"), ((state, m), dict(dilate=1.5), "dilate")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.texture_image(*args, **kw)
    with pytest.raises(lib.MofaError, match="channels"):
        mesh.texture_state(m, 17)
    tex, ok = torch.zeros(4, 5, 3, device=DEV), torch.zeros(4, 5, dtype=torch.bool, device=DEV)
    for args, match in (((tex, ok, -1), "iterations"), ((tex, ok, 1.5), "iterations"), ((tex, ok[:3], 1), "valid"), ((tex, ok.to(torch.uint8), 1), "valid"),
                        ((tex[..., :0], ok, 1), "texture"), ((tex[0], ok, 1), "texture"), ((tex.double(), ok, 1), "float32"), ((tex, ok.cpu(), 1), "GPU")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.dilate_texture(*args)
    face, bary = torch.zeros(3, 4, dtype=torch.int32, device=DEV), torch.zeros(3, 4, 3, device=DEV)
    for args, kw, match in (((tex, face.long(), bary, uvs, uv_faces), {}, "int32"), ((tex, face, bary[:2], uvs, uv_faces), {}, "bary"),
                            ((tex, face, bary.double(), uvs, uv_faces), {}, "float32"), ((tex[0], face, bary, uvs, uv_faces), {}, "texture"),
                            ((tex.cpu(), face, bary, uvs, uv_faces), {}, "GPU"), ((tex, face, bary, uvs, bad_index), {}, "outside"),
                            ((tex, face, bary, bad_uv, uv_faces), {}, "not finite"), ((tex, face, bary, uvs, uv_faces), dict(background="red"), "background")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.sample_texture(*args, **kw)


_PRODUCT = {}


def product():
    """The seeded product test_gpu_bake.py uses for ``bake_mesh``, built once."""
    if not _PRODUCT:
        render, kw, _ = make_product((8, 64, 8, 64), 0, 4096, DEV, with_tex=True)
        _PRODUCT.update(render=render, kw=kw)
    return _PRODUCT["render"], _PRODUCT["kw"]


def wave_frame(verts, faces, H, W, K, pose):
    """(field [H,W,3] at the rasterised surface point of every pixel — 0 where nothing is hit —, the rasteriser's dict)."""
    r = mesh.rasterize(verts, faces, H, W, K, pose, bary=True)
    corners = verts[faces.long()[r["face"].clamp(min=0).long()]].double()                     # [H,W,3 corners,3]
    point = (r["bary"].double()[..., None] * corners).sum(-2)
    field = 0.5 + 0.5 * torch.sin(2.0 * np.pi * point / 0.5)
    return (field * r["mask"][..., None]).float().contiguous(), r


def test_a_texture_shows_the_field_better_than_vertex_colours():
    """The sphere and the ten poses of the sphere scene; the frames show the field 0.5 + 0.5 sin(2 pi x_k / 0.5), evaluated per pixel at
    the rasterised surface point.  Baked into vertex colours and into a 64 x 128 texture, both rendered from a held-out eleventh pose with
    ``render_mesh``.  CONDITION: the textured view's mean |error| against the field on the mask is below HALF the vertex-coloured view's.
    The restatement on the CPU gives 0.0194 against 0.2056 (point-level probe of the issue: 0.013 against 0.167); measured on the
    MI355X: texture 0.0194, vertex colours 0.2056 (profiles/mesh_texture.md)."""
    s = br.SPHERE
    c = case_of("sphere")
    render, _ = product()
    verts, faces, normals, uvs, uv_faces = (dev(c[k]) for k in ("verts", "faces", "normals", "uvs", "uv_faces"))
    K, poses = br.sphere_camera(), br.sphere_poses()
    H, W = s["H"], s["W"]
    m = mesh.texel_map(uvs, uv_faces, (64, 128))
    points, pn = mesh.texel_surface(m, verts, faces, normals)
    texels, vertices = mesh.texture_state(m), mesh.bake_state(len(c["verts"]), 3, DEV)
    kw = dict(depth_tol=s["depth_tol"], cos_min=s["cos_min"], power=s["power"])
    for pose in poses:
        frame, r = wave_frame(verts, faces, H, W, K, pose)
        depth = mesh.depth_frame(r["depth"], r["mask"])
        mesh.bake_integrate(texels, points, frame, depth, K, pose, pn, **kw)
        mesh.bake_integrate(vertices, verts, frame, depth, K, pose, normals, **kw)
    image = mesh.texture_image(texels, m, dilate=2)
    colors = mesh.bake_colors(vertices)
    assert image["counts"]["colored"] == 64 * 128 and bool(colors["valid"].all())
    pose = np.asarray(pose_spherical(22.5, 0.0, s["distance"]), np.float32)[:3, :4].copy()
    pose[:, 3] += np.asarray(s["centre"], np.float32)                                         # look at the sphere's centre from a pose of no frame
    want, r = wave_frame(verts, faces, H, W, K, pose)
    mask = r["mask"]
    assert int(mask.sum()) > 300
    textured = render.render_mesh(H, W, K, pose, verts, faces, texture=image["texture"], uvs=uvs, uv_faces=uv_faces)
    coloured = render.render_mesh(H, W, K, pose, verts, faces, colors=colors["colors"])
    assert torch.equal(textured[2], mask) and torch.equal(coloured[2], mask) and "bary" in textured[3]
    err_t = float((textured[0] - want).abs()[mask].mean())
    err_v = float((coloured[0] - want).abs()[mask].mean())
    print(f"held-out view, mean |error| on the mask: texture {err_t:.4f}, vertex colours {err_v:.4f}")
    assert err_t < 0.5 * err_v, (err_t, err_v)


def test_render_mesh_without_the_new_arguments_is_unchanged():
    """One fixed input: the call without the new arguments, the call that passes ``texture=None`` explicitly and (for colours) the
    ``colors=``-only call give the bytes of the code path of the parent commit, restated here: ``mesh.rasterize(attrs=colors)``'s ``attr``,
    and the head-light shade of ``mesh.rasterize(normals=True)``."""
    from mofanerf_amd.rays import get_rays
    render, _ = product()
    c = case_of("sphere")
    verts, faces, uvs, uv_faces = (dev(c[k]) for k in ("verts", "faces", "uvs", "uv_faces"))
    H, W = 23, 31
    K = br.sphere_camera()
    pose = br.sphere_poses()[1]
    colors = dev(br.sphere_field(c["verts"]))
    plain = render.render_mesh(H, W, K, pose, verts, faces, colors=colors)
    explicit = render.render_mesh(H, W, K, pose, verts, faces, colors=colors, texture=None, uvs=None, uv_faces=None)
    parent = mesh.rasterize(verts, faces, H, W, K, pose, attrs=colors, znear=1e-3)
    for got in (plain, explicit):
        assert torch.equal(got[0], parent["attr"]) and torch.equal(got[1], parent["depth"]) and torch.equal(got[2], parent["mask"])
        assert set(got[3]) == {"face", "counts"} and torch.equal(got[3]["face"], parent["face"])
    shaded = render.render_mesh(H, W, K, pose, verts, faces)
    shaded_explicit = render.render_mesh(H, W, K, pose, verts, faces, texture=None)
    out = mesh.rasterize(verts, faces, H, W, K, pose, znear=1e-3, normals=True)
    _, d = get_rays(H, W, K, pose, device=verts.device)
    view = d / d.norm(dim=-1, keepdim=True)
    shade = 0.3 + (1. - 0.3) * (-(out["normal"] * view).sum(-1)).clamp(min=0.)
    want = (shade * out["mask"].to(torch.float32))[..., None].expand(H, W, 3)
    for got in (shaded, shaded_explicit):
        assert torch.equal(got[0], want) and torch.equal(got[1], out["depth"]) and set(got[3]) == {"face", "counts", "normal"}
    texture = torch.rand(8, 16, 3, device=DEV)
    for kw, match in ((dict(colors=colors, texture=texture, uvs=uvs, uv_faces=uv_faces), "colors and texture"), (dict(texture=texture), "go together"),
                      (dict(uvs=uvs, uv_faces=uv_faces), "go together"), (dict(texture=texture[..., :2], uvs=uvs, uv_faces=uv_faces), "Ht,Wt,3"),
                      (dict(texture=texture, uvs=uvs, uv_faces=uv_faces[:5]), "per face")):
        with pytest.raises(lib.MofaError, match=match):
            render.render_mesh(H, W, K, pose, verts, faces, **kw)
    path = render.render_path_mesh([np.concatenate([pose, [[0, 0, 0, 1]]]).astype(np.float32)], (H, W, None), K, verts, faces, texture=texture, uvs=uvs,
                                   uv_faces=uv_faces)
    one = render.render_mesh(H, W, K, pose, verts, faces, texture=texture, uvs=uvs, uv_faces=uv_faces)
    assert uvr.same_bits(path["rgb"][0], host(one[0]))


def test_renderer_bake_texture_is_the_hand_made_sequence():
    render, kw = product()
    H = W = 16
    K = synth.intrinsics(H, W)
    poses = [pose_spherical(az, el, 16.0)[:3, :4] for az, el in ((-30.0, 10.0), (0.0, -5.0), (40.0, 20.0))]
    bm, tex, exp = (x.to(DEV) for x in synth.codes(0))
    bounds, res = ((-3.0, -3.0, -3.0), (3.0, 3.5, 4.0)), (9, 9, 9)
    net = kw["network_fine"]
    level = float(render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm, expCodes=exp).median())
    verts, faces = (t.contiguous() for t in render.extract_mesh(net, bounds=bounds, resolution=res, level=level, shapeCodes=bm, expCodes=exp))
    F = int(faces.shape[0])
    assert verts.shape[0] > 50
    normals = mesh.vertex_normals(verts, faces).contiguous()                  # (a float index_add_ with no fixed order: computed ONCE)
    size = mesh.face_atlas(F, 4096)[2]["n"] * 6
    atlas_uvs, atlas_faces, _ = mesh.face_atlas(F, size)
    uvs, uv_faces = dev(atlas_uvs), dev(atlas_faces)
    rk = {k: v for k, v in kw.items() if k != "ndc"}
    codes = dict(shapeCodes=bm, uvCodes=tex, expCodes=exp, expType=20)
    for blend, cos_min, power, dilate in (("mean", 0.0, 2, 0), ("best", 0.2, 1, 3)):
        texture, valid, stats = render.bake_texture(poses, H, W, K, verts, faces, uvs, uv_faces, size=size, depth_tol=0.5, blend=blend, cos_min=cos_min,
                                                    power=power, dilate=dilate, normals=normals, **codes, **rk)
        m = mesh.texel_map(uvs, uv_faces, size)
        points, pn = mesh.texel_surface(m, verts, faces, normals)
        state = mesh.texture_state(m)
        for pose in poses:
            with torch.no_grad():                                              # bake_texture renders for inference: nothing is taped
                rgb = render.render_fitting(H, W, K, c2w=pose, **codes, **dict(rk, ndc=False))[0]
            r = mesh.rasterize(verts, faces, H, W, K, pose)
            mesh.bake_integrate(state, points, rgb.reshape(H, W, 3).contiguous(), mesh.depth_frame(r["depth"], r["mask"]), K, pose, pn,
                                depth_tol=0.5, cos_min=cos_min, power=power)
        render.check_launches(block=True)
        for k in br.STATE_KEYS:
            assert uvr.same_bits(host(render.bake_state[k]), host(state[k])), (blend, k)
        want = mesh.texture_image(state, m, blend, 0.0, dilate)
        assert uvr.same_bits(host(texture), host(want["texture"])) and torch.equal(valid, want["valid"]) and tuple(texture.shape) == (size, size, 3)
        assert {k: stats[k] for k in br.COUNTS} == {k: want["counts"][k] for k in br.COUNTS} and stats["frames"] == 3
        assert stats["colored"] > 0 and stats["remaining"] == want["remaining"] and render.bake_stats is stats
        assert {k: stats[k] for k in MAP_COUNTS} == {k: m["counts"][k] for k in MAP_COUNTS} and stats["multi"] == 0 and stats["vertices"] == stats["covered"]
        assert stats["faces_without_texels"] == 0 and stats["size"] == (size, size) and torch.equal(render.bake_map["index"], m["index"])
        assert len(stats["hit_share"]) == 3 and all(0.0 < s <= 1.0 for s in stats["hit_share"])
        assert set(stats["times"]) == {"texel_map", "render", "rasterize", "integrate", "resolve"} and all(t >= 0 for t in stats["times"].values())
        print(f"bake_texture, {blend}: {stats['colored']} of {stats['covered']} texels coloured ({size} x {size}, {F} faces), occluded "
              f"{stats['occluded']}, grazing {stats['grazing']}, unseen {stats['unseen']}, remaining {stats['remaining']}")
    with pytest.raises(lib.MofaError, match="ndc"):
        render.bake_texture(poses, H, W, K, verts, faces, uvs, uv_faces, size=size, depth_tol=0.5, **codes, **dict(rk, ndc=True))
    for bad, match in ((dict(depth_tol=-1.0), "depth_tol"), (dict(blend="median"), "blend"), (dict(cos_min=1.0), "cos_min"), (dict(power=9), "power"),
                       (dict(dilate=-1), "dilate"), (dict(size=0), "size"), (dict(size=(4, 4, 4)), "size")):
        with pytest.raises(lib.MofaError, match=match):
            render.bake_texture(poses, H, W, K, verts, faces, uvs, uv_faces, **dict(dict(size=size, depth_tol=0.5, **codes, **rk), **bad))
    with pytest.raises(lib.MofaError, match="no poses"):
        render.bake_texture([], H, W, K, verts, faces, uvs, uv_faces, size=size, depth_tol=0.5, **codes, **rk)
    with pytest.raises(lib.MofaError, match="UV faces"):
        render.bake_texture(poses, H, W, K, verts, faces, uvs, uv_faces[:5], size=size, depth_tol=0.5, **codes, **rk)
    # the default size is the encoder's: a 512 x 512 result goes through texEncoder and gives a finite code of the texture code's length
    big_uvs, big_faces, _ = mesh.face_atlas(F, 512)
    texture, valid, stats = render.bake_texture(poses[:1], H, W, K, verts, faces, dev(big_uvs), dev(big_faces), depth_tol=0.5, normals=normals, **codes, **rk)
    assert tuple(texture.shape) == (512, 512, 3) and stats["size"] == (512, 512) and stats["dilate"] == 8
    with torch.no_grad():
        code = render.texEncoder(texture.permute([2, 0, 1]).unsqueeze(0), None)[0]
    assert code.numel() == tex.numel() and bool(torch.isfinite(code).all())

"""The mesh rasteriser on the GPU (``mofa_raster_project`` / ``_faces`` / ``_resolve``, ``mesh.rasterize``, ``mesh.depth_agreement``,
``Renderer.render_mesh`` / ``render_path_mesh``) against the NumPy restatement of tests/raster_reference.py, which
tests/test_raster_reference_cpu.py holds against an independent fp64 ray caster.

Every frame is compared BIT FOR BIT: the fp32 steps are separately rounded operations in a fixed order, coverage is integer arithmetic,
interpolation is fp64 rounded once, and the z-buffer's key makes the winner of a pixel independent of the order of the atomics.  Outputs sit
in guarded buffers; each call is made twice and must give the same bits."""
import os

import numpy as np
import pytest
import torch

import occ_reference as occ
import raster_reference as ref
from mofanerf_amd import lib, mesh
from mofanerf_amd.rays import get_rays, pose_spherical
from mofanerf_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
MAX = ref.INT32_MAX
DEFAULT = mesh.WAVE_MIN_PIXELS
BUFFERS = ("depth", "face", "bary", "normal", "attr")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype, fill):
    whole = torch.full((shape[0] + 2 * GUARD, *shape[1:]), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + shape[0]]


def guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def gpu_frame(verts, faces, H, W, K, c2w, attrs=None, znear=1e-3, wmp=DEFAULT, **_):
    """The frame through the C ABI, as numpy: two runs that must agree bit for bit and leave the words around every output alone."""
    L = lib.load()
    v, f = dev(np.asarray(verts, np.float32).reshape(-1, 3)), dev(np.asarray(faces, np.int32).reshape(-1, 3))
    a = None if attrs is None else dev(np.asarray(attrs, np.float32))
    C = 1 if a is None else a.shape[1]
    V, F, P = len(v), len(f), H * W
    fx, fy, cx, cy = (float(x) for x in ref.intrinsics(K))
    pose = dev(ref.pose34(c2w))
    nbytes = L.mofa_raster_workspace_bytes(V, F, H, W)
    assert nbytes > 0
    got = []
    for _ in range(2):
        wsw, ws = guarded((nbytes,), torch.uint8, 0x5A)
        bufs = {"depth": guarded((P,), torch.float32, 7.0), "face": guarded((P,), torch.int32, -77), "bary": guarded((P, 3), torch.float32, 7.0),
                "normal": guarded((P, 3), torch.float32, 7.0), "counts": guarded((4,), torch.int64, -77)}
        if a is not None:
            bufs["attr"] = guarded((P, C), torch.float32, 7.0)
        lib.check(L.mofa_raster_project(v.data_ptr(), V, F, H, W, fx, fy, cx, cy, lib.ptr(pose), float(znear), ws.data_ptr(), lib.stream()),
                  "mofa_raster_project")
        lib.check(L.mofa_raster_faces(f.data_ptr(), F, V, H, W, int(wmp), ws.data_ptr(), bufs["counts"][1].data_ptr(), lib.stream()),
                  "mofa_raster_faces")
        lib.check(L.mofa_raster_resolve(v.data_ptr(), V, f.data_ptr(), F, lib.ptr(a), C, H, W, fx, fy, cx, cy, lib.ptr(pose), ws.data_ptr(),
                                        lib.ptr(bufs["depth"][1]), bufs["face"][1].data_ptr(), lib.ptr(bufs["bary"][1]),
                                        lib.ptr(bufs["attr"][1]) if a is not None else None, lib.ptr(bufs["normal"][1]), lib.stream()),
                  "mofa_raster_resolve")
        assert guards_intact(wsw, 0x5A)
        for k, (whole, _) in bufs.items():
            assert guards_intact(whole, -77 if k in ("face", "counts") else 7.0), k
        got.append({k: t.cpu().numpy().reshape((H, W) + tuple(t.shape[1:])) if k != "counts" else t.cpu().numpy() for k, (_, t) in bufs.items()})
    assert all(ref.same_bits(got[0][k], got[1][k]) for k in got[0])
    return got[0]


def want_frame(s, attrs=None, znear=1e-3, wmp=DEFAULT):
    return ref.rasterize(s["verts"], s["faces"], s["H"], s["W"], s["K"], s["c2w"], attrs=attrs, znear=znear, wave_min_pixels=wmp)


def assert_same(got, want, what=""):
    for k in BUFFERS:
        if k in want:
            assert ref.same_bits(got[k], want[k]), (what, k, np.argwhere(got[k].reshape(want[k].shape[0], want[k].shape[1], -1).view(np.uint32)
                                                                         != want[k].reshape(want[k].shape[0], want[k].shape[1], -1).view(np.uint32))[:6])
    assert got["counts"].tolist() == want["counts"].tolist(), (what, got["counts"], want["counts"])


def check_scene(s, attrs=None, znear=1e-3, wmps=(0, MAX)):
    """GPU == restatement under each wave_min_pixels; returns the GPU frame of the last."""
    for wmp in wmps:
        got = gpu_frame(**s, attrs=attrs, znear=znear, wmp=wmp)
        assert_same(got, want_frame(s, attrs, znear, wmp), wmp)
    return got


# ---- 1. scenes A, B and C (C: fx != fy, a generic pose) -----------------------------------------------------------------------------------------------------------------
_cache = {}


def scene_reference(name):
    """(scene, attrs [V,16], {wave_min_pixels: restated frame}) — computed once."""
    if name not in _cache:
        s = {"A": ref.scene_a, "B": ref.scene_b, "C": ref.scene_c}[name]()
        attrs = np.random.default_rng(7).normal(size=(len(s["verts"]), 16)).astype(np.float32)
        full = want_frame(s, attrs, wmp=MAX)
        frames = {MAX: full}
        for wmp in (0, 16, DEFAULT):                    # only the fourth counter depends on it
            frames[wmp] = dict(full, counts=want_frame(s, wmp=wmp)["counts"])
            assert frames[wmp]["counts"][:3].tolist() == full["counts"][:3].tolist()
        _cache[name] = (s, attrs, frames)
    return _cache[name]


@pytest.mark.parametrize("wmp", sorted({0, 16, DEFAULT, MAX}))
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_scenes_are_the_restatement_bit_for_bit_on_either_path(name, wmp):
    s, attrs, frames = scene_reference(name)
    want = frames[wmp]
    for C in (16, 3, 1):
        got = gpu_frame(**s, attrs=attrs[:, :C], wmp=wmp)
        assert_same(got, dict(want, attr=np.ascontiguousarray(want["attr"][..., :C])), (name, wmp, C))
    drawn, wave = int(got["counts"][0]), int(got["counts"][3])
    assert wave == (drawn if wmp == 0 else 0 if wmp == MAX else wave)
    if name == "A" and wmp == 16:
        assert 0 < wave < drawn                         # both paths in one frame
    assert (got["face"] >= 0).sum() > 300


# ---- 2. one face over the whole image ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(29, 37), (1, 1), (1, 64), (64, 1)])
def test_one_face_far_larger_than_the_image_covers_every_pixel(H, W):
    cam = ref.exact_camera(H, W, 3.0, 2.0)
    s = dict(cam, verts=ref.at_pixels([(-1000, -1000), (3000, -1000), (-1000, 3000)], 3.0, 2.0), faces=np.asarray([(0, 1, 2)], np.int32))
    for wmp in (0, DEFAULT, MAX):
        got = gpu_frame(**s, wmp=wmp)
        assert_same(got, want_frame(s, wmp=wmp), wmp)
        assert (got["face"] == 0).all() and (got["depth"] == 1.0).all()
        assert got["counts"].tolist() == [1, 0, 0, 0 if wmp == MAX or H * W < wmp else 1]


# ---- 3. exact edges ----------------------------------------------------------------------------------------------------------------------
def test_samples_exactly_on_edges_and_vertices():
    n = 8
    s = ref.quad_scene(n)
    got = check_scene(s)
    inside = np.zeros((s["H"], s["W"]), bool)
    inside[2:2 + n + 1, 2:2 + n + 1] = True
    assert np.array_equal(got["face"] >= 0, inside)                               # interior, border and the four corners (vertices)
    jj, ii = np.nonzero(inside)
    assert np.array_equal(got["face"][jj, ii], np.where(ii >= jj, 0, 1))           # the diagonal belongs to both: the lower index has it
    assert (got["depth"][inside] == 1.0).all()
    # the same faces twice: the first copy wins everywhere
    twice = check_scene(ref.quad_scene(n, doubled=True))
    assert np.array_equal(twice["face"], got["face"]) and ref.same_bits(twice["depth"], got["depth"])


def test_a_fan_around_a_vertex_at_a_pixel_centre():
    cam = ref.exact_camera(17, 19, 3.0, 2.0)
    ring = [(14, 8), (11, 13), (5, 13), (2, 8), (5, 3), (11, 3)]
    s = dict(cam, verts=ref.at_pixels([(8, 8)] + ring, 3.0, 2.0), faces=np.asarray([(0, 1 + k, 1 + (k + 1) % 6) for k in range(6)], np.int32))
    got = check_scene(s)
    # the hexagon in exact integers: every sample inside or on it is covered, no other
    inside = np.ones((17, 19), bool)
    j, i = np.mgrid[0:17, 0:19]
    for (ax, ay), (bx, by) in zip(ring, ring[1:] + ring[:1]):
        inside &= (bx - ax) * (j - ay) - (by - ay) * (i - ax) >= 0
    assert inside.sum() > 80 and np.array_equal(got["face"] >= 0, inside)
    assert got["face"][8, 8] == 0                                                 # the hub belongs to all six
    assert got["face"][8, 9] == 0 and got["face"][8, 7] == 2                      # the spokes along the row: faces 5|0 and 2|3


# ---- 4. occlusion ------------------------------------------------------------------------------------------------------------------------
def test_the_nearer_face_wins_per_pixel():
    cam = ref.exact_camera(14, 15, 3.0, 2.0)
    far = ref.at_pixels([(2, 2), (10, 2), (10, 10), (2, 10)], 3.0, 2.0, z=-2.0)
    near = ref.at_pixels([(4, 4), (8, 4), (8, 8), (4, 8)], 3.0, 2.0, z=-1.0)
    quad = [(0, 1, 2), (0, 2, 3)]
    for order in (0, 1):                                   # whichever comes first in the face list
        verts = np.concatenate([far, near] if order == 0 else [near, far])
        s = dict(cam, verts=verts, faces=np.asarray(quad + [tuple(4 + k for k in t) for t in quad], np.int32))
        got = check_scene(s)
        want = np.zeros((14, 15), np.float32)
        want[2:11, 2:11] = 2.0
        want[4:9, 4:9] = 1.0
        assert ref.same_bits(got["depth"], want)
        assert ((got["face"] >= 2) == ((want == 1.0) if order == 0 else (want == 2.0))).all()
    # two faces that pass through each other: the per-pixel minimum of the two alone
    px = [(2, 2), (12, 2), (2, 12)]                         # one triangle on the screen, two sets of depths that cross inside it
    a = np.concatenate([ref.at_pixels([p], 3.0, 2.0, z=-z) for p, z in zip(px, (1.0, 4.0, 2.0))])
    b = np.concatenate([ref.at_pixels([p], 3.0, 2.0, z=-z) for p, z in zip(px, (3.0, 1.0, 3.0))])
    both = dict(cam, verts=np.concatenate([a, b]), faces=np.asarray([(0, 1, 2), (3, 4, 5)], np.int32))
    got = check_scene(both)
    one = [gpu_frame(**dict(both, faces=both["faces"][k:k + 1])) for k in (0, 1)]
    d = [np.where(o["face"] >= 0, o["depth"], np.inf) for o in one]
    overlap = np.isfinite(d[0]) & np.isfinite(d[1])
    assert overlap.sum() >= 4 and (d[0] < d[1])[overlap].any() and (d[1] < d[0])[overlap].any()
    assert np.array_equal(np.where(got["face"] >= 0, got["depth"], np.inf), np.minimum(d[0], d[1]))
    assert np.array_equal(got["face"], np.where(np.isinf(np.minimum(d[0], d[1])), -1, np.where(d[0] <= d[1], 0, 1)))


# ---- 5. culling and the counters ---------------------------------------------------------------------------------------------------------
def test_culled_degenerate_and_off_screen_faces_are_counted_and_leave_no_pixel():
    cam = ref.exact_camera(16, 16, 3.0, 2.0)
    tri = [(2, 2), (12, 3), (4, 13)]
    groups = {                                             # name -> (vertices, kind)
        "visible": (ref.at_pixels(tri, 3.0, 2.0), "drawn"),
        "behind": (ref.at_pixels(tri, 3.0, 2.0, z=1.0), "culled"),
        "straddles_znear": (ref.at_pixels(tri, 3.0, 2.0) * np.float32([[1, 1, 1], [1, 1, 1], [0.25, 0.25, 0.25]]), "culled"),
        "nan": (ref.at_pixels(tri, 3.0, 2.0) + np.float32([[np.nan, 0, 0], [0, 0, 0], [0, 0, 0]]), "culled"),
        "inf": (ref.at_pixels(tri, 3.0, 2.0) + np.float32([[0, 0, 0], [0, np.inf, 0], [0, 0, 0]]), "culled"),
        "guard_band": (ref.at_pixels([(2, 2), (12, 3), (2.0 ** 20 + 64, 13)], 3.0, 2.0), "culled"),
        "collinear": (ref.at_pixels([(2, 2), (6, 4), (10, 6)], 3.0, 2.0), "degenerate"),
        "off_screen": (ref.at_pixels([(100, 100), (140, 103), (104, 150)], 3.0, 2.0), "drawn"),
    }
    verts = np.concatenate([v for v, _ in groups.values()])
    faces = [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(groups))]
    V = len(verts)
    faces += [(0, 1, -1), (0, V, 2), (0, 0, 1)]           # indices -1 and n_verts: culled; a repeated index: degenerate
    s = dict(cam, verts=verts, faces=np.asarray(faces, np.int32))
    for wmp in (0, DEFAULT, MAX):
        got = gpu_frame(**s, znear=0.5, wmp=wmp)
        assert_same(got, want_frame(s, znear=0.5, wmp=wmp), wmp)
        # the visible face's box holds 11 x 12 samples, the off-screen face's none
        assert got["counts"].tolist() == [2, 7, 2, 0 if wmp == MAX else int(132 >= wmp) + int(0 >= wmp)]
        assert set(np.unique(got["face"])) == {-1, 0}
    # each on its own, next to the visible face
    for k, (name, (_, kind)) in enumerate(groups.items()):
        one = dict(s, faces=np.asarray([faces[0], faces[k]], np.int32))
        got = gpu_frame(**one, znear=0.5)
        assert_same(got, want_frame(one, znear=0.5), name)
        assert got["counts"][:3].tolist() == [1 + (kind == "drawn"), int(kind == "culled"), int(kind == "degenerate")], name
        assert (got["face"] <= 0).all() if name != "visible" else True


# ---- 6. winding --------------------------------------------------------------------------------------------------------------------------
def test_reversed_faces_cover_the_same_pixels():
    s, _, frames = scene_reference("A")
    got = gpu_frame(**s)
    rev = dict(s, faces=np.ascontiguousarray(s["faces"][:, ::-1]))
    back = gpu_frame(**rev)
    assert_same(back, want_frame(rev), "reversed")
    assert np.array_equal(back["face"], got["face"]) and back["counts"].tolist() == got["counts"].tolist()
    # the fp64 sum is taken in another order before the single rounding
    assert np.abs(back["depth"].view(np.int32).astype(np.int64) - got["depth"].view(np.int32)).max() <= 1


# ---- 7. empty and refused ----------------------------------------------------------------------------------------------------------------
def test_empty_meshes_give_empty_frames_and_bad_arguments_are_refused():
    s = ref.scene_a()
    for verts, faces in ((s["verts"], np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), s["faces"][:5]),
                         (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        e = dict(s, verts=verts, faces=faces)
        attrs = np.zeros((len(verts), 3), np.float32)
        for wmp in (0, MAX):
            got = gpu_frame(**e, attrs=attrs, wmp=wmp)
            assert_same(got, want_frame(e, attrs, wmp=wmp))
            assert (got["face"] == -1).all() and not any(got[k].any() for k in ("depth", "bary", "normal", "attr"))
            assert got["counts"].tolist() == [0, len(faces), 0, 0]
    v, f = dev(s["verts"]), dev(s["faces"])
    args = (s["H"], s["W"], s["K"], s["c2w"])
    with pytest.raises(lib.MofaError, match="H = 0"):
        mesh.rasterize(v, f, 0, s["W"], s["K"], s["c2w"])
    with pytest.raises(lib.MofaError, match="C = 17"):
        mesh.rasterize(v, f, *args, attrs=torch.zeros(len(v), 17, device=DEV))
    with pytest.raises(lib.MofaError, match="znear"):
        mesh.rasterize(v, f, *args, znear=0.0)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.rasterize(v.cpu(), f, *args)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.rasterize(v, f.cpu(), *args)
    # the library refuses them itself
    L = lib.load()
    ws = torch.zeros(L.mofa_raster_workspace_bytes(len(v), len(f), 8, 8), dtype=torch.uint8, device=DEV)
    pose, out = dev(s["c2w"]), torch.zeros(8 * 8 * 17, device=DEV)
    assert L.mofa_raster_project(v.data_ptr(), len(v), len(f), 8, 8, 1., 1., 0., 0., lib.ptr(pose), 0.0, ws.data_ptr(), lib.stream()) == -1
    assert b"znear" in L.mofa_last_error()
    assert L.mofa_raster_project(v.data_ptr(), len(v), len(f), 0, 8, 1., 1., 0., 0., lib.ptr(pose), 0.1, ws.data_ptr(), lib.stream()) == -1
    assert b"H = 0" in L.mofa_last_error()
    assert L.mofa_raster_resolve(v.data_ptr(), len(v), f.data_ptr(), len(f), lib.ptr(out), 17, 8, 8, 1., 1., 0., 0., lib.ptr(pose), ws.data_ptr(),
                                 lib.ptr(out), ws.data_ptr(), None, lib.ptr(out), None, lib.stream()) == -1
    assert b"C = 17" in L.mofa_last_error()


# ---- 8. a mesh of the project's own ------------------------------------------------------------------------------------------------------
BALL = dict(centre=(0.1, -0.05, 0.2), radius=1.0, res=(17, 17, 17), bounds=((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)))


def ball_view():
    if "ball" not in _cache:
        res, lo, step = mesh.grid_spec(BALL["bounds"], BALL["res"])
        verts, faces = mesh.iso_surface(dev(occ.ball_grid(res, lo, step, BALL["centre"], BALL["radius"])), 0.0, lo, step)
        s = dict(verts=verts.cpu().numpy(), faces=faces.cpu().numpy(), H=32, W=32, K=ref.camera(32, 32), c2w=ref.pose34(pose_spherical(25.0, -20.0, 4.0)))
        colors = np.random.default_rng(3).uniform(0, 1, (len(s["verts"]), 3)).astype(np.float32)
        _cache["ball"] = (s, verts, faces, colors, want_frame(s, colors))
    return _cache["ball"]


def test_a_marching_tetrahedra_mesh_is_the_restatement_and_meets_the_ray_caster():
    s, verts, faces, colors, want = ball_view()
    assert len(s["faces"]) > 1000
    out = mesh.rasterize(verts, faces, s["H"], s["W"], s["K"], s["c2w"], attrs=dev(colors), bary=True, normals=True)
    assert set(out) == {"depth", "face", "mask", "counts", "bary", "attr", "normal"}
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert_same(got, want)
    assert np.array_equal(got["mask"], want["face"] >= 0) and got["mask"].dtype == np.bool_
    lean = mesh.rasterize(verts, faces, s["H"], s["W"], s["K"], s["c2w"])
    assert set(lean) == {"depth", "face", "mask", "counts"} and ref.same_bits(lean["depth"].cpu().numpy(), want["depth"])
    a = ref.agreement(got, ref.raycast(s["verts"], s["faces"], s["H"], s["W"], s["K"], s["c2w"]), s["verts"], s["faces"], s["K"], s["c2w"])
    print(a)
    assert a["covered"] > 150 and a["disagree"] <= ref.DISAGREE_CAP and a["outside"] == 0, a


# ---- 9. the renderer's views -------------------------------------------------------------------------------------------------------------
def test_render_mesh_and_render_path_mesh(tmp_path):
    s, verts, faces, colors, want = ball_view()
    H, W, K = s["H"], s["W"], s["K"]
    render = Renderer()
    rgb, depth, mask, ex = render.render_mesh(H, W, K, s["c2w"], verts, faces, colors=dev(colors))
    assert ref.same_bits(rgb.cpu().numpy(), want["attr"]) and ref.same_bits(depth.cpu().numpy(), want["depth"])
    assert np.array_equal(mask.cpu().numpy(), want["face"] >= 0) and ref.same_bits(ex["face"].cpu().numpy(), want["face"])
    assert ex["counts"].cpu().numpy().tolist() == want["counts"].tolist()
    shade, depth2, mask2, ex2 = render.render_mesh(H, W, K, s["c2w"], verts, faces, ambient=0.25)
    assert ref.same_bits(ex2["normal"].cpu().numpy(), want["normal"]) and ref.same_bits(depth2.cpu().numpy(), want["depth"])
    _, d = get_rays(H, W, K, torch.from_numpy(s["c2w"]), device=DEV)
    formula = 0.25 + 0.75 * (-(ex2["normal"] * (d / d.norm(dim=-1, keepdim=True))).sum(-1)).clamp(min=0.)
    assert torch.equal(shade, (formula * mask2.to(torch.float32))[..., None].expand(H, W, 3))
    lit = shade[..., 0][mask2]
    assert bool((lit >= 0.25).all()) and bool((lit <= 1.0 + 1e-6).all()) and float(lit.max()) > 0.9 and not bool(shade[~mask2].any())
    # the path: two poses, files, skipping
    poses = [pose_spherical(25.0, -20.0, 4.0), pose_spherical(-60.0, 10.0, 4.5)]
    out = render.render_path_mesh(poses, (H, W, float(K[0][0])), K, verts, faces, colors=dev(colors), savedir=str(tmp_path))
    names = sorted(f"{i:03d}_{what}.png" for i in (0, 1) for what in ("mesh", "mesh_depth"))
    assert out["rendered"] == [0, 1] and out["skipped"] == [] and sorted(os.listdir(tmp_path)) == names
    assert out["rgb"].shape == (2, H, W, 3) and out["depth"].shape == out["mask"].shape == out["face"].shape == (2, H, W)
    assert ref.same_bits(out["rgb"][0], want["attr"]) and ref.same_bits(out["depth"][0], want["depth"])
    second = ref.rasterize(s["verts"], s["faces"], H, W, K, ref.pose34(poses[1]))
    assert ref.same_bits(out["depth"][1], second["depth"]) and ref.same_bits(out["face"][1], second["face"])
    stamps = {n: os.stat(tmp_path / n).st_mtime_ns for n in names}
    again = render.render_path_mesh(poses, (H, W, float(K[0][0])), K, verts, faces, colors=dev(colors), savedir=str(tmp_path))
    assert again == {"rendered": [], "skipped": [0, 1]} and {n: os.stat(tmp_path / n).st_mtime_ns for n in names} == stamps
    os.remove(tmp_path / "001_mesh_depth.png")
    third = render.render_path_mesh(poses, (H, W, float(K[0][0])), K, verts, faces, colors=dev(colors), savedir=str(tmp_path))
    assert third["rendered"] == [1] and third["skipped"] == [0] and ref.same_bits(third["depth"][0], out["depth"][1])
    assert sorted(os.listdir(tmp_path)) == names


# ---- 10. agreement with a volume's depth -------------------------------------------------------------------------------------------------
def test_depth_agreement_of_the_ball_with_its_analytic_depth():
    s, verts, faces, _, want = ball_view()
    H, W = s["H"], s["W"]
    # the "volume": the analytic ball along the rays of get_rays (ray parameter of the first intersection), fp64
    _, _, o = ref.camera64(s["K"], s["c2w"])
    i, j = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="xy")
    d = ref.rays64(i, j, s["K"], s["c2w"])
    oc = o - np.asarray(BALL["centre"], np.float64)
    qa, qb, qc = (d * d).sum(-1), (d * oc).sum(-1), (oc * oc).sum() - BALL["radius"] ** 2
    disc = qb * qb - qa * qc
    hit = disc >= 0
    depth_vol = np.where(hit, (-qb - np.sqrt(np.where(hit, disc, 0))) / qa, 0.0).astype(np.float32)
    acc = hit.astype(np.float32)
    out = mesh.rasterize(verts, faces, H, W, s["K"], s["c2w"])
    got = mesh.depth_agreement(out["depth"], out["mask"], dev(depth_vol), dev(acc), 0.5)
    same = mesh.depth_agreement(dev(want["depth"]), dev(want["face"] >= 0), dev(depth_vol), dev(acc), 0.5)
    print(got)
    assert got == same
    both = (want["face"] >= 0) & hit
    delta = np.abs(want["depth"].astype(np.float64) - depth_vol.astype(np.float64))[both]
    union = ((want["face"] >= 0) | hit).sum()
    assert got["n_mesh"] == (want["face"] >= 0).sum() and got["n_vol"] == hit.sum() and got["n_both"] == both.sum() > 150
    assert got["iou"] == both.sum() / union
    assert got["median_abs"] == pytest.approx(np.quantile(delta, 0.5), rel=1e-12) and got["p95_abs"] == pytest.approx(np.quantile(delta, 0.95), rel=1e-12)
    empty = mesh.depth_agreement(out["depth"], torch.zeros_like(out["mask"]), dev(depth_vol), dev(np.zeros_like(acc)), 0.5)
    assert empty["iou"] == 1.0 and empty["n_both"] == 0 and np.isnan(empty["median_abs"])

"""Depth-map fusion on the GPU (``mofa_tsdf_integrate`` / ``mofa_tsdf_field``, ``mesh.tsdf_*``, ``Renderer.fuse_geometry``) against the NumPy
restatement (tests/fuse_reference.py; tests/test_fuse_reference_cpu.py shows what the comparison catches):

* ``tsdf_integrate`` is the restatement's state bit for bit (``acc``, ``wsum``) and integer for integer (``front``, ``behind``) on the whole
  catalogue; views in batches of 1, 3 and all give the same bytes, also on another stream;
* ``tsdf_field`` is the restatement's for every ``unobserved`` x ``close_border``, counters included, and ``tsdf_surface`` is
  ``mesh.iso_surface`` of the restated field bit for bit; the sphere's mesh is closed;
* end to end through the project's own tools — a UV sphere cast by ``mesh.ray_cast`` from the sphere scene's poses, encoded by
  ``depth_frame``, fused and marched — every vertex lies within one grid step plus the polyhedron's sagitta of the sphere;
* ``Renderer.fuse_geometry`` equals streaming ``tsdf_integrate`` over the same ``render_geometry`` frames and the restatement on them;
* bad input raises ``MofaError``.
"""
import numpy as np
import pytest
import torch

import fuse_reference as fr
import raster_reference as rast
from harness import make_product
from mofanerf_amd import lib, mesh, rays, synth
from mofanerf_amd.rays import pose_spherical

pytestmark = pytest.mark.gpu
DEV = "cuda"
CATALOGUE = fr.catalogue()
NAMES = [c["name"] for c in CATALOGUE]
WANT = {c["name"]: fr.fuse(c) for c in CATALOGUE}                 # the restated states: computed once, never modified
KEYS = ("acc", "wsum", "front", "behind")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def case_of(name):
    (c,) = [c for c in CATALOGUE if c["name"] == name]
    return c


def cameras(c, sl=slice(None)):
    """(K, c2w) of a catalogue entry's views ``sl``: one camera, or one per view."""
    cams = c["cams"] if len(c["cams"]) == 1 else c["cams"][sl]
    K = np.zeros((len(cams), 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cams[:, 0], cams[:, 1], cams[:, 2], cams[:, 3], 1
    pose = cams[:, 4:].reshape(-1, 3, 4)
    return (K[0], pose[0]) if len(cams) == 1 else (K, pose)


def gpu_fuse(c, batch=None):
    state = mesh.tsdf_volume(c["res"], c["lo"], c["step"], c["trunc"], DEV)
    n = len(c["depth"])
    batch = n if batch is None else batch
    for first in range(0, n, batch):
        sl = slice(first, min(first + batch, n))
        weight = None if c["weight"] is None else dev(c["weight"][sl])
        depth = dev(c["depth"][sl])
        out = mesh.tsdf_integrate(state, depth[0] if depth.shape[0] == 1 and first % 2 else depth, *cameras(c, sl),
                                  weight=None if weight is None else weight.reshape(depth.shape), carve=c["carve"])
        assert out is state
    assert state["frames"] == n
    return state


def host_state(state):
    return {k: state[k].cpu().numpy() for k in KEYS}


def differing(got, want):
    return [k for k in KEYS if not fr.same_bits(got[k], want[k])]


@pytest.mark.parametrize("name", NAMES)
def test_integrate_equals_the_restatement(name):
    c = case_of(name)
    got = host_state(gpu_fuse(c))
    assert differing(got, WANT[name]) == [], (name, [(k, int((got[k] != WANT[name][k]).sum())) for k in KEYS])
    assert (got["front"] > 0).any()


@pytest.mark.parametrize("name", NAMES)
def test_batches_and_another_stream_give_the_same_bytes(name):
    c = case_of(name)
    for batch in (1, 3):
        assert differing(host_state(gpu_fuse(c, batch)), WANT[name]) == [], (name, batch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = gpu_fuse(c, 3)
    side.synchronize()
    assert differing(host_state(other), WANT[name]) == [], name


@pytest.mark.parametrize("name", NAMES)
def test_field_and_surface_equal_the_restatement(name):
    c = case_of(name)
    state = gpu_fuse(c)
    n = int(np.prod(c["res"]))
    for unobserved in fr.UNOBSERVED:
        for close_border in (False, True):
            want, counts = fr.field(WANT[name], c["res"], unobserved, close_border)
            got, stats = mesh.tsdf_field(state, unobserved, close_border)
            assert got.shape == tuple(c["res"]) and got.dtype == torch.float32
            assert fr.same_bits(got.cpu().numpy(), want), (name, unobserved, close_border)
            assert {k: stats[k] for k in fr.COUNTS} == counts and stats["voxels"] == n and stats["frames"] == len(c["depth"])
            verts, faces = mesh.tsdf_surface(state, unobserved, close_border)
            v_ref, f_ref = mesh.iso_surface(dev(want), 0.0, c["lo"], c["step"])
            assert torch.equal(faces, f_ref) and fr.same_bits(verts.cpu().numpy(), v_ref.cpu().numpy()), (name, unobserved, close_border)


def test_the_sphere_mesh_is_closed_and_within_a_step():
    c = case_of("sphere")
    verts, faces = mesh.tsdf_surface(gpu_fuse(c))
    assert verts.shape[0] > 5000 and faces.shape[0] > 10000
    centre = dev(np.asarray([fr.SPHERE_C, (3.0, 3.0, 3.0)], np.float32))
    w = mesh.winding_number(centre, verts, faces, require_closed=True)               # raises if an edge is open
    assert w["winding"].cpu().tolist() == [1, 0]                                     # the normals point outward
    err = fr.sphere_error(verts.cpu().numpy(), c["step"])
    print(f"sphere (analytic depth): max {err.max():.4f} median {np.median(err):.4f} steps over {len(err)} vertices")
    assert err.max() <= 1.0
    for post in (mesh.components(verts, faces)["n_components"], mesh.smooth(verts, faces, iterations=2)[0].shape[0]):
        assert post >= 1


def test_end_to_end_through_ray_cast_and_depth_frame():
    """A UV sphere (64 x 64, R = 1) cast by mesh.ray_cast from the sphere scene's eight poses, encoded by depth_frame, fused and marched.
    CONDITION: | |v - c| - R | <= one grid step + the polyhedron's sagitta R (1 - cos(pi / 64)) for every vertex."""
    c = case_of("sphere")
    v_np, f_np = rast.uv_sphere(64, 64, radius=fr.SPHERE_R, centre=fr.SPHERE_C)
    v, f = dev(v_np), dev(f_np)
    H, W = fr.SPHERE_H, fr.SPHERE_W
    K = fr.sphere_camera()
    state = mesh.tsdf_volume(c["res"], c["lo"], c["step"], c["trunc"], DEV)
    shares = []
    for pose in fr.sphere_poses():
        o, d = rays.get_rays(H, W, K, pose, DEV)
        cast = mesh.ray_cast(o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), v, f)
        frame = mesh.depth_frame(cast["t"].reshape(H, W), cast["hit"].reshape(H, W), "empty")
        assert bool(torch.isposinf(frame[~cast["hit"].reshape(H, W)]).all())
        shares.append(float(cast["hit"].float().mean()))
        mesh.tsdf_integrate(state, frame, K, pose)
    assert 0.1 < min(shares) and max(shares) < 0.9
    verts, faces = mesh.tsdf_surface(state)
    step = float(np.max(c["step"]))
    r = np.linalg.norm(verts.cpu().numpy().astype(np.float64) - np.asarray(fr.SPHERE_C), axis=1)
    bound = step + fr.SPHERE_R * (1 - np.cos(np.pi / 64))
    print(f"end to end: max | |v - c| - R | = {np.abs(r - fr.SPHERE_R).max():.5f} (bound {bound:.5f}, step {step:.5f}) over {len(r)} vertices")
    assert len(r) > 5000 and np.abs(r - fr.SPHERE_R).max() <= bound
    mesh.winding_number(dev(np.asarray([fr.SPHERE_C], np.float32)), verts, faces, require_closed=True)


def test_renderer_fuse_geometry_streams_the_frames_it_renders():
    render, kw, _ = make_product((8, 64, 8, 64), 0, 4096, DEV)
    H, W = 6, 9
    K = synth.intrinsics(H, W)
    poses = [pose_spherical(az, el, 16.0)[:3, :4] for az, el in ((-30.0, 10.0), (0.0, -5.0), (40.0, 20.0))]
    bm, _, exp = (x.to(DEV) for x in synth.codes(0))
    bounds, res, trunc = ((-3.0, -3.0, -3.0), (3.0, 3.5, 4.0)), (9, 9, 9), 1.25
    for surface, weight, background in (("median", None, "empty"), ("expected", "acc", "unknown")):
        verts, faces, stats = render.fuse_geometry(poses, H, W, K, bounds=bounds, resolution=res, trunc=trunc, shapeCodes=bm, expType=20,
                                                   expCodes=exp, surface=surface, weight=weight, background=background, acc_min=0.5, **kw)
        fused = host_state(render.fuse_state)
        _, lo, step = mesh.grid_spec(bounds, res)
        state = mesh.tsdf_volume(res, lo, step, trunc, DEV)
        want = fr.new_state(res)
        for pose in poses:
            depth, _, acc, ex = render.render_geometry(H, W, K, c2w=pose, shapeCodes=bm, expType=20, expCodes=exp, median=True, **dict(kw, ndc=False))
            d = (ex["depth_median"] if surface == "median" else depth).reshape(H, W)
            mask = acc.reshape(H, W) >= 0.5
            frame = mesh.depth_frame(d, mask, background)
            wmap = torch.clamp(torch.where(mask, acc.reshape(H, W), 1.0 - acc.reshape(H, W)), min=0.0) if weight else None
            mesh.tsdf_integrate(state, frame, K, pose, weight=wmap)
            assert fr.same_bits(frame.cpu().numpy(), fr.depth_frame(d.cpu().numpy(), mask.cpu().numpy(), background))
            fr.integrate(want, res, lo, step, trunc, frame.cpu().numpy()[None], fr.cam_table(K, pose.numpy()),
                         None if wmap is None else wmap.cpu().numpy()[None])
        render.check_launches(block=True)
        assert differing(fused, host_state(state)) == [] and differing(fused, want) == [], (surface, weight)
        v_ref, f_ref = mesh.tsdf_surface(state)
        assert torch.equal(faces, f_ref) and fr.same_bits(verts.cpu().numpy(), v_ref.cpu().numpy())
        fld, counts = fr.field(want, res)
        assert {k: stats[k] for k in fr.COUNTS} == counts and stats["frames"] == 3 and stats["trunc"] == trunc and stats["resolution"] == res
        assert len(stats["hit_share"]) == 3 and all(0.0 <= s <= 1.0 for s in stats["hit_share"])
        assert set(stats["times"]) == {"render", "integrate", "march"} and all(t >= 0 for t in stats["times"].values())
    with pytest.raises(lib.MofaError, match="ndc"):
        render.fuse_geometry(poses, H, W, K, bounds=bounds, resolution=res, trunc=trunc, shapeCodes=bm, expCodes=exp, **dict(kw, ndc=True))
    for bad in (dict(trunc=0.0), dict(trunc=float("inf")), dict(surface="mean"), dict(weight="depth"), dict(background="white"),
                dict(unobserved="maybe")):
        with pytest.raises(lib.MofaError, match="fuse_geometry"):
            render.fuse_geometry(poses, H, W, K, **dict(dict(bounds=bounds, resolution=res, trunc=trunc, shapeCodes=bm, expCodes=exp, **kw), **bad))


def test_refusals():
    c = case_of("non_cubic")
    K, pose = cameras(c)
    depth = dev(c["depth"])
    for trunc in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(lib.MofaError, match="trunc"):
            mesh.tsdf_volume(c["res"], c["lo"], c["step"], trunc, DEV)
    for res in ((2048, 2048, 512), (1, 8, 8)):                                       # past the limit: refused before anything is allocated
        with pytest.raises(lib.MofaError, match="refused"):
            mesh.tsdf_volume(res, c["lo"], c["step"], 0.2, DEV)
    state = mesh.tsdf_volume(c["res"], c["lo"], c["step"], c["trunc"], DEV)
    mesh.tsdf_integrate(state, depth, K, pose, trunc=c["trunc"])                     # the volume's own trunc is accepted
    before = host_state(state)
    with pytest.raises(lib.MofaError, match="fixed for the life"):
        mesh.tsdf_integrate(state, depth, K, pose, trunc=2 * c["trunc"])
    for w in (-1.0, float("nan"), float("inf")):
        weight = torch.ones_like(depth)
        weight[1, 2, 3] = w
        with pytest.raises(lib.MofaError, match="weight"):
            mesh.tsdf_integrate(state, depth, K, pose, weight=weight)
    for bad, match in (((depth, K[:2], pose), "frames"), ((depth, K, pose[:2]), "frames"), ((depth[:2], K, pose), "frames"),
                       ((depth.cpu(), K, pose), "GPU"), ((depth.double(), K, pose), "float32"), ((depth[0, 0], K[0], pose[0]), "depth"),
                       ((depth, K[:, :1], pose), "K")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.tsdf_integrate(state, *bad)
    with pytest.raises(lib.MofaError, match="weight"):
        mesh.tsdf_integrate(state, depth, K, pose, weight=torch.ones_like(depth)[:, :5].contiguous())
    with pytest.raises(lib.MofaError, match="GPU"):                                  # state and frames on different devices
        mesh.tsdf_integrate(state, depth, K, pose, weight=torch.ones_like(depth).cpu())
    cpu_state = dict(state, acc=state["acc"].cpu())
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.tsdf_integrate(cpu_state, depth, K, pose)
    with pytest.raises(lib.MofaError, match="unobserved"):
        mesh.tsdf_field(state, "maybe")
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.depth_frame(depth.cpu(), depth.cpu() > 0)
    with pytest.raises(lib.MofaError, match="mask"):
        mesh.depth_frame(depth, (depth > 0)[:1])
    with pytest.raises(lib.MofaError, match="background"):
        mesh.depth_frame(depth, depth > 0, "white")
    assert differing(host_state(state), before) == []                                # a refused call leaves the volume as it was

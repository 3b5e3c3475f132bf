"""Multi-view colour baking on the GPU (``mofa_bake_integrate`` / ``mofa_bake_resolve`` / ``mofa_bake_fill``, ``mesh.bake_*`` /
``fill_colors``, ``Renderer.bake_mesh``) against the NumPy restatement (tests/bake_reference.py; tests/test_bake_reference_cpu.py shows
what the comparison catches):

* the state after ``bake_integrate`` is the restatement's bit for bit (``csum``, ``wsum``, ``wbest``, ``cbest``) and integer for integer
  (``seen``, ``occluded``, ``grazing``) on the whole catalogue, and ``bake_colors`` gives its colours, validity and counts for both blends;
* views streamed in several calls, a second run and another stream give the same bytes;
* ``fill_colors`` is the restatement's for 0, 1 and 5 iterations;
* end to end through the GPU's own ``mesh.rasterize(attrs=...)`` on the sphere: every vertex coloured, within the bound of DESIGN.md 3.26;
* ``Renderer.bake_mesh`` equals the hand-made sequence ``render_fitting`` -> ``rasterize`` -> ``depth_frame`` -> ``bake_integrate`` ->
  ``bake_colors`` bit for bit, and refuses ``ndc=True``;
* the three entry points and the four ``mesh`` calls refuse bad arguments.
"""
import numpy as np
import pytest
import torch

import bake_reference as br
from harness import make_product
from mofanerf_amd import lib, mesh, synth
from mofanerf_amd.rays import pose_spherical

pytestmark = pytest.mark.gpu
DEV = "cuda"
CATALOGUE = br.catalogue()
NAMES = [c["name"] for c in CATALOGUE]
WANT = {c["name"]: br.bake(c) for c in CATALOGUE}                 # the restated states: computed once, never modified
FILL = br.fill_cases()


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


def gpu_bake(c, batch=None):
    V, C = len(c["verts"]), c["images"].shape[-1]
    state = mesh.bake_state(V, C, DEV)
    verts, normals = dev(c["verts"]), None if c["normals"] is None else dev(c["normals"])
    n = len(c["depth"])
    batch = n if batch is None else batch
    for first in range(0, n, batch):
        sl = slice(first, min(first + batch, n))
        images, depth = dev(c["images"][sl]), dev(c["depth"][sl])
        single = images.shape[0] == 1 and first % 2 == 0                      # a lone frame also goes in without its leading axis
        out = mesh.bake_integrate(state, verts, images[0] if single else images, depth[0] if single else depth, *cameras(c, sl), normals,
                                  depth_tol=c["depth_tol"], cos_min=c["cos_min"], power=c["power"])
        assert out is state
    assert state["frames"] == n
    return state


def host_state(state):
    return {k: state[k].cpu().numpy() for k in br.STATE_KEYS}


def differing(got, want):
    return [k for k in br.STATE_KEYS if not br.same_bits(got[k], want[k])]


@pytest.mark.parametrize("name", NAMES)
def test_integrate_and_colors_equal_the_restatement(name):
    c = case_of(name)
    state = gpu_bake(c)
    got = host_state(state)
    assert differing(got, WANT[name]) == [], (name, [(k, int((got[k] != WANT[name][k]).sum())) for k in br.STATE_KEYS])
    assert (got["seen"] > 0).any()
    for blend, fill in (("mean", 0.0), ("best", -2.5)):
        want = br.resolve(WANT[name], blend, fill)
        out = mesh.bake_colors(state, blend, fill)
        assert out["colors"].dtype == torch.float32 and out["valid"].dtype == torch.bool and out["seen"] is state["seen"]
        assert br.same_bits(out["colors"].cpu().numpy(), want["colors"]) and np.array_equal(out["valid"].cpu().numpy(), want["valid"]), (name, blend)
        assert {k: out["counts"][k] for k in br.COUNTS} == want["counts"], (name, blend)
        assert out["counts"]["vertices"] == len(c["verts"]) == sum(want["counts"].values()) and out["counts"]["frames"] == len(c["depth"])


@pytest.mark.parametrize("name", NAMES)
def test_streaming_a_second_run_and_another_stream_give_the_same_bytes(name):
    c = case_of(name)
    n = len(c["depth"])
    for batch in sorted({1, 2, n}):                                           # 3 views: 1 + 1 + 1, 2 + 1 and 3 + 0
        assert differing(host_state(gpu_bake(c, batch)), WANT[name]) == [], (name, batch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = gpu_bake(c, 2)
    side.synchronize()
    assert differing(host_state(other), WANT[name]) == [], name


@pytest.mark.parametrize("case", FILL, ids=[f["name"] for f in FILL])
def test_fill_colors_equals_the_restatement(case):
    colors, valid, faces = dev(case["colors"]), dev(case["valid"]), dev(case["faces"])
    for iterations in (0, 1, 5):
        want_c, want_v, want_left = br.fill_colors(case["colors"], case["valid"], case["faces"], iterations)
        for _ in range(2):                                                    # and again: the same bytes
            got_c, got_v, left = mesh.fill_colors(colors, valid, faces, iterations)
            assert br.same_bits(got_c.cpu().numpy(), want_c) and np.array_equal(got_v.cpu().numpy(), want_v) and left == want_left, \
                (case["name"], iterations)
        assert got_c.data_ptr() != colors.data_ptr() and br.same_bits(colors.cpu().numpy(), case["colors"])     # the input is left alone
    if case["name"] == "island":
        assert mesh.fill_colors(colors, valid, faces, 50)[2] == case["n_island"]


def test_end_to_end_through_the_gpu_rasteriser_on_the_sphere():
    """The sphere's ten frames rasterised by ``mesh.rasterize(attrs=A x + b)`` on the GPU, its normals from ``mesh.vertex_normals``.
    CONDITIONS: every vertex is coloured, and | colour - (A x + b) | <= the bound of DESIGN.md 3.26 (the one of the CPU test)."""
    s = br.SPHERE
    v_np, f_np, _ = br.sphere_mesh()
    verts, faces = dev(v_np), dev(f_np)
    K, poses = br.sphere_camera(), br.sphere_poses()
    attrs = dev(br.sphere_field(v_np))
    normals = (-mesh.vertex_normals(verts, faces)).contiguous()               # (uv_sphere winds its faces with the normals inward)
    assert bool(((normals * (verts - dev(np.asarray(s["centre"], np.float32)))).sum(-1) > 0).all())
    state = mesh.bake_state(len(v_np), 3, DEV)
    for pose in poses:
        r = mesh.rasterize(verts, faces, s["H"], s["W"], K, pose, attrs=attrs)
        mesh.bake_integrate(state, verts, r["attr"], mesh.depth_frame(r["depth"], r["mask"]), K, pose, normals, depth_tol=s["depth_tol"],
                            cos_min=s["cos_min"], power=s["power"])
    bound, parts = br.sphere_bound(v_np, f_np, normals.cpu().numpy(), br.cam_table(K, poses, len(poses)), s["depth_tol"], s["cos_min"], s["H"], s["W"])
    want = br.sphere_field(v_np).astype(np.float64)
    for blend in ("mean", "best"):
        out = mesh.bake_colors(state, blend)
        assert bool(out["valid"].all()) and out["counts"]["colored"] == len(v_np), (blend, out["counts"])
        err = np.linalg.norm(out["colors"].cpu().numpy().astype(np.float64) - want, axis=1)
        print(f"sphere end to end, {blend}: max |colour - (A x + b)| = {err.max():.5f}, bound {bound:.5f} (slack {parts['slack']:.3f})")
        assert err.max() <= bound, (blend, err.max(), bound)


def test_renderer_bake_mesh_is_the_hand_made_sequence():
    render, kw, _ = make_product((8, 64, 8, 64), 0, 4096, DEV)
    H = W = 16
    K = synth.intrinsics(H, W)
    poses = [pose_spherical(az, el, 16.0)[:3, :4] for az, el in ((-30.0, 10.0), (0.0, -5.0), (40.0, 20.0))]
    bm, tex, exp = (x.to(DEV) for x in synth.codes(0))
    bounds, res = ((-3.0, -3.0, -3.0), (3.0, 3.5, 4.0)), (9, 9, 9)
    net = kw["network_fine"]
    level = float(render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm, expCodes=exp).median())
    verts, faces = (t.contiguous() for t in render.extract_mesh(net, bounds=bounds, resolution=res, level=level, shapeCodes=bm, expCodes=exp))
    assert verts.shape[0] > 50
    normals = mesh.vertex_normals(verts, faces).contiguous()                  # (a float index_add_ with no fixed order: computed ONCE)
    rk = {k: v for k, v in kw.items() if k != "ndc"}
    codes = dict(shapeCodes=bm, uvCodes=tex, expCodes=exp, expType=20)
    for blend, cos_min, power in (("mean", 0.0, 2), ("best", 0.2, 1)):
        colors, valid, stats = render.bake_mesh(poses, H, W, K, verts, faces, depth_tol=0.5, blend=blend, cos_min=cos_min, power=power,
                                                normals=normals, **codes, **rk)
        state = mesh.bake_state(verts.shape[0], 3, DEV)
        for pose in poses:
            with torch.no_grad():                                              # bake_mesh renders for inference: nothing is taped
                rgb = render.render_fitting(H, W, K, c2w=pose, **codes, **dict(rk, ndc=False))[0]
            r = mesh.rasterize(verts, faces, H, W, K, pose)
            mesh.bake_integrate(state, verts, rgb.reshape(H, W, 3).contiguous(), mesh.depth_frame(r["depth"], r["mask"]), K, pose, normals,
                                depth_tol=0.5, cos_min=cos_min, power=power)
        render.check_launches(block=True)
        got, hand = host_state(render.bake_state), host_state(state)
        assert differing(got, hand) == [], (blend, float(np.abs(got["csum"] - hand["csum"]).max()))
        want = mesh.bake_colors(state, blend)
        assert br.same_bits(colors.cpu().numpy(), want["colors"].cpu().numpy()) and torch.equal(valid, want["valid"])
        assert {k: stats[k] for k in br.COUNTS} == {k: want["counts"][k] for k in br.COUNTS} and stats["frames"] == 3
        assert stats["colored"] > 0 and stats["remaining"] == verts.shape[0] - stats["colored"] and render.bake_stats is stats
        assert len(stats["hit_share"]) == 3 and all(0.0 < s <= 1.0 for s in stats["hit_share"])
        assert set(stats["times"]) == {"render", "rasterize", "integrate", "resolve"} and all(t >= 0 for t in stats["times"].values())
        print(f"bake_mesh, {blend}: {stats['colored']} of {verts.shape[0]} vertices coloured, occluded {stats['occluded']}, grazing "
              f"{stats['grazing']}, unseen {stats['unseen']}")
    filled, filled_valid, filled_stats = render.bake_mesh(poses, H, W, K, verts, faces, depth_tol=0.5, blend="best", cos_min=0.2, power=1,
                                                          normals=normals, fill_iterations=3, **codes, **rk)
    want_c, want_v, want_left = mesh.fill_colors(colors, valid, faces, 3)
    assert br.same_bits(filled.cpu().numpy(), want_c.cpu().numpy()) and torch.equal(filled_valid, want_v) and filled_stats["remaining"] == want_left
    default, default_valid, _ = render.bake_mesh(poses, H, W, K, verts, faces, depth_tol=0.5, blend="best", cos_min=0.2, power=1, **codes, **rk)
    assert default.shape == colors.shape and default_valid.shape == valid.shape          # its own vertex_normals: no bits are promised
    with pytest.raises(lib.MofaError, match="ndc"):
        render.bake_mesh(poses, H, W, K, verts, faces, depth_tol=0.5, **codes, **dict(rk, ndc=True))
    for bad, match in ((dict(depth_tol=-1.0), "depth_tol"), (dict(blend="median"), "blend"), (dict(cos_min=1.0), "cos_min"), (dict(power=9), "power"),
                       (dict(fill_iterations=-1), "fill_iterations")):
        with pytest.raises(lib.MofaError, match=match):
            render.bake_mesh(poses, H, W, K, verts, faces, **dict(dict(depth_tol=0.5, **codes, **rk), **bad))
    with pytest.raises(lib.MofaError, match="no poses"):
        render.bake_mesh([], H, W, K, verts, faces, depth_tol=0.5, **codes, **rk)


def test_the_entry_points_refuse_bad_arguments():
    L = lib.load()
    V, C, H, W, n = 8, 3, 4, 5, 2
    f = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
    verts, images, depth, cams = f(V, 3), f(n, H, W, C), f(n, H, W), f(n, 16)
    st = mesh.bake_state(V, C, DEV)
    sp = [st[k].data_ptr() for k in br.STATE_KEYS]
    call = lambda verts=verts.data_ptr(), V=V, H=H, W=W, C=C, n=n, n_cams=n, tol=0.1, cos_min=0.0, power=2, last=sp[-1]: L.mofa_bake_integrate(
        verts, None, V, images.data_ptr(), depth.data_ptr(), n, H, W, C, cams.data_ptr(), n_cams, tol, cos_min, power, *sp[:-1], last, lib.stream())
    assert call() == 0                                                         # the arguments below differ from a call that is accepted
    for kw in (dict(verts=None), dict(last=None), dict(V=0), dict(C=0), dict(C=17), dict(H=1), dict(W=1), dict(H=65536, W=32768), dict(n=0),
               dict(n_cams=3), dict(tol=-0.1), dict(tol=float("nan")), dict(tol=float("inf")), dict(cos_min=1.0), dict(cos_min=-0.1),
               dict(cos_min=float("nan")), dict(power=-1), dict(power=9)):
        assert call(**kw) != 0 and L.mofa_last_error(), kw
    colors, valid, ws, counts = f(V, C), f(V, dtype=torch.uint8), f(64, dtype=torch.uint8), f(4, dtype=torch.int64)
    resolve = lambda V=V, C=C, blend=0, counts=counts.data_ptr(): L.mofa_bake_resolve(
        V, C, sp[0], sp[1], sp[3], sp[4], sp[5], sp[6], blend, 0.0, colors.data_ptr(), valid.data_ptr(), ws.data_ptr(), counts, lib.stream())
    assert resolve() == 0
    for kw in (dict(V=0), dict(C=0), dict(C=17), dict(blend=2), dict(blend=-1), dict(counts=None)):
        assert resolve(**kw) != 0 and L.mofa_last_error(), kw
    offsets, nbr = f(V + 1, dtype=torch.int64), f(4, dtype=torch.int32)
    out_c, out_v = f(V, C), f(V, dtype=torch.uint8)
    fill = lambda V=V, C=C, E=0, out=out_c.data_ptr(), vout=out_v.data_ptr(), offsets=offsets.data_ptr(): L.mofa_bake_fill(
        colors.data_ptr(), valid.data_ptr(), V, C, offsets, nbr.data_ptr(), E, out, vout, lib.stream())
    assert fill() == 0
    for kw in (dict(V=0), dict(C=0), dict(C=17), dict(E=-1), dict(E=2 ** 31), dict(out=colors.data_ptr()), dict(vout=valid.data_ptr()),
               dict(offsets=None)):
        assert fill(**kw) != 0 and L.mofa_last_error(), kw
    torch.cuda.synchronize()


def test_the_mesh_calls_refuse_bad_arguments():
    c = case_of("cams_per_view")
    K, pose = cameras(c)
    verts, normals, images, depth = dev(c["verts"]), dev(c["normals"]), dev(c["images"]), dev(c["depth"])
    V = len(c["verts"])
    state = mesh.bake_state(V, 3, DEV)
    mesh.bake_integrate(state, verts, images, depth, K, pose, normals, depth_tol=0.2)
    before = host_state(state)
    for args, kw, match in (((verts[:5], images, depth, K, pose), {}, "verts"), ((verts, images, depth, K, pose, normals[:5]), {}, "normals"),
                            ((verts.double(), images, depth, K, pose), {}, "float32"), ((verts, images[..., :2], depth, K, pose), {}, "contiguous"),
                            ((verts, images[..., :2].contiguous(), depth, K, pose), {}, "images"), ((verts, images, depth[:2], K, pose), {}, "images"),
                            ((verts, images.cpu(), depth, K, pose), {}, "GPU"), ((verts, images, depth, K[:2], pose), {}, "frames"),
                            ((verts, images, depth, K, pose[:2]), {}, "frames"), ((verts, images[:, :1].contiguous(), depth[:, :1].contiguous(), K, pose), {}, "refused"),
                            ((verts, images, depth, K, pose), dict(depth_tol=-1.0), "depth_tol"),
                            ((verts, images, depth, K, pose), dict(cos_min=1.5), "cos_min"), ((verts, images, depth, K, pose), dict(power=9), "power")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.bake_integrate(state, *args, **dict(dict(depth_tol=0.2), **kw))
    with pytest.raises(lib.MofaError, match="channels"):
        mesh.bake_integrate(dict(state, channels=17), verts, images, depth, K, pose, depth_tol=0.2)
    with pytest.raises(lib.MofaError, match="csum"):
        mesh.bake_integrate(dict(state, csum=state["csum"][:5]), verts, images, depth, K, pose, depth_tol=0.2)
    with pytest.raises(lib.MofaError, match="blend"):
        mesh.bake_colors(state, "median")
    with pytest.raises(lib.MofaError, match="fill"):
        mesh.bake_colors(state, "mean", fill="red")
    assert differing(host_state(state), before) == []                          # a refused call leaves the state as it was
    empty = mesh.bake_colors(mesh.bake_state(0, 3, DEV))
    assert empty["colors"].shape == (0, 3) and empty["counts"]["colored"] == 0 and empty["counts"]["vertices"] == 0
    colors, valid, faces = dev(FILL[1]["colors"]), dev(FILL[1]["valid"]), dev(FILL[1]["faces"])
    bad_faces = faces.clone()
    bad_faces[3, 1] = len(colors)
    with pytest.raises(lib.MofaError, match="outside"):                        # before any step runs
        mesh.fill_colors(colors, valid, bad_faces, 1)
    for args, match in (((colors, valid, faces, -1), "iterations"), ((colors, valid, faces, 1.5), "iterations"), ((colors, valid[:5], faces, 1), "valid"),
                        ((colors, valid.to(torch.uint8), faces, 1), "valid"), ((colors[:, :0], valid, faces, 1), "colors"),
                        ((colors, valid, faces.cpu(), 1), "GPU"), ((colors.double(), valid, faces, 1), "float32")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.fill_colors(*args)

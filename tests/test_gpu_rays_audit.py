"""Ray generation and the camera-pose gradient on anisotropic, non-square, off-centre cameras with generic poses, against the NumPy
restatement of tests/rays_reference.py (held to the oracle, fp64 and autograd by tests/test_rays_reference_cpu.py, which also shows that
every fault of ``rays_reference.FAULTS`` breaks these comparisons and that the old square camera could not see seven of them).

``mofa_get_rays`` / ``mofa_get_rays_at`` / the layer-0 camera mode are compared BIT FOR BIT (origins, directions, view directions: every
step is one correctly rounded fp32 operation); ``mofa_rays_pose_backward`` within ``rays_reference.pose_grad_bound`` of the exact sums
(one fp32 rounding + the reordering of an n-term fp64 sum), and exactly where a single term is summed.  Outputs sit between NaN-filled guard
rows and start as NaN."""
import numpy as np
import pytest
import torch

import bwd_reference as br
import rays_reference as rr
from harness import make_product
from mofanerf_amd import lib, mesh, rays, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
EINVAL = -1


def L():
    return lib.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Out:
    """[n,3] float32 between GUARD rows on either side, all of it NaN until a kernel writes."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full(((n + 2 * GUARD) * 3,), float("nan"), device=DEV)
        self.out = self.buf[GUARD * 3:(GUARD + n) * 3]

    def ptr(self):
        return self.out.data_ptr()

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:GUARD * 3]).all()) and bool(torch.isnan(self.buf[(GUARD + self.n) * 3:]).all())

    def untouched(self):
        return self.guards_intact() and bool(torch.isnan(self.out).all())

    def numpy(self):
        assert self.guards_intact(), "a guard row was written"
        return self.out.reshape(self.n, 3).cpu().numpy()


def intr(cam):
    return float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"])


def gpu_rays(cam, pix0=0, n=0, pixels=None, view=True):
    """(rays_o, rays_d, viewdirs or None) as numpy through the C ABI: the contiguous range [pix0, pix0 + n) or the int32 list ``pixels``."""
    n = n if pixels is None else len(pixels)
    o, d, v = Out(n), Out(n), Out(n)
    pose = dev(cam["c2w"])
    if pixels is None:
        rc = L().mofa_get_rays(cam["H"], cam["W"], *intr(cam), lib.ptr(pose), int(pix0), n, o.ptr(), d.ptr(), v.ptr() if view else None, lib.stream())
    else:
        pl = dev(np.asarray(pixels, np.int32))
        rc = L().mofa_get_rays_at(cam["H"], cam["W"], *intr(cam), lib.ptr(pose), pl.data_ptr(), n, o.ptr(), d.ptr(), v.ptr() if view else None,
                                  lib.stream())
    lib.check(rc, "get_rays")
    torch.cuda.synchronize()
    assert view or v.untouched(), "viewdirs = NULL, yet something was written"
    return o.numpy(), d.numpy(), v.numpy() if view else None


def want_rays(cam, pix):
    return rr.rays(cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["c2w"], pix)


def assert_rays(cam, what, pix0=0, n=0, pixels=None):
    pix = np.asarray(pixels, np.int64) if pixels is not None else pix0 + np.arange(n, dtype=np.int64)
    want = want_rays(cam, pix)
    got = gpu_rays(cam, pix0, n, pixels)
    for name, g, w in zip(("rays_o", "rays_d", "viewdirs"), got, want):
        diff = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert len(diff) == 0, (what, name, len(diff), [(int(pix[r]), int(c), float(g[r, c]), float(w[r, c])) for r, c in diff[:4]])
    bare = gpu_rays(cam, pix0, n, pixels, view=False)
    assert rr.same_bits(bare[0], want[0]) and rr.same_bits(bare[1], want[1]), (what, "viewdirs = NULL")


# ---- 1. frames, ranges and lists ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.SMALL)
def test_frames_ranges_and_lists_are_the_restatement_bit_for_bit(name):
    cam = rr.CAMERAS[name]
    H, W = cam["H"], cam["W"]
    P = H * W
    assert_rays(cam, "frame", 0, P)
    mid = max(W - 3, 1)                                                            # mid-row wherever a row has more than one pixel
    assert_rays(cam, "three rows", mid, min(2 * W + 5, P - mid))
    assert_rays(cam, "one pixel", mid, 1)
    assert_rays(cam, "last pixel", P - 1, 1)
    rng = np.random.default_rng(W)
    some = rng.integers(0, P, 400)
    assert_rays(cam, "list", pixels=rng.permutation(np.concatenate([some, some[:77], [0, P - 1, P - 1]])))


def test_huge_images_index_in_64_bits():
    """46340 x 46340 through the int32 list (values just under 2^31) and 65536 x 65537 through contiguous ranges across 2^32 and up to the
    frame's last pixel: only n rays are allocated."""
    assert_rays(rr.CAMERAS["huge_list"], "huge list", pixels=rr.huge_list_pixels())
    for pix0, n in rr.HUGE_RANGES:
        assert_rays(rr.CAMERAS["huge_range"], f"huge range {pix0}", pix0, n)


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_write_nothing():
    cam = rr.CAMERAS["wide"]
    H, W, P = cam["H"], cam["W"], cam["H"] * cam["W"]
    big = rr.CAMERAS["huge_range"]
    pose, k = dev(cam["c2w"]), intr(cam)
    pl = dev(np.arange(8, dtype=np.int32))
    o, d, v = Out(8), Out(8), Out(8)
    st = lib.stream()
    cases = {
        "H = 0": lambda: L().mofa_get_rays(0, W, *k, lib.ptr(pose), 0, 8, o.ptr(), d.ptr(), v.ptr(), st),
        "H < 0": lambda: L().mofa_get_rays(-H, W, *k, lib.ptr(pose), 0, 8, o.ptr(), d.ptr(), v.ptr(), st),
        "W = 0": lambda: L().mofa_get_rays(H, 0, *k, lib.ptr(pose), 0, 8, o.ptr(), d.ptr(), v.ptr(), st),
        "n = 0": lambda: L().mofa_get_rays(H, W, *k, lib.ptr(pose), 0, 0, o.ptr(), d.ptr(), v.ptr(), st),
        "pix0 < 0": lambda: L().mofa_get_rays(H, W, *k, lib.ptr(pose), -1, 8, o.ptr(), d.ptr(), v.ptr(), st),
        "past the frame": lambda: L().mofa_get_rays(H, W, *k, lib.ptr(pose), P - 7, 8, o.ptr(), d.ptr(), v.ptr(), st),
        "past a huge frame": lambda: L().mofa_get_rays(big["H"], big["W"], *k, lib.ptr(pose), big["H"] * big["W"] - 7, 8, o.ptr(), d.ptr(), v.ptr(), st),
        "c2w NULL": lambda: L().mofa_get_rays(H, W, *k, None, 0, 8, o.ptr(), d.ptr(), v.ptr(), st),
        "rays_o NULL": lambda: L().mofa_get_rays(H, W, *k, lib.ptr(pose), 0, 8, None, d.ptr(), v.ptr(), st),
        "at: H = 0": lambda: L().mofa_get_rays_at(0, W, *k, lib.ptr(pose), pl.data_ptr(), 8, o.ptr(), d.ptr(), v.ptr(), st),
        "at: W = 0": lambda: L().mofa_get_rays_at(H, 0, *k, lib.ptr(pose), pl.data_ptr(), 8, o.ptr(), d.ptr(), v.ptr(), st),
        "at: n = 0": lambda: L().mofa_get_rays_at(H, W, *k, lib.ptr(pose), pl.data_ptr(), 0, o.ptr(), d.ptr(), v.ptr(), st),
        "at: c2w NULL": lambda: L().mofa_get_rays_at(H, W, *k, None, pl.data_ptr(), 8, o.ptr(), d.ptr(), v.ptr(), st),
        "at: rays_o NULL": lambda: L().mofa_get_rays_at(H, W, *k, lib.ptr(pose), pl.data_ptr(), 8, None, d.ptr(), v.ptr(), st),
        "at: pixels NULL": lambda: L().mofa_get_rays_at(H, W, *k, lib.ptr(pose), None, 8, o.ptr(), d.ptr(), v.ptr(), st),
        "at: 2^31 pixels": lambda: L().mofa_get_rays_at(46341, 46341, *k, lib.ptr(pose), pl.data_ptr(), 8, o.ptr(), d.ptr(), v.ptr(), st),
    }
    for what, call in cases.items():
        assert call() == EINVAL, what
        torch.cuda.synchronize()
        assert o.untouched() and d.untouched() and v.untouched(), what
    assert 46341 ** 2 >= 2 ** 31 > 46340 ** 2


# ---- 3. layer 0's camera mode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", [0, 10])
@pytest.mark.parametrize("name", ["wide", "tall", "huge_range"])
def test_layer0_camera_mode_is_layer0_on_the_restatements_rays(name, nf):
    """``mofa_layer0_forward_cam`` == ``mofa_layer0_forward`` (held to fp64 by tests/test_gpu_fwd_kernels.py) on the restatement's rays
    uploaded from the host: pixel list and contiguous range, one shared z row and a row per ray."""
    cam = rr.CAMERAS[name]
    H, W, S, Np = cam["H"], cam["W"], 5, 64
    rng = np.random.default_rng(nf + W)
    feats, kp = 3 + 6 * nf, L().mofa_pe_k_padded(nf)
    gen = torch.Generator(device=DEV).manual_seed(nf + W)
    w = torch.randn(Np, feats, generator=gen, device=DEV) / 8
    bias = torch.randn(Np, generator=gen, device=DEV)
    wp = br.pack_panels(w, Np, k_padded=kp)
    pose = dev(cam["c2w"])
    if name == "huge_range":
        forms = [(None, pix0, n) for pix0, n in rr.HUGE_RANGES] + [(rng.integers(0, 2 ** 31, 300).astype(np.int32), 0, 300)]
    else:
        forms = [(None, W - 3, 2 * W + 5), (rng.integers(0, H * W, 300).astype(np.int32), 0, 300)]
    for pixels, pix0, n in forms:
        pix = pixels.astype(np.int64) if pixels is not None else pix0 + np.arange(n, dtype=np.int64)
        ro, rd, _ = want_rays(cam, pix)
        o, d = dev(ro), dev(rd)
        pl = None if pixels is None else dev(pixels)
        for zs in (0, S):
            z = dev(np.sort(rng.uniform(2, 7, (n if zs else 1, S)).astype(np.float32), -1))
            M = n * S
            Mp = br.round_up(M, 256)
            ya, yb = (torch.full((Mp * Np,), float("nan"), device=DEV) for _ in range(2))
            lib.check(L().mofa_layer0_forward(lib.ptr(o), lib.ptr(d), lib.ptr(z), zs, None, M, S, nf, lib.ptr(wp), lib.ptr(bias), lib.ptr(ya), Mp, Np,
                                              None, lib.stream()), "layer0")
            lib.check(L().mofa_layer0_forward_cam(W, *intr(cam), lib.ptr(pose), None if pl is None else pl.data_ptr(), int(pix0), lib.ptr(z), zs, M, S,
                                                  nf, lib.ptr(wp), lib.ptr(bias), lib.ptr(yb), Mp, Np, lib.stream()), "layer0_cam")
            torch.cuda.synchronize()
            what = (name, nf, "list" if pixels is not None else pix0, zs)
            assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), what
            valid = br.unpack_panels(ya, Mp, Np)[:M]
            assert bool(torch.isfinite(valid).all()) and float(valid.abs().sum()) > 0, what


# ---- 4./5. the pose gradient -------------------------------------------------------------------------------------------------------------
def gpu_pose_grad(cam, g_o, g_d, pixels=None, pix0=0):
    """d_c2w [3,4] float32 as numpy: the list form (int32 ``pixels``) or the contiguous range from ``pix0``."""
    n = len(g_o)
    out = Out(4)
    go, gd = dev(np.asarray(g_o, np.float32)), dev(np.asarray(g_d, np.float32))
    pl = None if pixels is None else dev(np.asarray(pixels, np.int32))
    lib.check(L().mofa_rays_pose_backward(cam["W"], *intr(cam), None if pl is None else pl.data_ptr(), int(pix0), n, lib.ptr(go), lib.ptr(gd),
                                          out.ptr(), lib.stream()), "rays_pose_backward")
    torch.cuda.synchronize()
    return out.numpy().reshape(3, 4)


ONE_HOT_RAYS = (0, 63, 64, 127, 128, 255, 256, 999)


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_pose_gradient_of_one_hot_ray_gradients_is_exact(name):
    """One non-zero among the 2 x 1000 x 3 incoming gradients: the sum has one term, so d_c2w[a][b] is that fp64 product rounded once and
    every other entry exactly zero — for the first and last lane of each wavefront, the second trip of a thread's loop and the last ray."""
    cam = rr.CAMERAS[name]
    n, P = 1000, cam["H"] * cam["W"]
    pix = (5 + 7 * np.arange(n, dtype=np.int64)) % P
    dirs = np.stack(rr.camera_dirs(cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], pix), -1)
    for r in ONE_HOT_RAYS:
        for a in range(3):
            g = np.float32((-1) ** (r + a) * (1.2345678 + r / 7))
            hot, zero = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
            hot[r, a] = g
            want = np.zeros((3, 4), np.float32)
            want[a, :3] = (np.float64(g) * dirs[r].astype(np.float64)).astype(np.float32)
            got = gpu_pose_grad(cam, zero, hot, pixels=pix)
            assert np.array_equal(got, want), ("d_rays_d", r, a, got, want)
            want = np.zeros((3, 4), np.float32)
            want[a, 3] = g
            got = gpu_pose_grad(cam, hot, zero, pixels=pix)
            assert np.array_equal(got, want), ("d_rays_o", r, a, got, want)


def _grads(n, seed, spread):
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(2, n, 3))
    if spread:
        g = g * 2.0 ** rng.integers(-20, 21, size=(2, n, 3))
    return g[0].astype(np.float32), g[1].astype(np.float32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 4099])
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_pose_gradient_dense_within_the_derived_bound(name, n):
    """Random gradients, and gradients whose magnitudes spread over 2^+-20, through the list form and through the range form from a pixel
    that starts no row: within ``pose_grad_bound`` of the exact sums, and the same bytes twice."""
    cam = rr.CAMERAS[name]
    W, P = cam["W"], cam["H"] * cam["W"]
    k = (W, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    worst = 0.0
    for spread in (False, True):
        g_o, g_d = _grads(n, n + W, spread)
        listed = np.random.default_rng(n).integers(0, P, n)
        pix0 = W - 3                                                               # (the kernel takes no H: a range may run on past the frame)
        for form, pix, kw in (("list", listed, dict(pixels=listed)), ("range", pix0 + np.arange(n, dtype=np.int64), dict(pix0=pix0))):
            ref, mag = rr.pose_grad64(*k, pix, g_o, g_d)
            got = gpu_pose_grad(cam, g_o, g_d, **kw)
            assert rr.same_bits(got, gpu_pose_grad(cam, g_o, g_d, **kw)), (form, "two runs differ")
            ratio = float((np.abs(got.astype(np.float64) - ref) / rr.pose_grad_bound(ref, mag, n)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (form, spread, ratio, got, ref)
    print(f"pose gradient {name} n={n}: worst |got - ref| / bound {worst:.3f}")


def test_pose_gradient_on_a_range_past_2_to_the_32():
    """`huge_range` (65536 x 65537) through the contiguous-range form, ``pixels == NULL``: across 2^32 and up to the frame's last pixel,
    dense within the derived bound and the same bytes twice; one-hot at the rays on either side of pixel 2^32 and at both ends — a flat
    index or a product j * W held in 32 bits would move i and j there."""
    cam = rr.CAMERAS["huge_range"]
    k = (cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    worst = 0.0
    for pix0, n in rr.HUGE_RANGES:
        pix = pix0 + np.arange(n, dtype=np.int64)
        for spread in (False, True):
            g_o, g_d = _grads(n, n, spread)
            ref, mag = rr.pose_grad64(*k, pix, g_o, g_d)
            got = gpu_pose_grad(cam, g_o, g_d, pix0=pix0)
            assert rr.same_bits(got, gpu_pose_grad(cam, g_o, g_d, pix0=pix0)), "two runs differ"
            ratio = float((np.abs(got.astype(np.float64) - ref) / rr.pose_grad_bound(ref, mag, n)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (pix0, spread, ratio, got, ref)
    print(f"pose gradient huge_range: worst |got - ref| / bound {worst:.3f}")
    pix0, n = rr.HUGE_RANGES[0]
    pix = pix0 + np.arange(n, dtype=np.int64)
    assert pix[299] == 2 ** 32 - 1 and pix[300] == 2 ** 32
    dirs = np.stack(rr.camera_dirs(cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], pix), -1)
    for r in (0, 299, 300, 599):
        for a in range(3):
            g = np.float32((-1) ** (r + a) * (1.2345678 + r / 7))
            hot, zero = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
            hot[r, a] = g
            want = np.zeros((3, 4), np.float32)
            want[a, :3] = (np.float64(g) * dirs[r].astype(np.float64)).astype(np.float32)
            got = gpu_pose_grad(cam, zero, hot, pix0=pix0)
            assert np.array_equal(got, want), (r, a, got, want)


# ---- 6. autograd -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows4", [False, True])
@pytest.mark.parametrize("give_hw", [True, False])
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_rays_at_pixels_forward_bits_and_pose_gradient(name, give_hw, rows4):
    cam = rr.CAMERAS[name]
    H, W, n = cam["H"], cam["W"], 300
    rng = np.random.default_rng(H + 2 * give_hw + rows4)
    rows, cols = rng.integers(0, H, n), rng.integers(0, W, n)
    cols[0] = W - 1                                                                # (the W = 0 default reads the width off the largest column)
    full = np.eye(4, dtype=np.float32)
    full[:3] = cam["c2w"]
    c2w = dev(full[:4 if rows4 else 3]).requires_grad_(True)
    out = rays.rays_at_pixels(rr.intrinsics(cam), c2w, dev(rows), dev(cols), *((H, W) if give_hw else ()))
    pix = rows.astype(np.int64) * W + cols
    ro, rd, _ = want_rays(cam, pix)
    assert rr.same_bits(out[0].detach().cpu().numpy(), ro) and rr.same_bits(out[1].detach().cpu().numpy(), rd)
    g_o, g_d = _grads(n, H, False)
    ((out[0] * dev(g_o)).sum() + (out[1] * dev(g_d)).sum()).backward()
    torch.cuda.synchronize()
    got = c2w.grad.cpu().numpy().astype(np.float64)
    ref, mag = rr.pose_grad64(W, cam["fx"], cam["fy"], cam["cx"], cam["cy"], pix, g_o, g_d)
    assert (np.abs(got[:3] - ref) <= rr.pose_grad_bound(ref, mag, n)).all()
    assert got.shape == ((4, 4) if rows4 else (3, 4)) and (not rows4 or not got[3].any())


# ---- 7. one whole frame ------------------------------------------------------------------------------------------------------------------
def test_a_frame_from_the_pose_is_the_frame_from_the_restatements_rays():
    """`wide` through ``render(H, W, K, c2w=pose)`` and through ``render(rays=...)`` / the same for ``render_geometry``: bit-equal maps."""
    cam = rr.CAMERAS["wide"]
    H, W, K = cam["H"], cam["W"], rr.intrinsics(cam)
    render, kw, _ = make_product((8, 64, 10, 64), 0, 4096, DEV, with_tex=True)
    bm, _, exp = (t.to(DEV) for t in synth.codes(0))
    uv = dev(np.random.default_rng(5).uniform(0, 1, (512, 512, 3)).astype(np.float32))
    ro, rd, _ = want_rays(cam, np.arange(H * W, dtype=np.int64))
    held = torch.stack([dev(ro).reshape(H, W, 3), dev(rd).reshape(H, W, 3)], 0)
    pose = torch.from_numpy(cam["c2w"])
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    with torch.no_grad():
        a = render.render(H, W, K, chunk=512, c2w=pose, shapeCodes=bm, uvMap=uv, expType=3, **kw)
        b = render.render(H, W, K, chunk=512, rays=held, shapeCodes=bm, uvMap=uv, expType=3, **kw)
    for k, what in enumerate(("rgb", "disp", "acc")):
        assert a[k].shape[:2] == (H, W) and same(a[k], b[k]), what
    assert float(a[2].max()) > 0.1
    ga = render.render_geometry(H, W, K, chunk=512, c2w=pose, shapeCodes=bm, expType=20, expCodes=exp, **kw)
    gb = render.render_geometry(H, W, K, chunk=512, rays=held, shapeCodes=bm, expType=20, expCodes=exp, **kw)
    for k, what in enumerate(("depth", "disp", "acc")):
        assert ga[k].shape == (H, W) and same(ga[k], gb[k]), what


# ---- 8. the rasteriser's camera is the rays' camera --------------------------------------------------------------------------------------
def test_a_small_face_on_a_ray_covers_that_rays_pixel():
    """The two camera conventions against each other on `wide`: a triangle of a third of a pixel around o + 5 d_ij, in the plane at camera
    depth 5, is drawn into pixel (i, j) and no other, at depth 5."""
    cam = rr.CAMERAS["wide"]
    H, W = cam["H"], cam["W"]
    targets = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (17, 9), (18, 10), (5, 20), (30, 3)]          # (i, j) = (column, row)
    pix = np.asarray([j * W + i for i, j in targets], np.int64)
    ro, rd, _ = want_rays(cam, pix)
    centre = ro.astype(np.float64) + 5.0 * rd.astype(np.float64)
    R = cam["c2w"][:, :3].astype(np.float64)
    rx, ry = 5.0 / cam["fx"] / 3, 5.0 / cam["fy"] / 3                              # a third of a pixel's footprint at depth 5
    verts = np.concatenate([centre[k] + np.stack([rx * np.cos(t) * R[:, 0] + ry * np.sin(t) * R[:, 1] for t in (0.3, 2.4, 4.5)]) for k in range(8)])
    faces = np.arange(24, dtype=np.int32).reshape(8, 3)
    out = mesh.rasterize(dev(verts.astype(np.float32)), dev(faces), H, W, rr.intrinsics(cam).astype(np.float32), cam["c2w"])
    face, depth = out["face"].cpu().numpy(), out["depth"].cpu().numpy()
    assert (face >= 0).sum() == 8
    for k, (i, j) in enumerate(targets):
        assert face[j, i] == k and abs(float(depth[j, i]) - 5.0) <= 8 * 2.0 ** -24 * 5, (k, i, j, face[j, i], depth[j, i])


# ---- 9. NDC ------------------------------------------------------------------------------------------------------------------------------
def test_ndc_rays_within_four_times_the_cpu_evaluations_own_error():
    """``rays.ndc_rays`` on the device against the oracle's formula in fp64.  The formula cancels, so the tolerance is measured, not
    derived: the CPU fp32 oracle's own worst error on these rays, four times over (the device may order the elementwise operations
    differently); profiles/ray_generation_audit.md holds both figures."""
    cam = rr.CAMERAS["wide"]
    cpu_err, swapped, (o64, d64) = rr.ndc_figures()
    ro, rd, _ = want_rays(cam, np.arange(cam["H"] * cam["W"], dtype=np.int64))
    o, d = rays.ndc_rays(cam["H"], cam["W"], rr.NDC_FOCAL, rr.NDC_NEAR, dev(ro), dev(rd))
    err = max(np.abs(o.cpu().numpy().astype(np.float64) - o64).max(), np.abs(d.cpu().numpy().astype(np.float64) - d64).max())
    print(f"ndc_rays on wide: device worst error {err:.3e}, CPU fp32 oracle {cpu_err:.3e}, allowed {4 * cpu_err:.3e} (H/W swapped: {swapped:.3e})")
    assert err <= 4 * cpu_err < swapped

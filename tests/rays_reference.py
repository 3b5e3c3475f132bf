"""Yardsticks of ray generation and the camera-pose gradient (``mofa_get_rays`` / ``mofa_get_rays_at`` / ``mofa_rays_pose_backward`` /
``mofa_layer0_forward_cam``: ``k_get_rays``, ``k_rays_pose_backward``, ``pinhole_ray`` and the layer-0 prologue).  NumPy only (the one NDC helper imports torch itself).

* :func:`rays` restates ``pinhole_ray`` + the view-direction normalisation in fp32, one rounding per operation.  NumPy's fp32
  ``+ - * / sqrt`` are the correctly rounded ones, so the device must give the same BITS for origins, directions and view directions.
  :func:`rays64` is the same formula in fp64; :func:`rays_window` the distance the fp32 result may keep from it.
* :func:`pose_grad64` forms ``dirs`` in fp32 exactly as ``k_rays_pose_backward`` does and takes the twelve sums exactly (``math.fsum`` of
  fp64 products of fp32 factors, which are exact); :func:`pose_grad_bound` is the distance the device may keep from it.
* ``CAMERAS``: anisotropic, non-square, off-centre cameras with generic poses; ``FAULTS``: the mistakes the comparisons must see
  (tests/test_rays_reference_cpu.py shows that they do, and that the old square camera could not)."""
import math

import numpy as np

f32 = np.float32
U24, U52 = 2.0 ** -24, 2.0 ** -52

# (name, what it reaches): "dirs" faults change the camera-space direction (rays AND pose gradient), "rays" faults the world-space step or
# the normalisation, "pose" faults the reduction of k_rays_pose_backward.
FAULTS = (
    ("swap_f", "dirs"),            # fx <-> fy
    ("swap_c", "dirs"),            # cx <-> cy
    ("div_h", "dirs"),             # j = pix / H
    ("d1_sign", "dirs"),           # d1 = +(j - cy) / fy
    ("d2_plus", "dirs"),           # d2 = +1
    ("pix32", "dirs"),             # the flat pixel index of a contiguous range held in 32 bits (shows only where H * W >= 2^31)
    ("transpose", "rays"),         # c[b][a] for c[a][b]
    ("transpose_01_12", "rays"),   # only the pairs (0,1)/(1,0) and (1,2)/(2,1): all a zero-elevation pose can hide
    ("fma", "rays"),               # fused multiply-adds (fp64 emulation rounded once)
    ("assoc", "rays"),             # a + (b + c)
    ("norm64", "rays"),            # |rd| in fp64, rounded once
    ("pose_no_pix0", "pose"),      # the contiguous-range form starts at pixel 0
    ("pose_t256", "pose"),         # rays t >= 256 dropped (the thread's loop runs once)
    ("pose_lanes128", "pose"),     # threads 128..255 (wavefronts 2 and 3) dropped
    ("pose_col3_from_d", "pose"),  # d_c2w[a][3] summed from d_rays_d
)
FAULT_NAMES = tuple(n for n, _ in FAULTS)
OLD_TESTS_MISSED = ("swap_f", "swap_c", "div_h", "transpose_01_12", "pose_no_pix0", "pose_t256", "pose_lanes128")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- cameras ---------------------------------------------------------------------------------------------------------------------------
def pose_spherical(phi, theta, radius, roll=0.0, shift=(0.0, 0.0, 0.0)):
    """float32 [3,4]: R_y(phi) R_x(theta) T_z(radius) as the project's ``pose_spherical`` multiplies it (float32 products), then a roll
    about the optical axis (R_y R_x alone always has a zero at [1][0]) and a translation off the axis."""
    ph, th, ro = np.deg2rad(phi), np.deg2rad(theta), np.deg2rad(roll)
    t = np.eye(4, dtype=f32)
    t[2, 3] = radius
    rx = np.array([[1, 0, 0, 0], [0, np.cos(th), -np.sin(th), 0], [0, np.sin(th), np.cos(th), 0], [0, 0, 0, 1]], f32)
    ry = np.array([[np.cos(ph), 0, -np.sin(ph), 0], [0, 1, 0, 0], [np.sin(ph), 0, np.cos(ph), 0], [0, 0, 0, 1]], f32)
    rz = np.array([[np.cos(ro), -np.sin(ro), 0, 0], [np.sin(ro), np.cos(ro), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32)
    c = ry @ (rx @ t)
    if roll != 0.0:                    # (a product with the identity would still turn the zero-elevation poses' -0.0 entries into +0.0)
        c = c @ rz
    c[:3, 3] += np.asarray(shift, f32)
    return np.ascontiguousarray(c[:3, :4])


def _camera(H, W, fx, fy, cx, cy, pose):
    return dict(H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, c2w=pose_spherical(*pose))


_HUGE_LIST = 46340
CAMERAS = {
    "wide": _camera(23, 37, 41.5, 29.25, 17.75, 9.5, (35.0, -20.0, 4.0, 12.0, (0.3, -0.2, 0.15))),
    "tall": _camera(37, 23, 19.0, 47.0, -4.5, 40.25, (-50.0, 25.0, 3.5, -17.0, (-0.25, 0.4, 0.1))),
    "column": _camera(300, 1, 7.5, 211.25, 0.25, 149.5, (20.0, 15.0, 5.0, 8.0, (0.1, 0.2, -0.3))),
    "row": _camera(1, 300, 211.25, 7.5, 149.5, 0.25, (-25.0, -10.0, 5.0, -6.0, (-0.2, 0.1, 0.3))),
    "square": _camera(256, 256, 600.0, 600.0, 128.0, 128.0, (-60.0, 0.0, 16.0)),       # the old tests' camera: the control
    "huge_list": _camera(_HUGE_LIST, _HUGE_LIST, 40000.5, 52000.25, 23170.25, 23169.5, (35.0, -20.0, 4.0, 12.0, (0.3, -0.2, 0.15))),
    "huge_range": _camera(65536, 65537, 52000.25, 40000.5, 32768.5, 32767.25, (-50.0, 25.0, 3.5, -17.0, (-0.25, 0.4, 0.1))),
}
SMALL = ("wide", "tall", "column", "row", "square")
NEW = ("wide", "tall", "column", "row")
HUGE_RANGES = ((2 ** 32 - 300, 600), (65536 * 65537 - 257, 257))     # (pix0, n) of huge_range: across 2^32, and the frame's last pixels


def huge_list_pixels():
    """int64 [64]: pixels of ``huge_list`` (H * W < 2^31): the corners of the index range, row starts and ends, values just under 2^31."""
    H = W = _HUGE_LIST
    fixed = [0, W - 1, W, H * W - 1, H * W - W, H * W - W - 1, 2 ** 31 - 2 ** 24, (H - 1) * W - 1, 2 ** 30, 2 ** 30 + 1]
    fixed += [H * W - 2 - k for k in range(22)]
    rest = np.random.default_rng(5).integers(0, H * W, 64 - len(fixed))
    out = np.concatenate([np.asarray(fixed, np.int64), rest.astype(np.int64)])
    assert len(out) == 64 and out.max() < 2 ** 31 and out.max() > 2 ** 31 - 2 ** 17
    return out


def intrinsics(cam):
    return np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]], np.float64)


# ---- rays ------------------------------------------------------------------------------------------------------------------------------
def _wrap32(v):
    return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31


def camera_dirs(H, W, fx, fy, cx, cy, pix, fault=None, dtype=f32):
    """(d0, d1, d2) [n] each: ``[(i - cx) / fx, -((j - cy) / fy), -1]`` of the flat pixels ``pix`` (int64), one rounding per operation."""
    pix = np.asarray(pix, np.int64).reshape(-1)
    fx, fy, cx, cy = (dtype(v) for v in (fx, fy, cx, cy))
    if fault == "swap_f":
        fx, fy = fy, fx
    if fault == "swap_c":
        cx, cy = cy, cx
    div = int(H) if fault == "div_h" else int(W)
    if fault == "pix32":
        pix = _wrap32(pix)
    j = pix // div
    i = pix - j * div
    d0 = (i.astype(dtype) - cx) / fx
    d1 = (j.astype(dtype) - cy) / fy
    if fault != "d1_sign":
        d1 = -d1
    d2 = np.full(len(pix), 1 if fault == "d2_plus" else -1, dtype)
    return d0, d1, d2


def rays(H, W, fx, fy, cx, cy, c2w, pix, fault=None):
    """(rays_o, rays_d, viewdirs) float32 [n,3] of the flat pixel indices ``pix`` (int64), in the header's arithmetic:
    ``rd[a] = ((d0 c[a][0] + d1 c[a][1]) + d2 c[a][2])``, ``ro[a] = c[a][3]``, ``view = rd / sqrt((rd0^2 + rd1^2) + rd2^2)``."""
    assert fault is None or fault in FAULT_NAMES
    c = np.asarray(c2w, f32)[:3, :4]
    R = c[:, :3]
    if fault == "transpose":
        R = R.T
    elif fault == "transpose_01_12":
        R = R.copy()
        R[0, 1], R[1, 0], R[1, 2], R[2, 1] = c[1, 0], c[0, 1], c[2, 1], c[1, 2]
    d = camera_dirs(H, W, fx, fy, cx, cy, pix, fault)
    n = len(d[0])
    rd = np.empty((n, 3), f32)
    for a in range(3):
        if fault == "fma":
            t = d[0] * R[a, 0]
            t = (d[1].astype(np.float64) * np.float64(R[a, 1]) + t.astype(np.float64)).astype(f32)
            rd[:, a] = (d[2].astype(np.float64) * np.float64(R[a, 2]) + t.astype(np.float64)).astype(f32)
        elif fault == "assoc":
            rd[:, a] = d[0] * R[a, 0] + (d[1] * R[a, 1] + d[2] * R[a, 2])
        else:
            rd[:, a] = (d[0] * R[a, 0] + d[1] * R[a, 1]) + d[2] * R[a, 2]
    ro = np.broadcast_to(c[:, 3], (n, 3)).copy()
    if fault == "norm64":
        r64 = rd.astype(np.float64)
        nrm = np.sqrt((r64[:, 0] * r64[:, 0] + r64[:, 1] * r64[:, 1]) + r64[:, 2] * r64[:, 2]).astype(f32)
    else:
        nrm = np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2])
    view = rd / nrm[:, None]
    assert ro.dtype == rd.dtype == view.dtype == f32
    return ro, rd, view


def rays64(H, W, fx, fy, cx, cy, c2w, pix):
    """The same formula in fp64 from the same float32 inputs: (rays_o, rays_d, viewdirs, terms) — ``terms`` [n,3] = sum_b |d_b c[a][b]|."""
    c = np.asarray(c2w, f32)[:3, :4].astype(np.float64)
    fx, fy, cx, cy = (float(f32(v)) for v in (fx, fy, cx, cy))
    d = np.stack(camera_dirs(H, W, fx, fy, cx, cy, pix, dtype=np.float64), -1)              # [n,3]
    rd = d @ c[:, :3].T
    terms = np.abs(d) @ np.abs(c[:, :3]).T
    view = rd / np.sqrt((rd * rd).sum(-1, keepdims=True))
    return np.broadcast_to(c[:, 3], rd.shape).copy(), rd, view, terms


def rays_window(terms):
    """|rd32 - rd64| <= 4 * 2^-24 * sum |terms|.  A term d_b c[a][b] passes through at most four roundings on its way into rd[a]: the
    division, the product and the two sums (the subtraction i - cx is exact for every camera of the table: an integer below 2^17 minus a
    multiple of 1/4 of the same size; tests/test_rays_reference_cpu.py asserts it); d2 c[a][2] = -c[a][2] passes through one.  Every
    partial sum is bounded by sum |terms| (second-order terms, 6 u^2, are 2^-22 of the window)."""
    return 4 * U24 * terms


# ---- pose gradient ---------------------------------------------------------------------------------------------------------------------
def pose_grad64(W, fx, fy, cx, cy, pix, g_o, g_d, fault=None, H=None, pix0=None):
    """(d_c2w float64 [3,4], sum_abs float64 [3,4]): ``d_c2w[a][b] = sum_t g_d[t][a] dirs[t][b]`` (b < 3), ``d_c2w[a][3] = sum_t g_o[t][a]``
    with ``dirs`` in fp32 as the kernel forms them and the sums exact (``math.fsum``; a product of two float32 is exact in fp64);
    ``sum_abs`` is the sum of the magnitudes of the same terms.  ``pix0``: the start of a contiguous range (only the fault that ignores it
    needs to know)."""
    assert fault is None or fault in FAULT_NAMES
    pix = np.asarray(pix, np.int64).reshape(-1)
    if fault == "pose_no_pix0" and pix0 is not None:
        pix = pix - int(pix0)
    dirs = np.stack(camera_dirs(H if H is not None else W, W, fx, fy, cx, cy, pix, fault), -1).astype(np.float64)   # [n,3], float32 values
    g_o, g_d = np.asarray(g_o, f32).reshape(-1, 3).astype(np.float64), np.asarray(g_d, f32).reshape(-1, 3).astype(np.float64)
    assert len(g_o) == len(g_d) == len(pix)
    t = np.arange(len(pix))
    keep = np.ones(len(pix), bool)
    if fault == "pose_t256":
        keep = t < 256
    elif fault == "pose_lanes128":
        keep = (t % 256) < 128
    out, mag = np.zeros((3, 4)), np.zeros((3, 4))
    for a in range(3):
        for b in range(3):
            terms = (g_d[:, a] * dirs[:, b])[keep]
            out[a, b], mag[a, b] = math.fsum(terms), math.fsum(np.abs(terms))
        terms = (g_d[:, a] if fault == "pose_col3_from_d" else g_o[:, a])[keep]
        out[a, 3], mag[a, 3] = math.fsum(terms), math.fsum(np.abs(terms))
    return out, mag


def pose_grad_bound(ref, sum_abs, n):
    """Per entry ``2^-24 |ref| + n 2^-52 sum |terms|``: the kernel adds exact fp64 products in fp64 in an order of its own — any order of
    an n-term sum is within (n - 1) 2^-53 sum |terms| of the exact one to first order, taken twice over here, which also covers the
    second-order terms and the error's own share of the final rounding — and rounds the result once to float32 (2^-24 |ref|)."""
    return U24 * np.abs(ref) + n * U52 * sum_abs


# ---- NDC -------------------------------------------------------------------------------------------------------------------------------
NDC_NEAR, NDC_FOCAL = 1.0, 41.5


def ndc_figures():
    """(worst |oracle fp32 - oracle fp64| over both outputs, worst |fp64 with H and W exchanged - fp64|, (o64, d64)) of the oracle's
    ``ndc_rays`` on the rays of `wide`.  The oracle is torch: imported here, so that the module itself needs NumPy only."""
    import torch
    from oracle import mofa_oracle as orc
    cam = CAMERAS["wide"]
    ro, rd, _ = rays(cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["c2w"], np.arange(cam["H"] * cam["W"], dtype=np.int64))
    o, d = torch.from_numpy(ro), torch.from_numpy(rd)
    o32, d32 = orc.ndc_rays(cam["H"], cam["W"], NDC_FOCAL, NDC_NEAR, o, d)
    o64, d64 = orc.ndc_rays(cam["H"], cam["W"], NDC_FOCAL, NDC_NEAR, o.double(), d.double())
    os_, ds_ = orc.ndc_rays(cam["W"], cam["H"], NDC_FOCAL, NDC_NEAR, o.double(), d.double())
    err = max(float((o32.double() - o64).abs().max()), float((d32.double() - d64).abs().max()))
    swapped = max(float((os_ - o64).abs().max()), float((ds_ - d64).abs().max()))
    return err, swapped, (o64.numpy(), d64.numpy())

"""tests/rays_reference.py held against the oracle, fp64 and autograd on the CPU — and the record of what the old ray tests could not see.

The restatement is what tests/test_gpu_rays_audit.py compares the device with bit for bit, so it is checked here against three independent
statements of the same camera: ``oracle.mofa_oracle.get_rays`` (the reference's formula on CPU torch), the formula in fp64, and fp64 torch
autograd through the CPU branch of ``rays.rays_at_pixels``.  Every entry of ``FAULTS`` must break a comparison on one of the new cameras;
the entries of ``OLD_TESTS_MISSED`` must NOT break it on the old tests' inputs (256 x 256, fx = fy = 600, cx = cy = 128, zero elevation,
pixels (::37, ::41), 96 listed rays)."""
import numpy as np
import pytest
import torch

import rays_reference as rr
from mofanerf_amd import rays as prays, synth
from oracle import mofa_oracle as orc


def _all_pixels(cam):
    return np.arange(cam["H"] * cam["W"], dtype=np.int64)


def _args(cam):
    return cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["c2w"]


def _grads(n, seed, spread=False):
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(2, n, 3))
    if spread:
        g = g * 2.0 ** rng.integers(-20, 21, size=(2, n, 3))
    return g[0].astype(np.float32), g[1].astype(np.float32)


@pytest.mark.parametrize("name", [n for n in rr.CAMERAS if n != "square"])
def test_poses_are_generic(name):
    """No rotation entry is 0 or +-1 and the block is not symmetric: a transposed or permuted rotation changes every ray."""
    R = rr.CAMERAS[name]["c2w"][:, :3].astype(np.float64)
    assert (np.abs(R) > 0.01).all() and (np.abs(R) < 0.99).all() and np.abs(R - R.T)[np.triu_indices(3, 1)].min() > 0.01
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.abs(rr.CAMERAS[name]["c2w"][:, 3]).min() > 0.01


@pytest.mark.parametrize("name", rr.SMALL)
def test_restatement_is_the_oracle_bit_for_bit(name):
    """``rays`` == ``oracle.get_rays`` on every pixel: torch's CPU sum over the three products is ((a + b) + c), like the header's, on
    every camera of the table, so none is held to the fp64 window instead.  One difference is a zero's sign: ``torch.sum`` starts from +0,
    so where all three products are -0 (row cy of `square`, whose pose has zeros) it returns +0 and the header's order -0.  There — and
    only on `square` — the comparison is by value; every non-zero element, and every element of the other cameras, is compared by bits.
    `square` is ALSO held to the fp64 window, the oracle's directions and the restatement's alike, as for a camera whose order differed."""
    cam = rr.CAMERAS[name]
    ro, rd, _ = rr.rays(*_args(cam), _all_pixels(cam))
    oo, od = orc.get_rays(cam["H"], cam["W"], rr.intrinsics(cam), torch.from_numpy(cam["c2w"]))
    od = od.reshape(-1, 3).numpy()
    assert rr.same_bits(ro, oo.reshape(-1, 3).contiguous().numpy())
    if name == "square":
        zero = (rd == 0) & (od == 0)
        assert 0 < zero.sum() <= 256 and rr.same_bits(np.where(zero, np.float32(0), rd), np.where(zero, np.float32(0), od))
        _, d64, _, terms = rr.rays64(*_args(cam), _all_pixels(cam))
        for x32 in (rd, od):
            assert (np.abs(x32.astype(np.float64) - d64) <= rr.rays_window(terms)).all()
    else:
        assert rr.same_bits(rd, od)


@pytest.mark.parametrize("name", list(rr.CAMERAS))
def test_restatement_stays_in_the_fp64_window_and_views_are_unit(name):
    cam = rr.CAMERAS[name]
    if name == "huge_list":
        pix = rr.huge_list_pixels()
    elif name == "huge_range":
        pix = np.concatenate([p0 + np.arange(n, dtype=np.int64) for p0, n in rr.HUGE_RANGES])
    else:
        pix = _all_pixels(cam)
    ro, rd, view = rr.rays(*_args(cam), pix)
    o64, d64, v64, terms = rr.rays64(*_args(cam), pix)
    # i - cx and j - cy are exact in float32 (rays_window's premise)
    i, j = (pix % cam["W"]).astype(np.float64), (pix // cam["W"]).astype(np.float64)
    assert np.array_equal((i - cam["cx"]).astype(np.float32).astype(np.float64), i - cam["cx"])
    assert np.array_equal((j - cam["cy"]).astype(np.float32).astype(np.float64), j - cam["cy"])
    err, win = np.abs(rd.astype(np.float64) - d64), rr.rays_window(terms)
    ratio = np.where(err > 0, err / np.maximum(win, 1e-300), 0.0)
    print(f"{name}: worst |rd32 - rd64| / window {ratio.max():.3f}")
    assert ratio.max() <= 1.0 and np.array_equal(ro.astype(np.float64), o64)
    assert np.abs(np.sqrt((view.astype(np.float64) ** 2).sum(-1)) - 1).max() <= 2.0 ** -22
    assert np.abs(view.astype(np.float64) - v64).max() <= 8 * rr.U24 * (terms / np.sqrt((d64 * d64).sum(-1, keepdims=True))).max()


@pytest.mark.parametrize("name", rr.NEW)
def test_pose_gradient_is_fp64_autograd_of_the_cpu_branch(name):
    """``pose_grad64`` == d/d c2w of sum(g_o . rays_o + g_d . rays_d) through ``rays.rays_at_pixels`` on a float64 CPU pose: the same
    twelve sums (autograd forms dirs in fp64, the kernel in fp32: 2 * 2^-24 relative on a term, and fp64 summation noise)."""
    cam = rr.CAMERAS[name]
    n = 500
    pix = np.random.default_rng(3).integers(0, cam["H"] * cam["W"], n)
    g_o, g_d = _grads(n, 11)
    ref, mag = rr.pose_grad64(cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], pix, g_o, g_d)
    for shape in ((3, 4), (4, 4)):
        full = np.eye(4)
        full[:3] = cam["c2w"]
        c2w = torch.tensor(full[:shape[0]], dtype=torch.float64, requires_grad=True)
        out = prays.rays_at_pixels(rr.intrinsics(cam), c2w, torch.from_numpy(pix // cam["W"]), torch.from_numpy(pix % cam["W"]), cam["H"], cam["W"])
        (out[0] * torch.from_numpy(g_o).double()).sum().add((out[1] * torch.from_numpy(g_d).double()).sum()).backward()
        got = c2w.grad.numpy()
        assert np.abs(got[:3] - ref).max() <= (2 * rr.U24 * mag + rr.pose_grad_bound(ref, mag, n)).max()
        assert (np.abs(got[:3] - ref) <= 2 * rr.U24 * mag + n * rr.U52 * mag).all()
        assert shape[0] == 3 or not got[3].any()


def _ray_fault_seen(cam, pix, fault):
    want, got = rr.rays(*_args(cam), pix), rr.rays(*_args(cam), pix, fault=fault)
    return not all(rr.same_bits(a, b) for a, b in zip(want, got))


def _pose_fault_seen(cam, pix, fault, n, pix0=None, seed=17):
    g_o, g_d = _grads(n, seed)
    a = (cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], pix, g_o, g_d)
    ref, mag = rr.pose_grad64(*a)
    bad, _ = rr.pose_grad64(*a, fault=fault, H=cam["H"], pix0=pix0)
    # the device result is within the bound of `ref`; a faulty device would be within the bound of `bad`: seen iff the two cannot both hold
    return bool((np.abs(bad - ref) > 2 * rr.pose_grad_bound(ref, mag, n)).any())


def _fault_seen(name, fault, kind):
    """Rays over the whole frame (a range across 2^32 for huge_range); the pose gradient over 1000 listed pixels, or — for the fault that
    ignores pix0 — over a contiguous range that starts mid-row.  A `dirs` fault has to show in both."""
    cam = rr.CAMERAS[name]
    P = cam["H"] * cam["W"]
    if name == "huge_range":
        pix0, n = rr.HUGE_RANGES[0]
        frame = listed = pix0 + np.arange(n, dtype=np.int64)
    else:
        pix0 = max(cam["W"] - 3, 5)
        frame, listed = _all_pixels(cam), (pix0 + 7 * np.arange(1000, dtype=np.int64)) % P
    seen = []
    if kind in ("dirs", "rays"):
        seen.append(_ray_fault_seen(cam, frame, fault))
    if fault == "pose_no_pix0":
        n = min(600, P - pix0)
        seen.append(_pose_fault_seen(cam, pix0 + np.arange(n, dtype=np.int64), fault, n, pix0=pix0))
    elif kind in ("dirs", "pose"):
        seen.append(_pose_fault_seen(cam, listed, fault, len(listed)))
    return all(seen)


@pytest.mark.parametrize("fault,kind", rr.FAULTS)
def test_every_fault_breaks_a_comparison_on_the_new_cameras(fault, kind):
    seen = {name: _fault_seen(name, fault, kind) for name in rr.NEW}
    print(fault, seen)
    if fault == "pix32":                                                           # only an image of 2^31 pixels or more shows it
        assert not any(seen.values()) and _fault_seen("huge_range", fault, kind)
    else:
        assert any(seen.values()), seen


def test_the_old_cameras_could_not_see_these_faults():
    """The gap on record: on the old tests' inputs — the square camera, three zero-elevation poses, the pixels (::37, ::41) of
    test_get_rays_golden / test_get_rays_at_pixel_list_is_bit_exact, the 64 x 64 list and range of the layer-0 test (fx == fy, centred), 96
    listed rays in the pose gradient — the faults of ``OLD_TESTS_MISSED`` change nothing, while each of them is seen above."""
    sq = rr.CAMERAS["square"]
    rows, cols = np.meshgrid(np.arange(0, 256, 37), np.arange(0, 256, 41), indexing="ij")
    sub = (rows * 256 + cols).reshape(-1).astype(np.int64)
    for fault in ("swap_f", "swap_c", "div_h", "transpose_01_12"):
        for ang in (-60.0, 0.0, 60.0):
            cam = dict(sq, c2w=rr.pose_spherical(ang, 0.0, 16.0))
            assert rr.same_bits(cam["c2w"], orc.pose_spherical(ang, 0.0, 16.0)[:3, :4].contiguous().numpy())
            assert not _ray_fault_seen(cam, sub, fault), (fault, ang)
            assert not _ray_fault_seen(cam, _all_pixels(cam), fault), (fault, ang)         # the whole frame cannot see them either
    # the layer-0 test's camera: 64 x 64, synth.intrinsics (fx == fy, centred), -35 degrees, its 300 listed pixels and its range [1000, 1517)
    K = synth.intrinsics(64, 64)
    l0 = dict(H=64, W=64, fx=float(K[0][0]), fy=float(K[1][1]), cx=float(K[0][2]), cy=float(K[1][2]), c2w=rr.pose_spherical(-35.0, 0.0, 16.0))
    assert l0["fx"] == l0["fy"] and l0["cx"] == l0["cy"]
    for pix in (np.random.default_rng(31).choice(64 * 64, 300, replace=False).astype(np.int64), 1000 + np.arange(517, dtype=np.int64)):
        for fault in ("swap_f", "swap_c", "div_h", "transpose_01_12"):
            assert not _ray_fault_seen(l0, pix, fault), fault
    assert _ray_fault_seen(sq, sub, "transpose")                                   # (the full transpose was visible at +-60 degrees)
    # the pose gradient: 96 listed pixels of a square image, W named H
    pix96 = np.random.default_rng(2).choice(256 * 256, 96, replace=False).astype(np.int64)
    for fault in ("swap_f", "swap_c", "div_h", "pose_no_pix0", "pose_t256", "pose_lanes128"):
        assert not _pose_fault_seen(sq, pix96, fault, 96), fault
    for fault in ("swap_f", "swap_c", "div_h", "pose_t256", "pose_lanes128"):      # ... and are seen at 1000 rays of `wide`
        wide = rr.CAMERAS["wide"]
        assert _pose_fault_seen(wide, np.arange(1000, dtype=np.int64) % (23 * 37), fault, 1000), fault
    assert set(rr.OLD_TESTS_MISSED) <= set(rr.FAULT_NAMES)


def test_ndc_scale_factors_swapped_exceed_the_measured_bound():
    """``rays.ndc_rays`` on `wide`: the CPU fp32 evaluation's own worst error against fp64 (the figure the GPU test allows four times
    over), and an H / W swap in the scale factors far outside it."""
    err, swapped, _ = rr.ndc_figures()
    print(f"ndc on wide: CPU fp32 worst error {err:.3e}; H/W swapped {swapped:.3e}")
    assert swapped > 1000 * 4 * err


"""The sigma-gated forward (mofa_net_forward_gated) on a GPU: the colour half of a chain-capable network runs only where the raw density is
not <= 0, and every frame is the same bits as the full forward's.  MOFA_GATE=0 is the full forward: the A/B arm of every test here."""
import os

import numpy as np
import pytest
import torch

from harness import make_product
from mofanerf_amd import lib, synth
from mofanerf_amd.rays import get_rays, pose_spherical

pytestmark = pytest.mark.gpu
DEV = "cuda"
KNOBS = ("MOFA_PIPE", "MOFA_CHAIN", "MOFA_FUSED", "MOFA_CHAIN_TRAIN", "MOFA_GATE", "MOFA_STREAMS")


@pytest.fixture(autouse=True)
def _shipped_launch_forms(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    lib.reload_env()
    lib.test_hooks()
    yield
    monkeypatch.undo()
    lib.reload_env()
    lib.test_hooks()


def set_gate(on):
    os.environ["MOFA_GATE"] = "1" if on else "0"
    lib.reload_env()


def codes():
    return [t.to(DEV) for t in synth.codes(0)]


def scene(H, angle=25.0):
    K = synth.intrinsics(H, H)
    ro, rd = get_rays(H, H, K, pose_spherical(angle, 0.0, 16.0), device=DEV)
    return K, torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0).contiguous()


def frame(render, kw, H, K, rays, chunk=4096, seed=0, grad=False, **more):
    bm, tex, exp = codes()
    torch.manual_seed(seed)                       # perturbed sampling draws from torch's generator: the same numbers in both arms
    with torch.set_grad_enabled(grad):
        rgb, disp, acc, ex = render.render_fitting(H, H, K, chunk=chunk, rays=rays, shapeCodes=bm, uvCodes=tex, expType=20, expCodes=exp,
                                                   verbose=True, **dict(kw, **more))
    render.check_launches(block=True)
    out = dict(rgb=rgb, disp=disp, acc=acc, **{k: v for k, v in ex.items() if torch.is_tensor(v)})
    return {k: v.detach().clone() for k, v in out.items()}


def same_frames(a, b):
    assert a.keys() == b.keys() and {"rgb", "acc", "rgb0", "acc0", "z_std", "_z_samples", "_z_fine", "_weights0"} <= a.keys()
    for k in a:
        if k.startswith("disp"):
            assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])) and torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k])), k
        else:
            assert torch.equal(a[k], b[k]), k


def fine(render, kw):
    return render._hip(kw["network_fine"])


def stats_of(render, h):
    return render.gate_stats(reset=True).get((h.D, h.W), {"samples": 0, "live": 0})


@pytest.mark.parametrize("W", [512, 1024])
@pytest.mark.parametrize("white,perturb,streams", [(False, 0., 1), (True, 0., 1), (False, 1., 1), (True, 1., 2)])
def test_a_gated_frame_is_the_full_forwards_frame_bit_for_bit(W, white, perturb, streams):
    """render_fitting with MOFA_GATE=1 against MOFA_GATE=0: det / perturbed sampling, white background, three sub-batches per pass (the
    last one short), one and two streams.  The fine pass must really have been gated, on a mix of live and dead samples."""
    H = 12                                                  # 144 rays x 128 fine samples, 64 rays per sub-batch: 64 + 64 + 16 rays
    render, kw, _ = make_product((8, 64, 10, W), 0, 8192, DEV)
    render.n_streams = streams
    K, rays = scene(H)
    more = dict(white_bkgd=white, perturb=perturb)
    set_gate(False)
    ref = frame(render, kw, H, K, rays, **more)
    h = fine(render, kw)
    assert h.last_gated in (None, 0) and stats_of(render, h)["samples"] == 0
    set_gate(True)
    out = frame(render, kw, H, K, rays, **more)
    st = stats_of(render, h)
    print("gate", W, white, perturb, streams, st)
    assert h.last_gated == 1
    assert st["samples"] == H * H * 128 and 0 < st["live"] < st["samples"], st
    assert render._hip(kw["network_fn"]).last_gated == 0    # width 64: the persistent kernel, never gated — and it says so
    same_frames(out, ref)


@pytest.mark.parametrize("W", [512, 1024])
@pytest.mark.parametrize("points", [False, True])
def test_the_entry_point_keeps_sigma_everywhere_and_rgb_on_the_live_rows(W, points):
    """mofa_net_forward_gated against mofa_net_forward on the same sub-batch (rays with z, or explicit points): sigma is the same bits
    everywhere, all four channels on the live rows, rgb is exactly 0 on the dead rows; a NaN density is live."""
    render, kw, _ = make_product((8, 64, 10, W), 0, 8192, DEV)
    H = 8
    K, rays = scene(H)
    frame(render, kw, H, K, rays)                           # folds the codes of the fine network
    h, folded = fine(render, kw), render._folded_fine
    render.gate_stats(reset=True)                           # (that frame's own counts)
    R, S = 37, 128                                          # 4,736 samples: 18.5 row tiles
    g = torch.Generator().manual_seed(5)
    o = (rays[0, :R] + 0.05 * torch.randn(R, 3, generator=g).to(DEV)).contiguous()
    d = rays[1, :R].contiguous()
    o[3] = float("nan")                                     # a non-finite ray: NaN densities, which must stay live
    vd = torch.nn.functional.normalize(torch.nan_to_num(d), dim=-1).contiguous()
    z = (8.0 + 18.0 * torch.rand(R, S, generator=g)).sort(-1).values.to(DEV).contiguous()
    full, gated = torch.full((R, S, 4), 7.0, device=DEV), torch.full((R, S, 4), 7.0, device=DEV)
    if points:
        pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).contiguous()
        h.forward_points(pts, vd, S, full, folded)
        h.forward_points(pts, vd, S, gated, folded, gate=True)
    else:
        h.forward_rays(o, d, z, S, vd, S, full, folded)
        h.forward_rays(o, d, z, S, vd, S, gated, folded, gate=True)
    torch.cuda.synchronize()
    h.check_verdict(block=True)
    assert h.last_gated == 1
    n, live_n = (int(v) for v in h.gate_stats_dev.tolist())
    bits = lambda t: t.contiguous().view(torch.int32)
    sigma = full[..., 3]
    live = ~(sigma <= 0)
    print("entry", W, points, n, live_n)
    # (the ragged case; a live count at an exact multiple of 256 is prescribed in tests/test_gpu_gate_patterns.py)
    assert n == R * S and live_n == int(live.sum()) and 0 < live_n < n and live_n % 256 != 0
    assert torch.isnan(sigma[3]).all() and live[3].all()
    assert torch.equal(bits(gated[..., 3]), bits(sigma))
    assert torch.equal(bits(gated[live]), bits(full[live]))
    assert torch.equal(bits(gated[~live][:, :3]), torch.zeros(int((~live).sum()), 3, dtype=torch.int32, device=DEV))
    assert (full[~live][:, :3] != 0).any()                  # the full forward did compute colours there: the comparison is not vacuous


@pytest.mark.parametrize("shift", [1e6, -1e6])
def test_all_live_and_all_dead_networks_give_equal_frames(shift):
    render, kw, _ = make_product((8, 64, 10, 512), 0, 8192, DEV)
    H = 12
    K, rays = scene(H)
    with torch.no_grad():
        kw["network_fine"].alpha_linear[0].bias += shift
    set_gate(False)
    ref = frame(render, kw, H, K, rays)
    set_gate(True)
    out = frame(render, kw, H, K, rays)
    h = fine(render, kw)
    st = stats_of(render, h)
    assert h.last_gated == 1 and st["samples"] == H * H * 128 and st["live"] == (st["samples"] if shift > 0 else 0), st
    same_frames(out, ref)


def test_a_gated_render_under_no_grad_issues_no_host_sync():
    """tests/test_gpu_render.py::test_render_under_no_grad_issues_no_host_sync at a chain-capable width: the live count never leaves the device."""
    render, kw, _ = make_product((8, 64, 10, 512), 0, 4096, DEV)
    bm, tex, exp = codes()
    K = synth.intrinsics(16, 16)
    poses = [pose_spherical(a, 0.0, 16.0)[:3, :4].to(DEV) for a in (0.0, 30.0)]
    call = lambda pose: render.render_fitting(16, 16, K, chunk=96, c2w=pose, shapeCodes=bm, uvCodes=tex, expType=20, expCodes=exp, **kw)
    with torch.no_grad():
        ref = [t.clone() if torch.is_tensor(t) else t for t in call(poses[1])[:3]]      # warm-up: packs weights, caches the sample rows
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            call(poses[0])
            out = call(poses[1])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert fine(render, kw).last_gated == 1
    assert all(torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() for a, b in zip(out[:3], ref))
    assert torch.equal(out[0], ref[0])


def test_retraw_noise_and_gradients_take_the_full_forward():
    """Whoever reads raw itself (retraw), adds noise to sigma, or keeps a tape gets today's path: the gated entry is not even called."""
    render, kw, _ = make_product((8, 64, 10, 512), 0, 8192, DEV)
    H = 8
    K, rays = scene(H)
    h = fine(render, kw)
    set_gate(False)
    noisy_ref = frame(render, kw, H, K, rays, raw_noise_std=1.0, pytest=True)
    set_gate(True)
    h.last_gated = None
    noisy = frame(render, kw, H, K, rays, raw_noise_std=1.0, pytest=True)
    assert h.last_gated is None
    same_frames(noisy, noisy_ref)
    frame(render, kw, H, K, rays, grad=True)
    assert h.last_gated is None
    gated = frame(render, kw, H, K, rays)                    # (also leaves self.rays and the folded codes for the direct call below)
    assert h.last_gated == 1
    h.last_gated = None
    args = dict(network_fn=kw["network_fn"], network_fine=kw["network_fine"], N_samples=64, N_importance=64)
    with torch.no_grad():
        ret = render.render_rays([0, H * H], retraw=True, **args)
        assert h.last_gated is None
        full = torch.empty_like(ret["raw"])
        z_fine = render.render_rays([0, H * H], verbose=True, **args)["_z_fine"].contiguous()
        h.forward_rays(rays[0], rays[1], z_fine, 128, render.rays[:, 8:11].contiguous(), 128, full, render._folded_fine)
    render.check_launches(block=True)
    assert torch.equal(ret["raw"], full) and (full[..., :3][full[..., 3] <= 0] != 0).any()
    assert torch.equal(ret["rgb_map"].reshape(-1, 3), gated["rgb"].reshape(-1, 3))


def test_an_incomplete_colour_launch_is_loud_not_wrong():
    """mofa_test_hooks(chain_spin_limit=1) on the COLOUR launch alone (colour_only: the geometry launch keeps the shipped budget, so the live
    count is the real one): a NaN frame and a MofaError, as for the single chained launch — raised by the colour launch's own verification
    (expected tiles = the device's live row tiles x tiles per row tile), which the verdict words show: of the six launches of the fine
    pass's three sub-batches exactly the three colour launches are bad, and the last one finished fewer tiles than it has."""
    render, kw, _ = make_product((8, 64, 10, 512), 0, 8192, DEV)
    H = 12
    K, rays = scene(H)
    good = frame(render, kw, H, K, rays)
    h = fine(render, kw)
    assert torch.isfinite(good["rgb"]).all() and h.last_gated == 1
    before = h._verdict.tolist()
    assert before[0] == 0 and before[5] == 0
    bm, tex, exp = codes()
    lib.test_hooks(chain_spin_limit=1, colour_only=True)
    with torch.no_grad():
        bad = render.render_fitting(H, H, K, chunk=4096, rays=rays, shapeCodes=bm, uvCodes=tex, expType=20, expCodes=exp, **kw)[0]
    torch.cuda.synchronize()
    lib.test_hooks()
    after = h._verdict.tolist()
    print("verdict", before, after)
    assert torch.isnan(bad).all()
    assert after[1] - before[1] == 6                        # 3 sub-batches x (geometry + colour)
    assert after[5] - before[5] == 3                        # the colour launches, flagged by their own verification
    assert after[0] & 1 and 0 < after[4] and after[3] < after[4]    # the last one: a wait timed out, finished < live row tiles x tiles per row tile
    with pytest.raises(lib.MofaError, match="did not complete"):
        render.check_launches(block=True)
    again = frame(render, kw, H, K, rays)
    same_frames(again, good)


def test_the_profiler_counts_the_row_tiles_executed_not_the_upper_bound():
    """mofa_prof_end's kind 5 (k_net_chain<0>) after ONE gated call: the geometry half over every row tile plus the colour half over the
    live row tiles only — a host term and a device-side sum — and below the dense figure of the same call."""
    import ctypes as C
    W, D = 1024, 10
    render, kw, _ = make_product((8, 64, D, W), 0, 8192, DEV)
    H = 8
    K, rays = scene(H)
    frame(render, kw, H, K, rays)
    h, folded = fine(render, kw), render._folded_fine
    render.gate_stats(reset=True)
    R, S = 37, 128
    o, d = rays[0, :R].contiguous(), rays[1, :R].contiguous()
    vd = torch.nn.functional.normalize(d, dim=-1).contiguous()
    z = torch.linspace(8.0, 26.0, S, device=DEV)[None, :].expand(R, S).contiguous()
    raw = torch.empty(R, S, 4, device=DEV)
    L = lib.load()

    def session(gate):
        ms, launches, flops = (C.c_double * lib.PROF_KINDS)(), (C.c_int64 * lib.PROF_KINDS)(), (C.c_double * lib.PROF_KINDS)()
        torch.cuda.synchronize()
        lib.check(L.mofa_prof_begin(), "mofa_prof_begin")
        h.forward_rays(o, d, z, S, vd, S, raw, folded, gate=gate)
        lib.check(L.mofa_prof_end(ms, launches, flops), "mofa_prof_end")
        return int(launches[5]), float(flops[5])

    dense_launches, dense = session(False)
    gated_launches, got = session(True)
    n, live = (int(v) for v in h.gate_stats_dev.tolist())
    tiles, live_tiles = (R * S + 255) // 256, (live + 255) // 256
    # MACs per row over the MFMA layers (padded widths; layer 0 contracts the 64-wide encoding panels)
    geometry = 64 * W + 3 * W * W + 5 * W * W + 2 * W * W + (D - 6) * W * W
    colour = 5 * W * W + 2 * W * W + (D - 6) * W * W + W * (W // 2)
    print("prof", n, live, tiles, live_tiles, dense, got)
    assert h.last_gated == 1 and n == R * S and 0 < live_tiles < tiles
    assert (dense_launches, gated_launches) == (1, 2)
    assert dense == 2.0 * 256 * tiles * (geometry + colour)
    assert got == 2.0 * 256 * (tiles * geometry + live_tiles * colour) and got < dense

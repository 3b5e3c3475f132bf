#!/usr/bin/env python3
"""A/B of the sigma-gated forward at the headline shape (bench.py's: a 512^2 view, 64 coarse + 128 fine samples, coarse 256 x 8 and fine
1024 x 10 networks, seeded weights, the three novel views 0 / -60 / +60 degrees): renders every view with ``MOFA_GATE=0`` and with
``MOFA_GATE=1`` (interleaved, ``--reps`` times each after one warm-up), checks that the frames are the same bits and prints ONE JSON line:
the median frame time per view and arm, the live share of the fine pass per view (device-side counters, read outside the timed region)
and the predicted frame-time ratio 1 - f * 0.45 * (1 - live) for ``--chain-share f``.

``--all-live`` / ``--all-dead`` add / subtract 1e6 to the fine network's ``alpha_linear.0.bias``: every sample live (what the gate costs
when it saves nothing) / every sample dead (what the colour launch costs when it has nothing to do).

  python tools/gate_ab.py --reps 2
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import factory, lib, synth  # noqa: E402
from mofanerf_amd.rays import get_rays, pose_spherical  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arch", type=int, nargs=4, default=[8, 256, 10, 1024], metavar=("Dc", "Wc", "Df", "Wf"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=2, help="timed frames per view and arm")
    ap.add_argument("--angles", type=float, nargs="+", default=[0.0, -60.0, 60.0])
    ap.add_argument("--chain-share", type=float, default=0.9685, help="k_net_chain<0>'s share of the ungated frame (bench.py --full)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--all-live", action="store_true")
    g.add_argument("--all-dead", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    Dc, Wc, Df, Wf = a.arch
    args = factory.default_args(netdepth=Dc, netwidth=Wc, netdepth_fine=Df, netwidth_fine=Wf, no_reload=True, device=dev,
                                basedir="/nonexistent", N_samples=64, N_importance=128)
    _, kw, _, _, _, _, render = factory.create_nerf(args)
    kw["network_fn"].load_state_dict(synth.nerf_state(Dc, Wc, 0, "coarse"))
    kw["network_fine"].load_state_dict(synth.nerf_state(Df, Wf, 0, "fine"))
    render.idSpecificMod.load_state_dict(synth.style_state(0))
    for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(0)):
        dst.data[:] = src.to(dst.device)
    kw.update(near=8.0, far=26.0)
    render.eval()
    if a.all_live or a.all_dead:
        with torch.no_grad():
            kw["network_fine"].alpha_linear[0].bias += 1e6 if a.all_live else -1e6
    bm, tex, exp = (t.to(dev) for t in synth.codes(0))
    H = a.size
    K = synth.intrinsics(H, H)
    rays = {}
    for ang in a.angles:
        ro, rd = get_rays(H, H, K, pose_spherical(ang, 0.0, 16.0), device=dev)
        rays[ang] = torch.stack([ro.reshape(-1, 3), rd.reshape(-1, 3)], 0).contiguous()

    def frame(ang, gate):
        os.environ["MOFA_GATE"] = "1" if gate else "0"
        lib.reload_env()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        with torch.no_grad():
            rgb, disp, acc, _ = render.render_fitting(H, H, K, chunk=args.chunk, rays=rays[ang], shapeCodes=bm, uvCodes=tex, expType=20,
                                                      expCodes=exp, **kw)
        e1.record()
        torch.cuda.synchronize()
        render.check_launches(block=True)
        return e0.elapsed_time(e1), (rgb, disp, acc)

    frame(a.angles[0], False), frame(a.angles[0], True)                    # warm-up: packs, const rows, workspaces
    render.gate_stats(reset=True)
    ms = {(ang, gate): [] for ang in a.angles for gate in (0, 1)}
    live, same = {}, True
    for ang in a.angles:
        for _ in range(a.reps):
            t0, ref = frame(ang, False)
            t1, out = frame(ang, True)
            ms[ang, 0].append(t0), ms[ang, 1].append(t1)
            same = same and torch.equal(out[0], ref[0]) and torch.equal(out[2], ref[2]) and \
                torch.equal(torch.nan_to_num(out[1]), torch.nan_to_num(ref[1])) and torch.equal(torch.isnan(out[1]), torch.isnan(ref[1]))
        st = render.gate_stats(reset=True).get((Df, Wf), {"samples": 0, "live": 0})
        live[ang] = st["live"] / max(1, st["samples"])
    med = lambda v: round(statistics.median(v), 1)
    views = {str(ang): {"full_ms": med(ms[ang, 0]), "gated_ms": med(ms[ang, 1]), "ratio": round(med(ms[ang, 1]) / med(ms[ang, 0]), 4),
                        "live_share": round(live[ang], 4),
                        "predicted_ratio": round(1.0 - a.chain_share * 0.45 * (1.0 - live[ang]), 4)} for ang in a.angles}
    full, gated = sum(v["full_ms"] for v in views.values()), sum(v["gated_ms"] for v in views.values())
    print(json.dumps({"arm": "all-live" if a.all_live else "all-dead" if a.all_dead else "seeded", "arch": a.arch, "size": H, "reps": a.reps,
                      "frames_equal": bool(same), "views": views, "ratio_all_views": round(gated / full, 4),
                      "dead_share_all_views": round(1.0 - sum(live.values()) / len(live), 4)}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

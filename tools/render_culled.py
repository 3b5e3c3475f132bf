#!/usr/bin/env python3
"""Render novel views with occupancy culling (``Renderer.build_occupancy`` + ``render_fitting(..., occupancy=grid)``) and, with
``--compare``, without it; prints ONE JSON line: frame time of each arm (median after warm-up), the kept fraction per pass, the largest
|rgb| and |acc| difference to the un-culled frames and the grid build time.

Networks come from a checkpoint (``--ckpt DIR`` or one ``.tar``, as tools/extract_mesh.py) or from seeded synthetic weights
(``--synthetic DC WC DF WF``); codes from ``--fit saving_Parameters.tar`` or ``synth.codes``.  ``--bounds`` is required and
``--threshold`` has no default (no density level of a trained model has been measured).  ``--sphere RADIUS`` replaces the
network-derived grid by an analytic ball around ``--sphere-centre`` (density r^2 - |p - c|^2, threshold 0): a seeded network has no face
in it, so measurements of the culling itself use a ball of a chosen size; a radius beyond the bounds gives an all-occupied grid.

  python tools/render_culled.py --synthetic 8 256 10 1024 --bounds -4 -4 -4 4 4 4 --sphere 3.0 --size 512 --poses 3 --compare
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import factory, mesh, occupancy, synth  # noqa: E402
from mofanerf_amd.rays import pose_spherical  # noqa: E402


def load(a, dev):
    if a.synthetic:
        Dc, Wc, Df, Wf = a.synthetic
        args = factory.default_args(netdepth=Dc, netwidth=Wc, netdepth_fine=Df, netwidth_fine=Wf, netchunk=a.netchunk, no_reload=True,
                                    device=dev, basedir="/nonexistent", N_samples=a.samples[0], N_importance=a.samples[1])
    elif os.path.isdir(a.ckpt):
        path = os.path.abspath(a.ckpt)
        args = factory.default_args(basedir=os.path.dirname(path), expname=os.path.basename(path), device=dev, netchunk=a.netchunk,
                                    N_samples=a.samples[0], N_importance=a.samples[1])
    else:
        args = factory.default_args(ft_path=a.ckpt, device=dev, netchunk=a.netchunk, N_samples=a.samples[0], N_importance=a.samples[1])
    _, kw, _, _, _, _, render = factory.create_nerf(args)
    if a.synthetic:
        kw["network_fn"].load_state_dict(synth.nerf_state(Dc, Wc, a.seed, "coarse"))
        if kw.get("network_fine") is not None:
            kw["network_fine"].load_state_dict(synth.nerf_state(Df, Wf, a.seed, "fine"))
        render.idSpecificMod.load_state_dict(synth.style_state(a.seed))
        for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(a.seed)):
            dst.data[:] = src.to(dst.device)
    render.eval()
    if a.fit:
        fit = torch.load(a.fit, map_location=dev)
        bm, uv, exp = fit["saving_bm"], fit["saving_uv"], fit["saving_exp"]
    else:
        bm, uv, exp = synth.codes(a.seed)
    return render, kw, bm.reshape(1, -1).float().to(dev), uv.reshape(-1).float().to(dev), exp.reshape(1, -1).float().to(dev)


def sphere_grid(res, lo, step, centre, radius, dev):
    """Density r^2 - |p - c|^2 on the lattice (float32 coordinates as mofa_grid_points forms them)."""
    n = res[0] * res[1] * res[2]
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    mesh.grid_points(res, lo, step, 0, n, pts)
    c = torch.tensor(centre, dtype=torch.float32, device=dev)
    return (float(radius) ** 2 - ((pts - c) ** 2).sum(-1)).reshape(res).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint directory (the newest *.tar is used) or one .tar file")
    src.add_argument("--synthetic", type=int, nargs=4, metavar=("DC", "WC", "DF", "WF"), help="seeded synthetic coarse / fine networks")
    ap.add_argument("--fit", help="saving_Parameters.tar of run_fit.py (shape / texture / expression codes); default synth.codes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bounds", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--resolution", type=int, nargs=3, default=[129, 129, 129], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--threshold", type=float, default=None, help="density above which a lattice sample counts as occupied (no default)")
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--sphere", type=float, default=None, metavar="RADIUS", help="an analytic ball instead of the networks' density")
    ap.add_argument("--sphere-centre", type=float, nargs=3, default=[0.0, 0.0, 0.0])
    ap.add_argument("--size", type=int, default=512, help="frame height = width")
    ap.add_argument("--samples", type=int, nargs=2, default=[64, 128], metavar=("N_SAMPLES", "N_IMPORTANCE"))
    ap.add_argument("--near", type=float, default=8.0)
    ap.add_argument("--far", type=float, default=26.0)
    ap.add_argument("--chunk", type=int, default=196608)
    ap.add_argument("--netchunk", type=int, default=196608)
    ap.add_argument("--poses", type=int, default=3, help="timed frames (azimuths spread over -30 .. 30 degrees at radius 16)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--compare", action="store_true", help="also render every pose un-culled: its time and the differences")
    a = ap.parse_args(argv)
    if a.sphere is None and a.threshold is None:
        ap.error("--threshold is required (or --sphere RADIUS)")
    dev = torch.device("cuda", torch.cuda.current_device())
    render, kw, bm, uv, exp = load(a, dev)
    bounds, res = (tuple(a.bounds[:3]), tuple(a.bounds[3:])), tuple(a.resolution)
    nets = [n for n in (kw["network_fn"], kw.get("network_fine")) if n is not None]
    H = a.size
    K = synth.intrinsics(H, H)
    angles = np.linspace(-30.0, 30.0, max(a.poses, 1))
    poses = [pose_spherical(float(x), 0.0, 16.0)[:3, :4] for x in angles]

    def build():
        if a.sphere is not None:
            _, lo, step = mesh.grid_spec(bounds, res)
            return occupancy.occupancy_from_grid(sphere_grid(res, lo, step, a.sphere_centre, a.sphere, dev), 0.0, lo, step, dilate=a.dilate)
        return render.build_occupancy(nets, bounds=bounds, resolution=res, threshold=a.threshold, shapeCodes=bm, expType=20, expCodes=exp,
                                      dilate=a.dilate, netchunk=a.netchunk)

    def frame(pose, **more):
        with torch.no_grad():
            rgb, _, acc, _ = render.render_fitting(H, H, K, chunk=a.chunk, c2w=pose, shapeCodes=bm, uvCodes=uv, expType=20, expCodes=exp,
                                                   **dict(kw, near=a.near, far=a.far, **more))
        render.check_launches(block=True)
        torch.cuda.synchronize()
        return rgb, acc

    def arm(**more):
        for i in range(a.warmup):
            frame(poses[i % len(poses)], **more)
        ms, frames, kept = [], [], {"coarse": [0, 0], "fine": [0, 0]}
        for pose in poses:
            t = time.perf_counter()
            frames.append(frame(pose, **more))
            ms.append((time.perf_counter() - t) * 1e3)
            for which, st in (render.occupancy_stats or {}).items():
                kept[which][0] += st["kept"]
                kept[which][1] += st["samples"]
        return ms, frames, kept

    build()                                                                  # warm-up (binds the networks, packs the weights)
    torch.cuda.synchronize()
    t = time.perf_counter()
    grid = build()
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t) * 1e3
    out = {"size": H, "samples": a.samples, "chunk": a.chunk, "netchunk": a.netchunk, "near": a.near, "far": a.far, "poses": len(poses),
           "grid": {"bounds": a.bounds, "resolution": list(res), "dilate": a.dilate, "occupied_fraction": round(grid.fraction, 6),
                    "source": f"sphere r = {a.sphere} at {a.sphere_centre}" if a.sphere is not None else f"networks, threshold {a.threshold}",
                    "build_ms": round(build_ms, 2)}}
    if a.compare:
        ms, plain, _ = arm()
        out["unculled"] = {"frame_ms_median": round(statistics.median(ms), 2), "frame_ms": [round(v, 2) for v in ms]}
    ms, culled, kept = arm(occupancy=grid)
    out["culled"] = {"frame_ms_median": round(statistics.median(ms), 2), "frame_ms": [round(v, 2) for v in ms],
                     "kept_fraction": {k: round(v[0] / v[1], 6) if v[1] else None for k, v in kept.items()}}
    if a.compare:
        out["max_abs_d_rgb"] = max(float((c[0] - p[0]).abs().max()) for c, p in zip(culled, plain))
        out["max_abs_d_acc"] = max(float((c[1] - p[1]).abs().max()) for c, p in zip(culled, plain))
        out["speedup"] = round(out["unculled"]["frame_ms_median"] / out["culled"]["frame_ms_median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Render one view's geometry — depth, silhouette (acc) and disparity — with ``Renderer.render_geometry`` (density half of the networks
only) and the same view in full with ``render_fitting``; prints ONE JSON line: the frame time of the geometry render and of the full
render with the sigma gate as shipped and off (``MOFA_GATE=0``), each the median of ``--frames`` frames after ``--warmup`` frames,
whether the outputs the two renders share (disp, acc, disp0, acc0, z_std) are bit-identical, and the density half's share of the fine
network's dense FLOPs from ``mofa_net_layer_dims``.  Writes ``depth.npy``, ``acc.npy``, ``disp.npy`` and ``mask.png`` (acc through
``mesh.to8b``) into ``--out``.

``--surface median|expected`` adds a fourth arm, timed right after the geometry arm in the same process: the geometry render with its
surface buffers on (``normals=True``: median depth, points, normals).  It writes ``normals.png`` (``valid * (n + 1) / 2``),
``depth_median.npy`` and ``points.npy`` as well, and the line carries the arm's times, its ratio to the plain geometry arm, the share of
pixels with a valid normal and whether the buffers both arms share are bit-identical.

Networks come from a checkpoint (``--ckpt DIR`` or one ``.tar``) or from seeded synthetic weights (``--synthetic DC WC DF WF``); codes
from ``--fit saving_Parameters.tar`` or ``synth.codes`` — the options of tools/render_culled.py.  Seeded weights say nothing about a
trained face's live fraction: the gated full render's time depends on it, the other two arms do not.

  python tools/render_geometry.py --synthetic 8 256 10 1024 --size 512 --out geometry_out
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import lib, mesh  # noqa: E402
from mofanerf_amd import synth  # noqa: E402
from mofanerf_amd.rays import pose_spherical  # noqa: E402
from render_culled import load  # noqa: E402


def flop_share(h):
    """(density half, whole network) multiply-adds per sample from the plan's layer sizes: the point layers, the shape stack and the alpha
    head against every layer (the texture stack, the view layer and the rgb head are the rest)."""
    L = lib.load()
    no, ni = C.c_int32(), C.c_int32()
    sizes = []
    for li in range(L.mofa_net_num_layers(h.shape)):
        lib.check(L.mofa_net_layer_dims(h.shape, li, C.byref(no), C.byref(ni)), "mofa_net_layer_dims")
        sizes.append(no.value * ni.value)
    D = h.D
    geometry = sum(sizes[:4 + D]) + sizes[2 * D + 5]      # 4 point layers, D shape layers; layers 4 + 2 D .. : view, alpha head, rgb head
    return geometry, sum(sizes)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint directory (the newest *.tar is used) or one .tar file")
    src.add_argument("--synthetic", type=int, nargs=4, metavar=("DC", "WC", "DF", "WF"), help="seeded synthetic coarse / fine networks")
    ap.add_argument("--fit", help="saving_Parameters.tar of run_fit.py (shape / texture / expression codes); default synth.codes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--size", type=int, default=512, help="frame height = width")
    ap.add_argument("--samples", type=int, nargs=2, default=[64, 128], metavar=("N_SAMPLES", "N_IMPORTANCE"))
    ap.add_argument("--near", type=float, default=8.0)
    ap.add_argument("--far", type=float, default=26.0)
    ap.add_argument("--chunk", type=int, default=196608)
    ap.add_argument("--netchunk", type=int, default=196608)
    ap.add_argument("--angle", type=float, default=25.0, help="azimuth of the view in degrees (radius 16)")
    ap.add_argument("--frames", type=int, default=5, help="timed frames per arm (the median is reported)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="geometry_out", help="directory for depth.npy, acc.npy, disp.npy and mask.png")
    ap.add_argument("--surface", choices=("median", "expected"), help="also time and write the surface buffers (normals, points, median depth)")
    ap.add_argument("--acc-min", type=float, default=0.5, help="--surface: a pixel takes part in the normals iff acc >= this")
    ap.add_argument("--median-threshold", type=float, default=0.5, help="--surface: the accumulated weight the median depth is taken at")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    render, kw, bm, uv, exp = load(a, dev)
    H = a.size
    K = synth.intrinsics(H, H)
    pose = pose_spherical(a.angle, 0.0, 16.0)[:3, :4]
    kw = dict(kw, near=a.near, far=a.far)

    def geometry():
        out = render.render_geometry(H, H, K, chunk=a.chunk, c2w=pose, shapeCodes=bm, expType=20, expCodes=exp, **kw)
        render.check_launches(block=True)
        torch.cuda.synchronize()
        return out

    def surface():
        out = render.render_geometry(H, H, K, chunk=a.chunk, c2w=pose, shapeCodes=bm, expType=20, expCodes=exp, median=True, normals=True,
                                     surface=a.surface, acc_min=a.acc_min, median_threshold=a.median_threshold, **kw)
        render.check_launches(block=True)
        torch.cuda.synchronize()
        return out

    def full():
        with torch.no_grad():
            out = render.render_fitting(H, H, K, chunk=a.chunk, c2w=pose, shapeCodes=bm, uvCodes=uv, expType=20, expCodes=exp, **kw)
        render.check_launches(block=True)
        torch.cuda.synchronize()
        return out

    def arm(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(max(a.frames, 1)):
            t = time.perf_counter()
            out = fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return {"frame_ms_median": round(statistics.median(ms), 2), "frame_ms": [round(v, 2) for v in ms]}, out

    keep = os.environ.get("MOFA_GATE")
    t_geo, g = arm(geometry)
    if a.surface:
        t_surf, gs = arm(surface)
    os.environ["MOFA_GATE"] = "0"
    lib.reload_env()
    try:
        t_plain, f = arm(full)
    finally:
        if keep is None:
            del os.environ["MOFA_GATE"]
        else:
            os.environ["MOFA_GATE"] = keep
        lib.reload_env()
    t_gated, f_gated = arm(full)
    bits = lambda t: t.contiguous().view(torch.int32)
    shared = {"disp": (g[1], f[1]), "acc": (g[2], f[2])}
    shared.update({k: (g[3][k], f[3][k]) for k in ("disp0", "acc0", "z_std") if k in g[3]})
    identical = {k: bool(torch.equal(bits(x), bits(y))) for k, (x, y) in shared.items()}
    identical["gated_full_frame"] = all(bool(torch.equal(bits(x), bits(y))) for x, y in zip(f[:3], f_gated[:3]))
    geo_flops, all_flops = flop_share(render._hip(kw["network_fine"] if kw.get("network_fine") is not None else kw["network_fn"]))
    os.makedirs(a.out, exist_ok=True)
    depth, disp, acc = (t.cpu().numpy() for t in g[:3])
    for name, arr in (("depth", depth), ("acc", acc), ("disp", disp)):
        np.save(os.path.join(a.out, name + ".npy"), arr)
    from mofanerf_amd.io import write_png
    write_png(os.path.join(a.out, "mask.png"), np.repeat(mesh.to8b(acc)[..., None], 3, -1))
    extra = {}
    if a.surface:
        identical["surface_frame"] = (all(bool(torch.equal(bits(x), bits(y))) for x, y in zip(g[:3], gs[:3])) and
                                      all(bool(torch.equal(bits(g[3][k]), bits(gs[3][k]))) for k in g[3]))
        normals, valid = gs[3]["normals"].cpu().numpy(), gs[3]["normals_valid"].cpu().numpy()
        np.save(os.path.join(a.out, "depth_median.npy"), gs[3]["depth_median"].cpu().numpy())
        np.save(os.path.join(a.out, "points.npy"), gs[3]["points"].cpu().numpy())
        write_png(os.path.join(a.out, "normals.png"), mesh.to8b(valid[..., None] * (normals + 1.0) / 2.0))
        extra = {"surface": a.surface, "acc_min": a.acc_min, "median_threshold": a.median_threshold, "geometry_surface": t_surf,
                 "surface_over_geometry": round(t_surf["frame_ms_median"] / t_geo["frame_ms_median"], 4),
                 "normals_valid_share": round(float(valid.mean()), 4), "usable_share": round(float((acc >= a.acc_min).mean()), 4),
                 "median_found_share": round(float((gs[3]["median_index"] >= 0).float().mean()), 4)}
        print(f"valid normals: {100 * extra['normals_valid_share']:.2f} % of {H * H} pixels", file=sys.stderr)
    print(json.dumps({"size": H, "samples": a.samples, "chunk": a.chunk, "netchunk": a.netchunk, "near": a.near, "far": a.far, "angle": a.angle,
                      "geometry": t_geo, "full_ungated": t_plain, "full_gated": t_gated,
                      "geometry_over_full_ungated": round(t_geo["frame_ms_median"] / t_plain["frame_ms_median"], 4),
                      "geometry_over_full_gated": round(t_geo["frame_ms_median"] / t_gated["frame_ms_median"], 4),
                      "bit_identical": identical, "fine_density_flop_share": round(geo_flops / all_flops, 4),
                      "acc_mean": float(acc.mean()), "out": a.out, **extra}))
    return 0 if all(identical.values()) else 1


if __name__ == "__main__":
    sys.exit(main())

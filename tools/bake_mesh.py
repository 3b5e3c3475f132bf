#!/usr/bin/env python3
"""Vertex colours for a mesh with ANY triangulation, from the renderer's own frames: a ring of poses is rendered with
``render_fitting(ndc=False)``, every frame is projected onto the vertices as soon as it is rendered (``Renderer.bake_mesh``:
``mesh.rasterize`` of the mesh itself gives the visibility depth, ``mesh.vertex_normals`` the angle weights, ``mesh.bake_integrate`` /
``bake_colors`` / ``fill_colors`` do the rest), and the coloured PLY is written.

The mesh comes from a PLY (``--ply``: an extraction, or a template that was warped, simplified or smoothed — anything ``mesh.read_ply``
reads) or, without one, from ``extract_mesh(level=--level)`` on ``--bounds`` / ``--resolution``.  Networks come from a checkpoint
(``--ckpt``) or seeded synthetic weights (``--synthetic DC WC DF WF``), codes from ``--fit`` or ``synth.codes`` — the options of
tools/fuse_mesh.py.  ``--depth-tol`` is required: no depth tolerance of a trained model has been measured.

  python tools/bake_mesh.py --synthetic 8 256 10 1024 --bounds -4 -4 -4 4 4 4 --resolution 129 129 129 --level 0 --depth-tol 0.1 \
      --views 8 --size 512 --out baked.ply

``--compare-network`` also evaluates the network AT the vertices as ``extract_mesh(colors=True)`` does (one evaluation per vertex, looking
along minus the vertex normal, no compositing) and prints the difference to the baked colours over the coloured vertices.  ``--time N``
repeats the kernels alone N times on the last frame (HIP events) and prints the medians, with the bytes a vertex and view move.  ON SEEDED
WEIGHTS NONE OF THE COLOURS OR COUNTS SAYS ANYTHING ABOUT A TRAINED FACE: a seeded network's density is noise and its mesh a sponge; only
the times carry over.  Prints one JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import mesh, synth  # noqa: E402
from fuse_mesh import ring, timed  # noqa: E402
from render_culled import load  # noqa: E402


def network_colors(render, net, verts, faces, bm, uv, exp, netchunk):
    """``extract_mesh(colors=True)``'s colours at given vertices: sigmoid(raw[..., :3]) of one evaluation per vertex, looking along minus
    the area-weighted vertex normal."""
    with torch.no_grad():
        render._set_codes(bm, 20, exp)
        vd = (-mesh.vertex_normals(verts, faces)).contiguous()
        render.decoding_texCodes = uv
        keep, render.netchunk = render.netchunk, int(netchunk)
        try:
            raw = render.run_network(verts[:, None, :], vd, net)
        finally:
            render.netchunk = keep
        render.check_launches(block=True)
        return torch.sigmoid(raw[:, 0, :3])


def event_ms(fn, repeat):
    """Median, minimum and maximum HIP-event time of ``fn`` over ``repeat`` calls after two warm-up calls."""
    for _ in range(2):
        fn()
    times = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times)), float(max(times))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint directory (the newest *.tar is used) or one .tar file")
    src.add_argument("--synthetic", type=int, nargs=4, metavar=("DC", "WC", "DF", "WF"), help="seeded synthetic coarse / fine networks")
    ap.add_argument("--fit", help="saving_Parameters.tar of run_fit.py (shape / texture / expression codes); default synth.codes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ply", help="the mesh to colour (binary PLY of mesh.write_ply); without it: extract_mesh on --bounds / --resolution / --level")
    ap.add_argument("--bounds", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--resolution", type=int, nargs=3, default=[129, 129, 129], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--level", type=float, help="iso-level of the extraction (no default: none has been measured)")
    ap.add_argument("--depth-tol", type=float, required=True, help="how far behind the rasterised depth a vertex may lie and still count as "
                    "visible, in scene units (no default: none has been measured)")
    ap.add_argument("--cos-min", type=float, default=0.0, help="views at a cosine to the vertex normal not above this are rejected (untuned)")
    ap.add_argument("--power", type=int, default=2, help="a view weighs cos^power (0 .. 8; untuned)")
    ap.add_argument("--blend", choices=("mean", "best"), default="mean")
    ap.add_argument("--fill", type=int, default=0, metavar="N", help="Jacobi steps of hole filling over the vertex adjacency")
    ap.add_argument("--views", type=int, default=8, help="poses of the ring")
    ap.add_argument("--elevations", type=float, nargs="+", default=[-20.0, 15.0], help="elevations in degrees, taken in turn around the ring")
    ap.add_argument("--radius", type=float, default=16.0, help="distance of the cameras from the origin")
    ap.add_argument("--size", type=int, default=512, help="frame height = width")
    ap.add_argument("--compare-network", action="store_true", help="print the difference to extract_mesh(colors=True)-style colours")
    ap.add_argument("--time", type=int, default=0, metavar="N", help="also time the kernels alone, N repetitions each (HIP events)")
    ap.add_argument("--samples", type=int, nargs=2, default=[64, 128], metavar=("N_SAMPLES", "N_IMPORTANCE"))
    ap.add_argument("--near", type=float, default=8.0)
    ap.add_argument("--far", type=float, default=26.0)
    ap.add_argument("--chunk", type=int, default=196608)
    ap.add_argument("--netchunk", type=int, default=196608)
    ap.add_argument("--out", default="baked.ply")
    a = ap.parse_args(argv)
    if a.ply is None and (a.bounds is None or a.level is None):
        ap.error("without --ply the mesh is extracted: --bounds and --level are required")
    dev = torch.device("cuda", torch.cuda.current_device())
    render, kw, bm, uv, exp = load(a, dev)
    net = kw["network_fine"] if kw.get("network_fine") is not None else kw["network_fn"]
    H = a.size
    K = synth.intrinsics(H, H)
    poses = ring(a.views, a.elevations, a.radius)
    kw = {k: v for k, v in dict(kw, near=a.near, far=a.far).items() if k != "ndc"}
    if a.synthetic:
        print("seeded synthetic weights: the colours and counts below say NOTHING about a trained face (only the times carry over)", flush=True)
    out = {"views": a.views, "size": H, "depth_tol": a.depth_tol, "cos_min": a.cos_min, "power": a.power, "blend": a.blend,
           "synthetic_weights": bool(a.synthetic)}
    if a.ply:
        t, ply = timed(lambda: mesh.read_ply(a.ply))
        verts, faces = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in ply[:2])
        print(f"read {a.ply}: V = {verts.shape[0]}, F = {faces.shape[0]} ({t:.1f} ms)", flush=True)
        out["source"] = a.ply
    else:
        bounds = (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
        t, (verts, faces) = timed(lambda: tuple(x.contiguous() for x in render.extract_mesh(
            net, bounds=bounds, resolution=tuple(a.resolution), level=a.level, shapeCodes=bm, expType=20, expCodes=exp, netchunk=a.netchunk)[:2]))
        print(f"extract_mesh(level={a.level:g}): V = {verts.shape[0]}, F = {faces.shape[0]} in {t:.1f} ms", flush=True)
        out["source"] = f"extract_mesh(level={a.level:g}) at {a.resolution}"
    V = int(verts.shape[0])
    if not V or not faces.shape[0]:
        sys.exit("the mesh is empty: nothing to colour")
    codes = dict(shapeCodes=bm, uvCodes=uv, expType=20, expCodes=exp)
    t_all, (colors, valid, stats) = timed(lambda: render.bake_mesh(poses, H, H, K, verts, faces, depth_tol=a.depth_tol, blend=a.blend,
                                                                   cos_min=a.cos_min, power=a.power, fill_iterations=a.fill, chunk=a.chunk,
                                                                   **codes, **kw))
    tm = {k: round(1e3 * t, 3) for k, t in stats.pop("times").items()}
    print(f"baked {a.views} frames of {H} x {H} onto {V} vertices in {t_all:.1f} ms: " + ", ".join(f"{k} {x:.2f} ms" for k, x in tm.items())
          + f"; per frame: render {tm['render'] / a.views:.2f}, rasterize {tm['rasterize'] / a.views:.3f}, integrate "
          f"{tm['integrate'] / a.views:.3f} ms", flush=True)
    print(f"  vertices coloured {stats['colored']} ({100.0 * stats['colored'] / V:.1f} %), uncoloured: occluded {stats['occluded']}, grazing "
          f"{stats['grazing']}, unseen {stats['unseen']}; after {a.fill} filling steps {stats['remaining']} remain; the mesh covers "
          f"{min(stats['hit_share']):.3f} .. {max(stats['hit_share']):.3f} of a frame", flush=True)
    out.update(stats, V=V, F=int(faces.shape[0]), times_ms=tm, total_ms=round(t_all, 2))
    if a.time:
        normals = mesh.vertex_normals(verts, faces).contiguous()
        with torch.no_grad():
            rgb = render.render_fitting(H, H, K, chunk=a.chunk, c2w=poses[-1], ndc=False, **codes, **kw)[0].reshape(H, H, 3).contiguous()
        r = mesh.rasterize(verts, faces, H, H, K, poses[-1])
        frame = mesh.depth_frame(r["depth"], r["mask"])
        state = mesh.bake_state(V, 3, dev)
        one = event_ms(lambda: mesh.bake_integrate(state, verts, rgb, frame, K, poses[-1], normals, depth_tol=a.depth_tol, cos_min=a.cos_min,
                                                   power=a.power), a.time)
        n8 = min(8, a.views)
        rgb8, frame8 = rgb[None].expand(n8, H, H, 3).contiguous(), frame[None].expand(n8, H, H).contiguous()
        many = event_ms(lambda: mesh.bake_integrate(state, verts, rgb8, frame8, K, poses[-1], normals, depth_tol=a.depth_tol, cos_min=a.cos_min,
                                                    power=a.power), a.time)
        resolve = event_ms(lambda: mesh.bake_colors(state, a.blend), a.time)
        raster = event_ms(lambda: mesh.rasterize(verts, faces, H, H, K, poses[-1]), a.time)
        with torch.no_grad():
            frame_ms = event_ms(lambda: render.render_fitting(H, H, K, chunk=a.chunk, c2w=poses[-1], ndc=False, **codes, **kw), max(1, min(a.time, 3)))
        render.check_launches(block=True)
        state_bytes = 20 * 3 + 28                                # csum, cbest per channel; wsum, wbest, seen, occluded, grazing
        fixed = 2 * state_bytes + 24                             # the state read and written once per call, verts and normals read once
        gathered = 4 * 4 + 4 * 3 * 4                             # 4 depths and 4 x 3 texels per view that passes every test
        print(f"  kernels alone on {V} vertices (median of {a.time}, min - max): bake_integrate of 1 view {one[0]:.3f} ms ({one[1]:.3f} - "
              f"{one[2]:.3f}), of {n8} views in one call {many[0]:.3f} ms ({many[0] / n8:.3f} per view); bake_colors (with its read-back) "
              f"{resolve[0]:.3f} ms; rasterize {raster[0]:.3f} ms; one render_fitting frame {frame_ms[0]:.1f} ms", flush=True)
        print(f"  bytes per vertex: state {state_bytes} read + {state_bytes} written + 24 of vertex and normal per call, at most {gathered} "
              f"gathered per view: 1 view moves at most {(fixed + gathered) * V / 1e6:.1f} MB -> {(fixed + gathered) * V / one[0] / 1e6:.1f} GB/s; "
              f"{n8} views {(fixed + n8 * gathered) * V / 1e6:.1f} MB -> {(fixed + n8 * gathered) * V / many[0] / 1e6:.1f} GB/s "
              "(an upper estimate: a view that fails a test gathers less)", flush=True)
        out["kernels_ms"] = {"integrate_1_view": one, f"integrate_{n8}_views": many, "bake_colors": resolve, "rasterize": raster,
                             "render_fitting_frame": frame_ms}
    if a.compare_network:
        t, ref = timed(lambda: network_colors(render, net, verts, faces, bm, uv, exp, a.netchunk))
        ok = valid & torch.isfinite(ref).all(-1)
        diff = (colors - ref).abs()[ok]
        if diff.numel():
            print(f"  against the network evaluated at the vertices ({t:.1f} ms): over {int(ok.sum())} valid vertices (baked or filled) mean |difference| "
                  f"{float(diff.mean()):.4f}, 95 % {float(torch.quantile(diff.max(-1).values[:1 << 24], 0.95)):.4f}, max {float(diff.max()):.4f}", flush=True)
            out["compare_network"] = {"vertices": int(ok.sum()), "mean_abs": float(diff.mean()), "max_abs": float(diff.max())}
        else:
            print("  against the network evaluated at the vertices: no coloured vertex to compare", flush=True)
    t, _ = timed(lambda: mesh.write_ply(a.out, verts, faces, colors=colors.clamp(0.0, 1.0)))
    print(f"wrote {a.out}: V = {V}, F = {faces.shape[0]} with colours ({t:.1f} ms)", flush=True)
    out["out"] = a.out
    print(json.dumps(out))


if __name__ == "__main__":
    main()

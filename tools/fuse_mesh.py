#!/usr/bin/env python3
"""A mesh of the face WITHOUT an iso-level: depth frames from a ring of poses are fused into a truncated signed distance volume
(``mesh.tsdf_integrate``) and its zero level is marched (``mesh.tsdf_surface``) — the surface the frames show.

The frames come from the volume renderer (default: ``Renderer.fuse_geometry``, one ``render_geometry(median=True, ndc=False)`` frame per
pose, masked with ``acc >= --acc-min``) or, with ``--from-level L``, from the rasterised mesh of ``extract_mesh(level=L)``
(``mesh.rasterize`` depth through ``mesh.depth_frame``): the way back from any mesh to a clean closed one, and the shape the times in
profiles/mesh_fusion.md were taken at.  Networks come from a checkpoint (``--ckpt``) or seeded synthetic weights (``--synthetic DC WC DF
WF``), codes from ``--fit`` or ``synth.codes`` — the options of tools/render_mesh.py.  ``--bounds``, ``--resolution`` and ``--trunc`` are
required: no box, and no truncation distance, of a trained model has been measured.

  python tools/fuse_mesh.py --synthetic 8 256 10 1024 --bounds -4 -4 -4 4 4 4 --resolution 129 129 129 --trunc 0.25 --views 12 --size 256 \
      --out fused.ply

``--components largest|N``, ``--simplify M`` and ``--smooth N`` post-process the fused mesh through ``mesh.components`` /
``keep_components``, ``mesh.simplify`` and ``mesh.smooth``, in that order, as ``extract_mesh`` does.  ``--compare-level L`` extracts
``extract_mesh(level=L)`` as well and prints ``mesh.surface_distance(signed=True)`` between the fused mesh and it, and
``mesh.depth_agreement`` of both meshes (rasterised from every pose of the ring) against the volume's own frames: the number for choosing
a level.  ON SEEDED WEIGHTS NONE OF THESE NUMBERS SAYS ANYTHING ABOUT A TRAINED FACE: a seeded network's density is noise; only the times
carry over.  Prints one JSON line at the end.
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
from mofanerf_amd.rays import pose_spherical  # noqa: E402
from extract_mesh import components_arg, simplify_arg, smooth_arg  # noqa: E402
from render_culled import load  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def ring(n, elevations, radius):
    """n poses around the head: azimuth -180 + 360 k / n, the elevations taken in turn."""
    return [pose_spherical(-180.0 + 360.0 * k / n, elevations[k % len(elevations)], radius)[:3, :4] for k in range(n)]


def fuse_rasterised(verts, faces, poses, H, K, res, lo, step, a, dev):
    """The mesh rasterised from every pose, encoded and integrated frame by frame; (verts, faces, stats)."""
    state = mesh.tsdf_volume(res, lo, step, a.trunc, dev)
    ms = {"rasterize": 0.0, "integrate": 0.0}
    shares = []
    for pose in poses:
        t, r = timed(lambda: mesh.rasterize(verts, faces, H, H, K, pose, znear=a.znear))
        ms["rasterize"] += t
        t, _ = timed(lambda: mesh.tsdf_integrate(state, mesh.depth_frame(r["depth"], r["mask"], a.background), K, pose))
        ms["integrate"] += t
        shares.append(float(r["mask"].float().mean()))
    ms["field"], (field, stats) = timed(lambda: mesh.tsdf_field(state, a.unobserved, not a.open_border))
    ms["march"], (v, f) = timed(lambda: mesh.iso_surface(field, 0.0, lo, step))
    stats.update(hit_share=shares, times_ms={k: round(x, 3) for k, x in ms.items()})
    return v, f, stats


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint directory (the newest *.tar is used) or one .tar file")
    src.add_argument("--synthetic", type=int, nargs=4, metavar=("DC", "WC", "DF", "WF"), help="seeded synthetic coarse / fine networks")
    ap.add_argument("--fit", help="saving_Parameters.tar of run_fit.py (shape / texture / expression codes); default synth.codes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bounds", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--resolution", type=int, nargs=3, required=True, metavar=("NX", "NY", "NZ"))
    ap.add_argument("--trunc", type=float, required=True, help="truncation distance in scene units (no default: none has been measured)")
    ap.add_argument("--views", type=int, default=24, help="poses of the ring")
    ap.add_argument("--elevations", type=float, nargs="+", default=[-20.0, 15.0], help="elevations in degrees, taken in turn around the ring")
    ap.add_argument("--radius", type=float, default=16.0, help="distance of the cameras from the origin")
    ap.add_argument("--size", type=int, default=512, help="frame height = width")
    ap.add_argument("--from-level", type=float, default=None, metavar="L", help="fuse the rasterised mesh of extract_mesh(level=L) instead of "
                    "rendered frames")
    ap.add_argument("--surface", choices=("median", "expected"), default="median")
    ap.add_argument("--acc-min", type=float, default=0.5, help="a rendered frame's mask: acc >= this")
    ap.add_argument("--background", choices=("empty", "unknown"), default="empty", help="pixels outside the mask carve the volume, or say nothing")
    ap.add_argument("--weight", choices=("acc",), default=None, help="weigh a rendered pixel by acc (1 - acc outside the mask)")
    ap.add_argument("--unobserved", choices=("auto", "outside", "inside"), default="auto")
    ap.add_argument("--open-border", action="store_true", help="do not close the mesh at the volume's border")
    ap.add_argument("--components", type=components_arg, default=None, metavar="largest|N")
    ap.add_argument("--simplify", type=simplify_arg, default=None, metavar="M", help="vertex clustering on cells of M grid steps")
    ap.add_argument("--smooth", type=smooth_arg, default=None, metavar="N", help="Taubin iterations")
    ap.add_argument("--compare-level", type=float, default=None, metavar="L", help="also extract_mesh(level=L): signed surface distance to the "
                    "fused mesh and both meshes' depth agreement with the volume's frames")
    ap.add_argument("--samples", type=int, nargs=2, default=[64, 128], metavar=("N_SAMPLES", "N_IMPORTANCE"))
    ap.add_argument("--near", type=float, default=8.0)
    ap.add_argument("--far", type=float, default=26.0)
    ap.add_argument("--chunk", type=int, default=196608)
    ap.add_argument("--netchunk", type=int, default=196608)
    ap.add_argument("--znear", type=float, default=1e-3)
    ap.add_argument("--out", default="fused.ply")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    render, kw, bm, uv, exp = load(a, dev)
    net = kw["network_fine"] if kw.get("network_fine") is not None else kw["network_fn"]
    H = a.size
    K = synth.intrinsics(H, H)
    poses = ring(a.views, a.elevations, a.radius)
    kw = {k: v for k, v in dict(kw, near=a.near, far=a.far).items() if k != "ndc"}
    bounds = (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
    res, lo, step = mesh.grid_spec(bounds, tuple(a.resolution))
    codes = dict(shapeCodes=bm, expType=20, expCodes=exp)
    if a.synthetic:
        print("seeded synthetic weights: the meshes and distances below say NOTHING about a trained face (only the times carry over)", flush=True)
    extract = lambda level: tuple(t.contiguous() for t in render.extract_mesh(net, bounds=bounds, resolution=res, level=level, netchunk=a.netchunk,
                                                                              **codes)[:2])
    out = {"resolution": list(res), "trunc": a.trunc, "views": a.views, "size": H, "background": a.background, "unobserved": a.unobserved,
           "synthetic_weights": bool(a.synthetic)}
    if a.from_level is not None:
        t_extract, (v0, f0) = timed(lambda: extract(a.from_level))
        print(f"extract_mesh(level={a.from_level:g}): V = {v0.shape[0]}, F = {f0.shape[0]} in {t_extract:.1f} ms", flush=True)
        if not f0.shape[0]:
            sys.exit("the level has no surface in the box: nothing to rasterise")
        verts, faces, stats = fuse_rasterised(v0, f0, poses, H, K, res, lo, step, a, dev)
        out.update(source=f"rasterised extract_mesh(level={a.from_level:g})", source_faces=int(f0.shape[0]))
    else:
        t_all, (verts, faces, stats) = timed(lambda: render.fuse_geometry(
            poses, H, H, K, bounds=bounds, resolution=res, trunc=a.trunc, surface=a.surface, acc_min=a.acc_min, background=a.background,
            weight=a.weight, unobserved=a.unobserved, close_border=not a.open_border, chunk=a.chunk, **codes, **kw))
        stats["times_ms"] = {k: round(1e3 * t, 3) for k, t in stats.pop("times").items()}
        stats["resolution"] = list(stats["resolution"])
        out.update(source=f"render_geometry({a.surface}), acc >= {a.acc_min:g}", total_ms=round(t_all, 2))
    tm = stats["times_ms"]
    n = res[0] * res[1] * res[2]
    print(f"fused {a.views} frames of {H} x {H} into {res[0]} x {res[1]} x {res[2]} ({n} voxels, trunc {a.trunc:g}): "
          + ", ".join(f"{k} {x:.2f} ms" for k, x in tm.items()) + f"; integrate per frame {tm['integrate'] / a.views:.3f} ms", flush=True)
    print(f"  voxels observed {stats['observed']}, filled inside {stats['filled_inside']}, filled outside {stats['filled_outside']}, border "
          f"{stats['border']}; hit share per frame {min(stats['hit_share']):.3f} .. {max(stats['hit_share']):.3f}; V = {verts.shape[0]}, "
          f"F = {faces.shape[0]}", flush=True)
    out.update(stats, V=int(verts.shape[0]), F=int(faces.shape[0]))
    if not faces.shape[0]:
        sys.exit("the fused volume has no surface: nothing to write")
    verts, faces = verts.contiguous(), faces.contiguous()
    if a.components is not None:
        t, cs = timed(lambda: mesh.components(verts, faces))
        keep = mesh.select_components(cs, a.components)
        verts, faces = (x.contiguous() for x in mesh.keep_components(verts, faces, cs, keep)[:2])
        print(f"components={a.components}: kept {int(keep.sum())} of {cs['n_components']} components, {faces.shape[0]} faces ({t:.1f} ms)", flush=True)
        out["components"] = {"n_components": int(cs["n_components"]), "kept": int(keep.sum()), "F": int(faces.shape[0])}
    if a.simplify is not None:
        cell = (np.float32(a.simplify) * np.asarray(step, dtype=np.float32)).astype(np.float32)
        t, (verts, faces, ss) = timed(lambda: mesh.simplify(verts, faces, cell, origin=lo))
        verts, faces = verts.contiguous(), faces.contiguous()
        print(f"simplify={a.simplify}: V = {ss['verts_out']}, F = {ss['faces_out']} ({t:.1f} ms)", flush=True)
        out["simplify"] = {"V": int(ss["verts_out"]), "F": int(ss["faces_out"])}
    if a.smooth is not None:
        t, (verts, sm) = timed(lambda: mesh.smooth(verts, faces, iterations=a.smooth))
        verts = verts.contiguous()
        print(f"smooth={a.smooth}: max displacement {sm['max_displacement']:.5f} ({t:.1f} ms)", flush=True)
        out["smooth"] = {"max_displacement": float(sm["max_displacement"])}
    if a.compare_level is not None:
        lv, lf = extract(a.compare_level)
        spacing = float(min(step))
        print(f"extract_mesh(level={a.compare_level:g}): V = {lv.shape[0]}, F = {lf.shape[0]}")
        cmp = {"level": a.compare_level, "V": int(lv.shape[0]), "F": int(lf.shape[0])}
        if lf.shape[0]:
            try:
                err = mesh.surface_distance(verts, faces, lv, lf, spacing, signed=True)
                e, b = err["a_to_b"], err["b_to_a"]
                cmp["surface_distance"] = {"hausdorff": err["hausdorff"], **{d: {q: err[d][q] for q in (
                    "mean", "max", "p95", "signed_mean", "inside_fraction", "max_inside", "max_outside")} for d in ("a_to_b", "b_to_a")}}
                print(f"  signed surface distance, fused -> level {a.compare_level:g} (negative: the fused sample lies inside the level's mesh): signed "
                      f"mean {e['signed_mean']:.5f}, {100 * e['inside_fraction']:.1f} % inside, mean {e['mean']:.5f}, 95 % {e['p95']:.5f}; level -> "
                      f"fused: signed mean {b['signed_mean']:.5f}, mean {b['mean']:.5f}, 95 % {b['p95']:.5f}; Hausdorff {err['hausdorff']:.5f}", flush=True)
            except mesh.lib.MofaError as ex:                       # an open mesh has no inside
                print(f"  signed surface distance: not available ({ex})", flush=True)
            rows = {"fused": [], "level": []}
            for pose in poses:
                _, _, acc, ex = render.render_geometry(H, H, K, chunk=a.chunk, c2w=pose, ndc=False, median=True, acc_min=a.acc_min, **codes, **kw)
                for name, (mv, mf) in (("fused", (verts, faces)), ("level", (lv, lf))):
                    r = mesh.rasterize(mv, mf, H, H, K, pose, znear=a.znear)
                    rows[name].append(mesh.depth_agreement(r["depth"], r["mask"], ex["depth_median"], acc, a.acc_min))
            render.check_launches(block=True)
            for name, rs in rows.items():
                iou = float(np.mean([r["iou"] for r in rs]))
                med = float(np.nanmean([r["median_abs"] for r in rs])) if any(r["n_both"] for r in rs) else float("nan")
                cmp[f"depth_agreement_{name}"] = {"mean_iou": iou, "mean_median_abs": med}
                print(f"  depth agreement with the volume's {len(rs)} frames, {name:5s} mesh: mean IoU {iou:.4f}, mean of the median |depth "
                      f"difference| {med:.5f}", flush=True)
        out["compare"] = cmp
    t, _ = timed(lambda: mesh.write_ply(a.out, verts, faces))
    print(f"wrote {a.out}: V = {verts.shape[0]}, F = {faces.shape[0]} ({t:.1f} ms)", flush=True)
    out.update(out=a.out, V_written=int(verts.shape[0]), F_written=int(faces.shape[0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

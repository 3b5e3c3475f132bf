#!/usr/bin/env python3
"""Measure iso-levels: extract the face's mesh at one or several density levels (``Renderer.extract_mesh``), rasterise each from a pose
(``Renderer.render_mesh``, the GPU z-buffer of ``mesh.rasterize``), render the volume's own surface from the same pose ONCE
(``Renderer.render_geometry(median=True, ndc=False)``) and print, per level, how well the two agree (``mesh.depth_agreement``: mask IoU,
pixel counts, median and 95th-percentile |depth difference| on the overlap) next to the time of each stage.  The rasterised depth and the
volume's depth are the same quantity: the ray parameter of the pixel's ``get_rays`` ray.

Writes ``level_<level>_mesh.png`` (head-light shade) and ``level_<level>_mesh_depth.png`` per level and ``volume_depth.png`` into
``--out``; prints one JSON line at the end.  ``--refine K`` extracts every level a second time with its vertices moved onto the level by
K bisection steps along their lattice edges (``extract_mesh(refine=K)``) and prints the agreement without and with: the difference is
what the linear vertex placement contributed to the first number.  ``--components largest|N`` is passed to ``extract_mesh``: floaters
are removed before the mesh is rasterised, so a level's agreement can be read with and without them.  ``--simplify M`` extracts every
level once more with ``extract_mesh(simplify=M)`` (vertex clustering on cells of M grid steps, quadric-error representatives), rasterises
it from the same pose and prints its agreement with the volume next to the unsimplified mesh's, and the agreement of the simplified mesh
with the unsimplified one (the unsimplified mesh's mask standing in as ``acc`` with ``acc_min`` 0.5): what the simplification cost in depth
from this one camera.  Next to it the surface distance between the two meshes (``mesh.surface_distance``: all of the surface, both ways).
``--smooth N`` does the same with ``extract_mesh(smooth=N)`` (Taubin smoothing, ``--smooth-weights uniform|cotangent``): the depth agreement
with and without smoothing, and ``mesh.surface_distance(signed=True)`` between the two meshes — which way the surface moved, and how far
(a mesh that is open at the box has no inside: the tool then says so instead).
``--ray-cast`` casts the frame's own ``get_rays`` rays against every mesh (``mesh.ray_cast``, first hit) and prints, against the rasterised
frame of the same pose: the share of pixels with the same mask, the median / 95 % / largest |depth difference| on the pixels both hit, the
share of those with the same face index, and the times of both.  ``--mesh-bounds MARGIN`` additionally renders the volume once more with
the mesh's per-ray bounds (``Renderer.mesh_bounds``: first and last hit +- MARGIN) and prints ``mesh.depth_agreement`` of the scalar-bounds
render and of the mesh-bounds render against the rasterised mesh, and the share of the ``[near, far]`` span the bounds remove.

Networks come from a checkpoint (``--ckpt``) or seeded synthetic weights (``--synthetic DC WC DF WF``), codes from ``--fit`` or
``synth.codes`` — the options of tools/render_geometry.py.  ON SEEDED WEIGHTS THE AGREEMENT NUMBERS MEAN NOTHING ABOUT A TRAINED FACE:
a seeded network's density is noise, and the tool says so in its output; the stage times do not depend on the weights' values.

  python tools/render_mesh.py --synthetic 8 256 10 1024 --bounds -4 -4 -4 4 4 4 --resolution 129 129 129 --levels 0,0.5,1 --size 512
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import mesh, synth  # noqa: E402
from mofanerf_amd.io import PngSink  # noqa: E402
from mofanerf_amd.rays import get_rays, pose_spherical  # noqa: E402
from extract_mesh import components_arg, simplify_arg, smooth_arg  # noqa: E402
from render_culled import load  # noqa: E402


def median_ms(fn, warmup, frames):
    """(median ms, every ms, the last result) of ``fn`` after ``warmup`` calls; each call ends with a device synchronisation."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms, out = [], None
    for _ in range(max(frames, 1)):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ms), 3), [round(v, 3) for v in ms], out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint directory (the newest *.tar is used) or one .tar file")
    src.add_argument("--synthetic", type=int, nargs=4, metavar=("DC", "WC", "DF", "WF"), help="seeded synthetic coarse / fine networks")
    ap.add_argument("--fit", help="saving_Parameters.tar of run_fit.py (shape / texture / expression codes); default synth.codes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bounds", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--resolution", type=int, nargs=3, default=[129, 129, 129], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--brick", type=int, default=None, help="narrow-band extraction with bricks of B^3 cells (4, 8 or 16)")
    lv = ap.add_mutually_exclusive_group(required=True)
    lv.add_argument("--level", type=float, help="one iso-level of the pre-ReLU density (no default: none has been measured)")
    lv.add_argument("--levels", help="several, comma-separated: a,b,c")
    ap.add_argument("--refine", type=int, default=0, metavar="K", help="also extract every level with its vertices moved onto the level by K "
                    "bisection steps along their edges (extract_mesh(refine=K)); the agreement is printed without and with")
    ap.add_argument("--components", type=components_arg, default=None, metavar="largest|N", help="remove floaters before rasterising: "
                    "extract_mesh(components=...) keeps the component with the most faces, or every one with at least N faces")
    ap.add_argument("--simplify", type=simplify_arg, default=None, metavar="M", help="also extract every level simplified on cells of M grid "
                    "steps (extract_mesh(simplify=M)); its agreement with the volume and with the unsimplified mesh is printed")
    ap.add_argument("--smooth", type=smooth_arg, default=None, metavar="N", help="also extract every level smoothed by N Taubin iterations "
                    "(extract_mesh(smooth=N)); its agreement with the volume and the signed distance to the unsmoothed mesh are printed")
    ap.add_argument("--smooth-weights", choices=("uniform", "cotangent"), default="uniform", help="with --smooth: the Laplacian's weights")
    ap.add_argument("--ray-cast", action="store_true", help="also cast the frame's rays against every mesh (mesh.ray_cast) and print its agreement "
                    "with the rasterised frame and the times of both")
    ap.add_argument("--mesh-bounds", type=float, default=None, metavar="MARGIN", help="also render the volume with the mesh's per-ray bounds "
                    "(Renderer.mesh_bounds, first / last hit +- MARGIN) and print both renders' agreement with the rasterised mesh")
    ap.add_argument("--size", type=int, default=512, help="frame height = width")
    ap.add_argument("--samples", type=int, nargs=2, default=[64, 128], metavar=("N_SAMPLES", "N_IMPORTANCE"))
    ap.add_argument("--near", type=float, default=8.0)
    ap.add_argument("--far", type=float, default=26.0)
    ap.add_argument("--chunk", type=int, default=196608)
    ap.add_argument("--netchunk", type=int, default=196608)
    ap.add_argument("--angle", type=float, default=25.0, help="azimuth of the view in degrees")
    ap.add_argument("--radius", type=float, default=16.0, help="distance of the camera from the origin")
    ap.add_argument("--acc-min", type=float, default=0.5, help="the volume's mask: acc >= this")
    ap.add_argument("--median-threshold", type=float, default=0.5, help="the accumulated weight the volume's median depth is taken at")
    ap.add_argument("--znear", type=float, default=1e-3)
    ap.add_argument("--frames", type=int, default=5, help="timed frames per stage (the median is reported)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="mesh_out")
    a = ap.parse_args(argv)
    levels = [a.level] if a.levels is None else [float(v) for v in a.levels.split(",") if v.strip()]
    dev = torch.device("cuda", torch.cuda.current_device())
    render, kw, bm, uv, exp = load(a, dev)
    net = kw["network_fine"] if kw.get("network_fine") is not None else kw["network_fn"]
    H = a.size
    K = synth.intrinsics(H, H)
    pose = pose_spherical(a.angle, 0.0, a.radius)[:3, :4]
    kw = {k: v for k, v in dict(kw, near=a.near, far=a.far).items() if k != "ndc"}
    bounds = (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
    if a.synthetic:
        print("seeded synthetic weights: the agreement numbers below say NOTHING about a trained face (only the times carry over)", flush=True)

    def volume(**bounds_):
        out = render.render_geometry(H, H, K, chunk=a.chunk, c2w=pose, ndc=False, shapeCodes=bm, expType=20, expCodes=exp, median=True,
                                     acc_min=a.acc_min, median_threshold=a.median_threshold, **dict(kw, **bounds_))
        render.check_launches(block=True)
        return out

    t_vol, all_vol, (_, _, acc, ex) = median_ms(volume, a.warmup, a.frames)
    depth_vol = ex["depth_median"]
    print(f"volume: render_geometry(median=True) {H} x {H}, {a.samples[0]} + {a.samples[1]} samples: {t_vol:.2f} ms per frame "
          f"(median of {len(all_vol)}), {int((acc >= a.acc_min).sum())} pixels with acc >= {a.acc_min}", flush=True)
    os.makedirs(a.out, exist_ok=True)
    span = torch.full_like(depth_vol, a.far - a.near)
    rows = []
    with PngSink() as sink:
        sink.submit(os.path.join(a.out, "volume_depth.png"), (((depth_vol - a.near) / span) * (acc >= a.acc_min))[..., None].expand(H, H, 3))
        for level in levels:
            for k in ((0, a.refine) if a.refine else (0,)):       # with --refine: the plain mesh, then the refined one
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                verts, faces = render.extract_mesh(net, bounds=bounds, resolution=tuple(a.resolution), level=level, shapeCodes=bm, expType=20,
                                                   expCodes=exp, netchunk=a.netchunk, brick=a.brick, refine=k, components=a.components)[:2]
                torch.cuda.synchronize()
                t_extract = (time.perf_counter() - t0) * 1e3
                t_mesh, all_mesh, (rgb, depth, mask, mex) = median_ms(
                    lambda: render.render_mesh(H, H, K, pose, verts, faces, znear=a.znear), a.warmup, a.frames)
                t_raster, _, _ = median_ms(lambda: mesh.rasterize(verts, faces, H, H, K, pose, znear=a.znear), a.warmup, a.frames)
                agree = mesh.depth_agreement(depth, mask, depth_vol, acc, a.acc_min)
                drawn, culled, degenerate, wave = (int(v) for v in mex["counts"].cpu())
                if a.components is not None:
                    cs = render.mesh_stats["components"]
                    print(f"  components={a.components}: kept {int(cs['kept'].sum())} of {cs['n_components']} components, "
                          f"{int(faces.shape[0])} of {int(cs['n_faces'].sum())} faces ({cs['passes']} passes)", flush=True)
                row = {"level": level, "refine": k, "V": int(verts.shape[0]), "F": int(faces.shape[0]), "extract_ms": round(t_extract, 2), "render_mesh_ms": t_mesh,
                       "render_mesh_ms_all": all_mesh, "rasterize_ms": t_raster, "faces_drawn": drawn, "faces_culled": culled,
                       "faces_degenerate": degenerate, "faces_wave_path": wave, **agree}
                rows.append(row)
                print(f"level {level:g}{f' refined by {k} bisection steps' if k else ''}: V = {row['V']}, F = {row['F']} (culled {culled}, degenerate {degenerate}, wavefront path {wave}); extract "
                      f"{t_extract:.1f} ms, render_mesh {t_mesh:.3f} ms (rasterize alone {t_raster:.3f} ms) against the volume's {t_vol:.1f} ms; "
                      f"IoU {agree['iou']:.4f} (mesh {agree['n_mesh']}, volume {agree['n_vol']}, both {agree['n_both']}), |depth difference| median "
                      f"{agree['median_abs']:.5f}, 95 % {agree['p95_abs']:.5f}", flush=True)
                if culled:
                    print(f"  {culled} faces were culled whole (a vertex nearer than znear or outside the guard band): there is no near-plane clipping")
                stem = os.path.join(a.out, f"level_{level:g}" + (f"_refine{k}" if k else ""))
                sink.submit(stem + "_mesh.png", rgb)
                sink.submit(stem + "_mesh_depth.png", (((depth - a.near) / span) * mask)[..., None].expand(H, H, 3))
                if a.ray_cast or a.mesh_bounds is not None:
                    # the frame's own rays against the mesh: the rasteriser's pixels are these rays snapped to 1 / 256 pixel
                    ro, rd = (x.reshape(-1, 3).contiguous() for x in get_rays(H, H, K, pose, device=verts.device))
                    vc, fc = verts.contiguous(), faces.contiguous()
                    t_cast, _, cast = median_ms(lambda: mesh.ray_cast(ro, rd, vc, fc), a.warmup, a.frames)
                    rmask, rdepth, rface = cast["hit"].reshape(H, H), cast["t"].reshape(H, H), cast["face"].reshape(H, H)
                    both = rmask & mask
                    dd = (rdepth - depth)[both].abs().double()
                    q = lambda v: float(torch.quantile(dd, v)) if dd.numel() else float("nan")
                    row["ray_cast"] = {"ray_cast_ms": t_cast, "rasterize_ms": t_raster, "grid": list(cast["grid"]), "counts": cast["counts"],
                                       "same_mask": float((rmask == mask).double().mean()), "n_cast": int(rmask.sum()), "n_raster": int(mask.sum()),
                                       "n_both": int(both.sum()), "median_abs": q(0.5), "p95_abs": q(0.95),
                                       "max_abs": float(dd.max()) if dd.numel() else float("nan"),
                                       "same_face": float((rface[both] == mex["face"][both]).double().mean()) if dd.numel() else float("nan")}
                    rc = row["ray_cast"]
                    print(f"  ray_cast ({H * H} rays, grid {tuple(cast['grid'])}, {cast['counts']['face_tests'] / (H * H):.1f} face tests per ray): "
                          f"{t_cast:.3f} ms against rasterize's {t_raster:.3f} ms; same mask on {100 * rc['same_mask']:.3f} % of the pixels (cast "
                          f"{rc['n_cast']}, rasterised {rc['n_raster']}, both {rc['n_both']}), |depth difference| median {rc['median_abs']:.2e}, 95 % "
                          f"{rc['p95_abs']:.2e}, max {rc['max_abs']:.2e}; the same face on {100 * rc['same_face']:.3f} % of them", flush=True)
                    if a.mesh_bounds is not None:
                        t_b, _, (bn, bf, bhit) = median_ms(lambda: render.mesh_bounds(H, H, K, pose, vc, fc, a.near, a.far, a.mesh_bounds), a.warmup,
                                                           a.frames)
                        t_bvol, _, (_, _, bacc, bex) = median_ms(lambda: volume(near=bn, far=bf), a.warmup, a.frames)
                        scalar = mesh.depth_agreement(depth, mask, depth_vol, acc, a.acc_min)
                        hugged = mesh.depth_agreement(depth, mask, bex["depth_median"], bacc, a.acc_min)
                        removed = 1.0 - float(((bf - bn) / (a.far - a.near)).double().mean())
                        row["mesh_bounds"] = {"margin": a.mesh_bounds, "mesh_bounds_ms": t_b, "render_geometry_ms": t_bvol, "rays_hit": int(bhit.sum()),
                                              "span_removed": removed, "scalar_bounds": scalar, "mesh_bounds": hugged}
                        print(f"  mesh_bounds (margin {a.mesh_bounds:g}): {t_b:.3f} ms, {int(bhit.sum())} of {H * H} rays hit, {100 * removed:.1f} % of the "
                              f"[near, far] span removed; render_geometry with them {t_bvol:.2f} ms (scalar bounds {t_vol:.2f} ms)")
                        for label, g in (("scalar bounds", scalar), ("mesh bounds  ", hugged)):
                            print(f"    {label} against the rasterised mesh: IoU {g['iou']:.4f}, |depth difference| median {g['median_abs']:.5f}, 95 % "
                                  f"{g['p95_abs']:.5f}", flush=True)
                if a.smooth is not None:
                    # the same mesh smoothed, from the same pose: against the volume, against the unsmoothed mesh, and which way it moved
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    mv, mf = render.extract_mesh(net, bounds=bounds, resolution=tuple(a.resolution), level=level, shapeCodes=bm, expType=20,
                                                 expCodes=exp, netchunk=a.netchunk, brick=a.brick, refine=k, components=a.components,
                                                 smooth=a.smooth, smooth_weights=a.smooth_weights)[:2]
                    torch.cuda.synchronize()
                    t_smooth = (time.perf_counter() - t0) * 1e3
                    ms = {key: val for key, val in render.mesh_stats["smooth"].items() if key != "displacement"}
                    t_mmesh, _, (mrgb, mdepth, mmask, _) = median_ms(lambda: render.render_mesh(H, H, K, pose, mv, mf, znear=a.znear), a.warmup, a.frames)
                    m_vol = mesh.depth_agreement(mdepth, mmask, depth_vol, acc, a.acc_min)
                    m_full = mesh.depth_agreement(mdepth, mmask, depth, mask.to(torch.float32), 0.5)
                    row["smoothed"] = {"smooth": a.smooth, "weights": a.smooth_weights, "extract_ms": round(t_smooth, 2), "render_mesh_ms": t_mmesh, **ms,
                                       "against_volume": m_vol, "against_unsmoothed": m_full}
                    print(f"  smooth={a.smooth} ({a.smooth_weights} weights): {ms['passes']} passes, {ms['n_pinned']} of {int(mv.shape[0])} vertices pinned, "
                          f"max displacement {ms['max_displacement']:.5f}; extract + smooth {t_smooth:.1f} ms, render_mesh {t_mmesh:.3f} ms", flush=True)
                    print(f"    against the volume:     IoU {m_vol['iou']:.4f} (unsmoothed {agree['iou']:.4f}), |depth difference| median "
                          f"{m_vol['median_abs']:.5f} (unsmoothed {agree['median_abs']:.5f}), 95 % {m_vol['p95_abs']:.5f} (unsmoothed {agree['p95_abs']:.5f})")
                    print(f"    against the unsmoothed mesh: IoU {m_full['iou']:.4f}, |depth difference| median {m_full['median_abs']:.5f}, "
                          f"95 % {m_full['p95_abs']:.5f}", flush=True)
                    try:
                        spacing = float(min(mesh.grid_spec(bounds, tuple(a.resolution))[2]))
                        err = mesh.surface_distance(verts.contiguous(), faces.contiguous(), mv.contiguous(), mf.contiguous(), spacing, signed=True)
                        row["smoothed"]["surface_distance"] = {"hausdorff": err["hausdorff"], **{d: {q: err[d][q] for q in (
                            "mean", "max", "p95", "signed_mean", "inside_fraction", "max_inside", "max_outside")} for d in ("a_to_b", "b_to_a")}}
                        e = err["a_to_b"]
                        print(f"    signed surface distance, unsmoothed -> smoothed (negative: the sample lies inside the smoothed mesh, which moved "
                              f"outward there): signed mean {e['signed_mean']:.5f}, {100 * e['inside_fraction']:.1f} % inside, largest inside "
                              f"{e['max_inside']:.5f}, outside {e['max_outside']:.5f}; unsigned mean {e['mean']:.5f}, Hausdorff {err['hausdorff']:.5f}"
                              + ("  (seeded weights: nothing about a trained face)" if a.synthetic else ""), flush=True)
                    except mesh.lib.MofaError as ex:                      # an open mesh has no inside (a surface that leaves the box)
                        print(f"    signed surface distance: not available ({ex})", flush=True)
                    sink.submit(stem + f"_smooth{a.smooth}_mesh.png", mrgb)
                if a.simplify is None:
                    continue
                # the same mesh simplified, from the same pose: against the volume, and against the unsimplified mesh
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sv, sf = render.extract_mesh(net, bounds=bounds, resolution=tuple(a.resolution), level=level, shapeCodes=bm, expType=20,
                                             expCodes=exp, netchunk=a.netchunk, brick=a.brick, refine=k, components=a.components,
                                             simplify=a.simplify, simplify_error=True)[:2]
                torch.cuda.synchronize()
                t_simp = (time.perf_counter() - t0) * 1e3
                err = render.mesh_stats["simplify_error"]
                ss = {key: val for key, val in render.mesh_stats["simplify"].items() if key != "cluster_of"}
                t_smesh, _, (srgb, sdepth, smask, _) = median_ms(lambda: render.render_mesh(H, H, K, pose, sv, sf, znear=a.znear), a.warmup, a.frames)
                s_vol = mesh.depth_agreement(sdepth, smask, depth_vol, acc, a.acc_min)
                s_full = mesh.depth_agreement(sdepth, smask, depth, mask.to(torch.float32), 0.5)
                row["simplified"] = {"simplify": a.simplify, "extract_ms": round(t_simp, 2), "render_mesh_ms": t_smesh, **ss,
                                     "against_volume": s_vol, "against_unsimplified": s_full,
                                     "surface_distance": {"hausdorff": err["hausdorff"], "chamfer": err["chamfer"],
                                                          **{d: {q: err[d][q] for q in ("mean", "rms", "max", "p50", "p95", "n_samples")}
                                                             for d in ("a_to_b", "b_to_a")}}}
                print(f"  simplify={a.simplify}: V = {ss['verts_out']}, F = {ss['faces_out']} ({ss['faces_in'] / max(ss['faces_out'], 1):.1f}x fewer faces; "
                      f"placed {ss['placed_quadric']} quadric / {ss['placed_mean']} mean / {ss['placed_first']} first vertex, {ss['edges_multiple']} "
                      f"directed edges used twice); extract + simplify {t_simp:.1f} ms, render_mesh {t_smesh:.3f} ms", flush=True)
                print(f"    against the volume:      IoU {s_vol['iou']:.4f} (unsimplified {agree['iou']:.4f}), |depth difference| median "
                      f"{s_vol['median_abs']:.5f} (unsimplified {agree['median_abs']:.5f}), 95 % {s_vol['p95_abs']:.5f} (unsimplified {agree['p95_abs']:.5f})")
                print(f"    against the unsimplified mesh: IoU {s_full['iou']:.4f}, |depth difference| median {s_full['median_abs']:.5f}, "
                      f"95 % {s_full['p95_abs']:.5f}", flush=True)
                print(f"    surface distance (mesh.surface_distance, all of the surface, both ways; included in the {t_simp:.1f} ms): unsimplified -> "
                      f"simplified mean {err['a_to_b']['mean']:.5f}, 95 % {err['a_to_b']['p95']:.5f}, max {err['a_to_b']['max']:.5f}; simplified -> "
                      f"unsimplified mean {err['b_to_a']['mean']:.5f}, 95 % {err['b_to_a']['p95']:.5f}, max {err['b_to_a']['max']:.5f}; Hausdorff "
                      f"{err['hausdorff']:.5f}" + ("  (seeded weights: nothing about a trained face)" if a.synthetic else ""), flush=True)
                sink.submit(stem + f"_simplify{a.simplify}_mesh.png", srgb)
    print(json.dumps({"size": H, "samples": a.samples, "angle": a.angle, "radius": a.radius, "near": a.near, "far": a.far, "acc_min": a.acc_min,
                      "median_threshold": a.median_threshold, "resolution": a.resolution, "brick": a.brick, "refine": a.refine, "components": a.components,
                      "simplify": a.simplify, "smooth": a.smooth, "ray_cast": a.ray_cast, "mesh_bounds": a.mesh_bounds, "wave_min_pixels": mesh.WAVE_MIN_PIXELS, "synthetic_weights": bool(a.synthetic),
                      "agreement_says_nothing_about_a_trained_face": bool(a.synthetic), "render_geometry_ms": t_vol,
                      "render_geometry_ms_all": all_vol, "levels": rows, "out": a.out}))


if __name__ == "__main__":
    main()

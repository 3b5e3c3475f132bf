#!/usr/bin/env python3
"""A texture image for a mesh with a UV layout, from the renderer's own frames: a ring of poses is rendered with
``render_fitting(ndc=False)`` and every frame is projected onto the surface points of the texels as soon as it is rendered
(``Renderer.bake_texture``: ``mesh.texel_map`` / ``texel_surface`` / ``bake_integrate`` / ``texture_image``); OBJ + MTL + PNG are written.

The mesh comes from an OBJ with UVs (``--obj``), or from a PLY (``--ply``) or an extraction (``--bounds`` / ``--resolution`` /
``--level``, optionally ``--simplify STEPS`` grid steps per cluster) with ``--atlas SIZE``: the per-triangle atlas of ``mesh.face_atlas``
at ``SIZE x SIZE`` texels.  Networks come from a checkpoint (``--ckpt``) or seeded synthetic weights (``--synthetic DC WC DF WF``), codes
from ``--fit`` or ``synth.codes`` — the options of tools/bake_mesh.py.  ``--depth-tol`` is required: none has been measured.

  python tools/bake_texture.py --synthetic 8 256 10 1024 --bounds -4 -4 -4 4 4 4 --resolution 129 129 129 --level 0 --simplify 4 \
      --atlas 2048 --depth-tol 0.1 --views 8 --size 512 --out baked.obj

It prints the counts, the stage times and the error of a held-out pose's ``render_mesh(texture=...)`` against its ``render_fitting`` frame
on the mesh's mask; ``--compare-vertex`` prints the same for ``bake_mesh`` colours; ``--encode`` runs ``texEncoder`` on a 512 x 512
result and prints the distance of its code from ``uvCodes``; ``--time N`` repeats the kernels alone N times (HIP events, medians).  ON
SEEDED WEIGHTS NONE OF THE COLOURS, COUNTS, ERRORS OR CODE DISTANCES SAYS ANYTHING ABOUT A TRAINED FACE: a seeded network's density is
noise and its mesh a sponge; only the times carry over.  Prints one JSON line at the end.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import mesh, synth  # noqa: E402
from mofanerf_amd.rays import pose_spherical  # noqa: E402
from bake_mesh import event_ms  # noqa: E402
from fuse_mesh import ring, timed  # noqa: E402
from render_culled import load  # noqa: E402


def view_error(rgb, frame, mask):
    """mean |rgb - frame| over the pixels of ``mask`` (NaN when it is empty)."""
    return float((rgb - frame).abs()[mask].mean()) if bool(mask.any()) else float("nan")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint directory (the newest *.tar is used) or one .tar file")
    src.add_argument("--synthetic", type=int, nargs=4, metavar=("DC", "WC", "DF", "WF"), help="seeded synthetic coarse / fine networks")
    ap.add_argument("--fit", help="saving_Parameters.tar of run_fit.py (shape / texture / expression codes); default synth.codes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--obj", help="the mesh and its UV layout (Wavefront OBJ with vt)")
    ap.add_argument("--ply", help="a mesh without UVs (binary PLY of mesh.write_ply); needs --atlas")
    ap.add_argument("--bounds", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--resolution", type=int, nargs=3, default=[129, 129, 129], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--level", type=float, help="iso-level of the extraction (no default: none has been measured)")
    ap.add_argument("--simplify", type=float, default=0.0, metavar="STEPS", help="cluster the extraction's vertices in cells of STEPS grid steps")
    ap.add_argument("--atlas", type=int, metavar="SIZE", help="give a mesh without UVs mesh.face_atlas at SIZE x SIZE texels (also the texture's size)")
    ap.add_argument("--texture-size", type=int, default=512, help="texture height = width for --obj (512 is what texEncoder takes)")
    ap.add_argument("--padding", type=float, default=1.0, help="face_atlas' inset in texels")
    ap.add_argument("--dilate", type=int, default=8, help="gutter-filling steps")
    ap.add_argument("--depth-tol", type=float, required=True, help="how far behind the rasterised depth a texel's point may lie and still count "
                    "as visible, in scene units (no default: none has been measured)")
    ap.add_argument("--cos-min", type=float, default=0.0)
    ap.add_argument("--power", type=int, default=2)
    ap.add_argument("--blend", choices=("mean", "best"), default="mean")
    ap.add_argument("--views", type=int, default=8, help="poses of the ring")
    ap.add_argument("--elevations", type=float, nargs="+", default=[-20.0, 15.0])
    ap.add_argument("--radius", type=float, default=16.0)
    ap.add_argument("--size", type=int, default=512, help="frame height = width")
    ap.add_argument("--compare-vertex", action="store_true", help="print the held-out error of bake_mesh's vertex colours too")
    ap.add_argument("--encode", action="store_true", help="run texEncoder on the 512 x 512 result and print its code's distance from uvCodes")
    ap.add_argument("--time", type=int, default=0, metavar="N", help="also time the kernels alone, N repetitions each (HIP events)")
    ap.add_argument("--samples", type=int, nargs=2, default=[64, 128], metavar=("N_SAMPLES", "N_IMPORTANCE"))
    ap.add_argument("--near", type=float, default=8.0)
    ap.add_argument("--far", type=float, default=26.0)
    ap.add_argument("--chunk", type=int, default=196608)
    ap.add_argument("--netchunk", type=int, default=196608)
    ap.add_argument("--out", default="baked.obj")
    a = ap.parse_args(argv)
    if a.obj is None and a.atlas is None:
        ap.error("a mesh without UVs (--ply or an extraction) needs --atlas SIZE")
    if a.obj is None and a.ply is None and (a.bounds is None or a.level is None):
        ap.error("without --obj or --ply the mesh is extracted: --bounds and --level are required")
    dev = torch.device("cuda", torch.cuda.current_device())
    render, kw, bm, uv, exp = load(a, dev)
    net = kw["network_fine"] if kw.get("network_fine") is not None else kw["network_fn"]
    H = a.size
    K = synth.intrinsics(H, H)
    poses = ring(a.views, a.elevations, a.radius)
    held_out = pose_spherical(-180.0 + 180.0 / a.views, float(np.mean(a.elevations)), a.radius)[:3, :4]      # halfway between two of the ring
    kw = {k: v for k, v in dict(kw, near=a.near, far=a.far).items() if k != "ndc"}
    if a.synthetic:
        print("seeded synthetic weights: the colours, counts, errors and code distances below say NOTHING about a trained face (only the "
              "times carry over)", flush=True)
    out = {"views": a.views, "size": H, "depth_tol": a.depth_tol, "cos_min": a.cos_min, "power": a.power, "blend": a.blend,
           "synthetic_weights": bool(a.synthetic)}
    to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    uvs = uv_faces = None
    if a.obj:
        obj = mesh.read_obj(a.obj)
        if obj["uvs"] is None and a.atlas is None:
            sys.exit(f"{a.obj} has no vt: give --atlas SIZE")
        verts, faces = to_dev(obj["verts"]), to_dev(obj["faces"])
        if obj["uvs"] is not None and a.atlas is None:
            uvs, uv_faces = to_dev(obj["uvs"]), to_dev(obj["uv_faces"])
        out["source"] = a.obj
    elif a.ply:
        verts, faces = (to_dev(x) for x in mesh.read_ply(a.ply)[:2])
        out["source"] = a.ply
    else:
        bounds = (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
        t, (verts, faces) = timed(lambda: tuple(x.contiguous() for x in render.extract_mesh(
            net, bounds=bounds, resolution=tuple(a.resolution), level=a.level, shapeCodes=bm, expType=20, expCodes=exp, netchunk=a.netchunk)[:2]))
        print(f"extract_mesh(level={a.level:g}): V = {verts.shape[0]}, F = {faces.shape[0]} in {t:.1f} ms", flush=True)
        out["source"] = f"extract_mesh(level={a.level:g}) at {a.resolution}"
        if a.simplify > 0 and faces.shape[0]:
            _, _, step = mesh.grid_spec(bounds, tuple(a.resolution))
            t, (verts, faces, _) = timed(lambda: mesh.simplify(verts, faces, cell=float(a.simplify * np.max(step))))
            verts, faces = verts.contiguous(), faces.contiguous()
            print(f"simplify({a.simplify:g} grid steps): V = {verts.shape[0]}, F = {faces.shape[0]} in {t:.1f} ms", flush=True)
            out["source"] += f", simplified at {a.simplify:g} grid steps"
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if not V or not F:
        sys.exit("the mesh is empty: nothing to texture")
    size = a.texture_size
    if uvs is None:
        size = a.atlas
        t, (atlas_uvs, atlas_faces, info) = timed(lambda: mesh.face_atlas(F, size, a.padding))
        uvs, uv_faces = to_dev(atlas_uvs), to_dev(atlas_faces)
        print(f"face_atlas: {F} faces in {info['n']} x {info['n']} cells of {info['cell'][0]:.2f} texels at {size} x {size} ({t:.1f} ms)", flush=True)
        out["atlas"] = {"n": info["n"], "cell": info["cell"][0], "padding": a.padding}
    print(f"mesh: V = {V}, F = {F}, T = {uvs.shape[0]}; texture {size} x {size}", flush=True)
    codes = dict(shapeCodes=bm, uvCodes=uv, expType=20, expCodes=exp)
    normals = mesh.vertex_normals(verts, faces).contiguous()
    t_all, (texture, valid, stats) = timed(lambda: render.bake_texture(
        poses, H, H, K, verts, faces, uvs, uv_faces, size=size, depth_tol=a.depth_tol, blend=a.blend, cos_min=a.cos_min, power=a.power,
        dilate=a.dilate, normals=normals, chunk=a.chunk, **codes, **kw))
    tm = {k: round(1e3 * t, 3) for k, t in stats.pop("times").items()}
    M = stats["covered"]
    print(f"baked {a.views} frames of {H} x {H} onto {M} texels in {t_all:.1f} ms: " + ", ".join(f"{k} {x:.2f} ms" for k, x in tm.items()), flush=True)
    print(f"  texels covered {M} of {size * size} ({100.0 * M / (size * size):.1f} %), in two charts {stats['multi']}; UV faces without area "
          f"{stats['degenerate']}, faces without a texel {stats['faces_without_texels']}; coloured {stats['colored']} "
          f"({100.0 * stats['colored'] / max(M, 1):.1f} % of the covered), uncoloured: occluded {stats['occluded']}, grazing {stats['grazing']}, unseen "
          f"{stats['unseen']}; after {a.dilate} dilation steps {stats['remaining']} texels remain invalid", flush=True)
    out.update({k: v for k, v in stats.items() if k != "size"}, V=V, F=F, T=int(uvs.shape[0]), texture_size=size, times_ms=tm, total_ms=round(t_all, 2))
    with torch.no_grad():
        frame = render.render_fitting(H, H, K, chunk=a.chunk, c2w=held_out, ndc=False, **codes, **kw)[0].reshape(H, H, 3)
    rgb, _, mask, _ = render.render_mesh(H, H, K, held_out, verts, faces, texture=texture, uvs=uvs, uv_faces=uv_faces)
    out["held_out_texture_mean_abs"] = view_error(rgb, frame, mask)
    print(f"  held-out pose, render_mesh(texture=...) against its render_fitting frame on the mesh's mask ({int(mask.sum())} pixels): mean "
          f"|error| {out['held_out_texture_mean_abs']:.4f}", flush=True)
    if a.compare_vertex:
        colors, _, vstats = render.bake_mesh(poses, H, H, K, verts, faces, depth_tol=a.depth_tol, blend=a.blend, cos_min=a.cos_min, power=a.power,
                                             fill_iterations=a.dilate, normals=normals, chunk=a.chunk, **codes, **kw)
        rgb_v = render.render_mesh(H, H, K, held_out, verts, faces, colors=colors)[0]
        out["held_out_vertex_mean_abs"] = view_error(rgb_v, frame, mask)
        print(f"  the same for bake_mesh's vertex colours ({vstats['colored']} of {V} vertices coloured): mean |error| "
              f"{out['held_out_vertex_mean_abs']:.4f}", flush=True)
    if a.encode:
        if size != 512:
            print(f"  --encode: texEncoder takes 512 x 512, the texture is {size} x {size}: skipped", flush=True)
        else:
            with torch.no_grad():
                code = render.texEncoder(texture.clamp(0.0, 1.0).permute([2, 0, 1]).unsqueeze(0), None)[0].reshape(-1)
            dist = float((code - uv.reshape(-1).to(code)).norm())
            out["code_distance"], out["code_norm"] = dist, float(uv.norm())
            print(f"  texEncoder(texture): |code - uvCodes| = {dist:.4f} (|uvCodes| = {float(uv.norm()):.4f})", flush=True)
    if a.time:
        sizes = sorted({512, 2048, size})
        maps = {}
        for s in sizes:
            if uv_faces.shape[0] == F and (a.obj and a.atlas is None):
                s_uvs, s_faces = uvs, uv_faces
            else:
                try:
                    s_uvs, s_faces = (to_dev(x) for x in mesh.face_atlas(F, s, a.padding)[:2])
                except Exception as e:                               # the atlas does not fit this size
                    print(f"  texel_map at {s} x {s}: {e}", flush=True)
                    continue
            maps[s] = event_ms(lambda: mesh.texel_map(s_uvs, s_faces, s), a.time)
        tmap = render.bake_map
        points, pn = mesh.texel_surface(tmap, verts, faces, normals)
        surface = event_ms(lambda: mesh.texel_surface(tmap, verts, faces, normals), a.time)
        with torch.no_grad():
            rgb1 = render.render_fitting(H, H, K, chunk=a.chunk, c2w=poses[-1], ndc=False, **codes, **kw)[0].reshape(H, H, 3).contiguous()
        r = mesh.rasterize(verts, faces, H, H, K, poses[-1])
        depth = mesh.depth_frame(r["depth"], r["mask"])
        state = mesh.texture_state(tmap)
        bake = dict(depth_tol=a.depth_tol, cos_min=a.cos_min, power=a.power)
        one = event_ms(lambda: mesh.bake_integrate(state, points, rgb1, depth, K, poses[-1], pn, **bake), a.time)
        rgb8, depth8 = rgb1[None].expand(8, H, H, 3).contiguous(), depth[None].expand(8, H, H).contiguous()
        many = event_ms(lambda: mesh.bake_integrate(state, points, rgb8, depth8, K, poses[-1], pn, **bake), a.time)
        image = event_ms(lambda: mesh.texture_image(state, tmap, a.blend, 0.0, 8), a.time)
        rb = mesh.rasterize(verts, faces, 512, 512, synth.intrinsics(512, 512), held_out, bary=True)
        sample = event_ms(lambda: mesh.sample_texture(texture, rb["face"], rb["bary"], uvs, uv_faces), a.time)
        raster = event_ms(lambda: mesh.rasterize(verts, faces, H, H, K, poses[-1]), a.time)
        with torch.no_grad():
            frame_ms = event_ms(lambda: render.render_fitting(H, H, K, chunk=a.chunk, c2w=poses[-1], ndc=False, **codes, **kw), max(1, min(a.time, 3)))
        render.check_launches(block=True)
        print(f"  calls alone (median of {a.time} ms, with their host reads): " + ", ".join(f"texel_map {s}^2 {t[0]:.3f}" for s, t in maps.items())
              + f"; texel_surface of {M} texels {surface[0]:.3f}; bake_integrate of 1 view {one[0]:.3f}, of 8 views in one call {many[0]:.3f} "
              f"({many[0] / 8:.3f} per view); texture_image(dilate=8) {image[0]:.3f}; sample_texture at 512^2 {sample[0]:.3f}; rasterize {raster[0]:.3f}; "
              f"one render_fitting frame {frame_ms[0]:.1f}", flush=True)
        out["calls_ms"] = dict({f"texel_map_{s}": t for s, t in maps.items()}, texel_surface=surface, integrate_1_view=one, integrate_8_views=many,
                               texture_image_dilate8=image, sample_texture_512=sample, rasterize=raster, render_fitting_frame=frame_ms)
    t, _ = timed(lambda: mesh.write_obj(a.out, verts, faces, uvs, uv_faces, texture=texture.clamp(0.0, 1.0)))
    print(f"wrote {a.out} with its .mtl and .png: V = {V}, F = {F}, T = {uvs.shape[0]}, texture {size} x {size} ({t:.1f} ms)", flush=True)
    out["out"] = a.out
    print(json.dumps(out))


if __name__ == "__main__":
    main()

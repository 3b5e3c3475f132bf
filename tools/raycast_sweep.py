#!/usr/bin/env python3
"""Time the mesh ray casting (``mesh.ray_cast``) on an extraction of seeded weights: the ``--size``^2 rays of one ``get_rays`` frame against
the extracted mesh A and against B = ``mesh.simplify(A, --simplify cells)``, at the default grid and at every resolution of ``--grids``,
for first and last hits; a small ray set against B at ``grid=1`` (brute force through the same kernel) for scale; ``mesh.ray_bounds``; and
``mesh.rasterize`` of the same pose, in the same run, as context.  Every call is timed on the host after a warm-up call and ends with a
device synchronisation (the best of ``--repeats`` is stated); a call includes the two validations with their host reads, the binning and
its sort, the sort of the rays and the kernel.  Every grid must give the same bytes; the tool exits non-zero otherwise.  Prints markdown
tables and one JSON line (profiles/mesh_raycast.md keeps them).

  python tools/raycast_sweep.py --synthetic 8 256 10 1024 --bounds -4 -4 -4 4 4 4 --resolution 129 129 129 --level 0
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import mesh, synth  # noqa: E402
from mofanerf_amd.rays import get_rays, pose_spherical  # noqa: E402
from render_culled import load  # noqa: E402


def best_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms, out = [], None
    for _ in range(max(repeats, 1)):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return round(min(ms), 3), out


def bits(r):
    return torch.cat([r["t64"].view(torch.int64).reshape(-1), r["face"].reshape(-1).long(), r["front"].reshape(-1).long(),
                      r["bary"].view(torch.int32).reshape(-1).long(), r["point"].view(torch.int32).reshape(-1).long()])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint directory (the newest *.tar is used) or one .tar file")
    src.add_argument("--synthetic", type=int, nargs=4, metavar=("DC", "WC", "DF", "WF"), help="seeded synthetic coarse / fine networks")
    ap.add_argument("--fit", help="saving_Parameters.tar of run_fit.py; default synth.codes")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bounds", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--resolution", type=int, nargs=3, default=[129, 129, 129], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--level", type=float, required=True)
    ap.add_argument("--simplify", type=float, default=4.0, help="B's clustering cell in grid steps")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--grids", default="8,16,32,64,128,256")
    ap.add_argument("--small", type=int, default=4099, help="rays of the brute-force run (grid=1, against B)")
    ap.add_argument("--samples", type=int, nargs=2, default=[64, 128])
    ap.add_argument("--netchunk", type=int, default=196608)
    ap.add_argument("--angle", type=float, default=25.0)
    ap.add_argument("--radius", type=float, default=16.0)
    ap.add_argument("--near", type=float, default=8.0)
    ap.add_argument("--far", type=float, default=26.0)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    render, kw, bm, uv, exp = load(a, dev)
    net = kw["network_fine"] if kw.get("network_fine") is not None else kw["network_fn"]
    bounds = (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
    va, fa = render.extract_mesh(net, bounds=bounds, resolution=tuple(a.resolution), level=a.level, shapeCodes=bm, expType=20, expCodes=exp,
                                 netchunk=a.netchunk)[:2]
    va, fa = va.contiguous(), fa.contiguous()
    _, lo, step = mesh.grid_spec(bounds, tuple(a.resolution))
    vb, fb, _ = mesh.simplify(va, fa, a.simplify * float(min(step)), origin=lo)
    vb, fb = vb.contiguous(), fb.contiguous()
    H = a.size
    K = synth.intrinsics(H, H)
    pose = pose_spherical(a.angle, 0.0, a.radius)[:3, :4]
    ro, rd = (x.reshape(-1, 3).contiguous() for x in get_rays(H, H, K, pose, device=dev))
    grids = [None] + [int(g) for g in a.grids.split(",") if g.strip()]
    rows, same = [], True
    for name, (v, f) in (("A", (va, fa)), ("B", (vb, fb))):
        t_raster, _ = best_ms(lambda: mesh.rasterize(v, f, H, H, K, pose), a.repeats)
        rows.append({"mesh": name, "V": int(v.shape[0]), "F": int(f.shape[0]), "call": "rasterize", "ms": t_raster})
        for which in ("first", "last"):
            base = None
            for g in grids:
                if g is not None and g > mesh.DIST_GRID_CAP:
                    continue
                try:
                    ms, r = best_ms(lambda: mesh.ray_cast(ro, rd, v, f, which=which, grid=g), a.repeats)
                except mesh.lib.MofaError as ex:                      # more than 2^31 - 1 pairs at this resolution
                    rows.append({"mesh": name, "call": f"ray_cast {which}", "grid": g, "refused": str(ex)[:120]})
                    continue
                b = bits(r)
                base = b if base is None else base
                same = same and bool(torch.equal(b, base))
                rows.append({"mesh": name, "F": int(f.shape[0]), "call": f"ray_cast {which}", "grid": list(r["grid"]), "default": g is None, "ms": ms,
                             "hit": int(r["hit"].sum()), "face_tests_per_ray": round(r["counts"]["face_tests"] / (H * H), 2),
                             "max_slabs": r["counts"]["max_slabs"], "off_box": r["counts"]["off_box"]})
                del r, b
        ms, r = best_ms(lambda: mesh.ray_bounds(ro, rd, v, f, a.near, a.far, 0.25), a.repeats)
        rows.append({"mesh": name, "call": "ray_bounds (margin 0.25)", "grid": list(r["grid"]), "ms": ms, "hit": int(r["hit"].sum()),
                     "span_removed": round(1.0 - float(((r["far"] - r["near"]) / (a.far - a.near)).double().mean()), 4)})
    pick = torch.linspace(0, H * H - 1, a.small, device=dev).long()
    so, sd = ro[pick].contiguous(), rd[pick].contiguous()
    ms1, r1 = best_ms(lambda: mesh.ray_cast(so, sd, vb, fb, grid=1), 1)
    msd, rdft = best_ms(lambda: mesh.ray_cast(so, sd, vb, fb), a.repeats)
    same = same and bool(torch.equal(bits(r1), bits(rdft)))
    for label, ms, r in (("grid=1", ms1, r1), ("default", msd, rdft)):
        rows.append({"mesh": "B", "call": f"ray_cast first, {a.small} rays, {label}", "grid": list(r["grid"]), "ms": ms, "hit": int(r["hit"].sum()),
                     "face_tests_per_ray": round(r["counts"]["face_tests"] / a.small, 2)})
    print("| mesh | call | grid | ms | rays that hit | face tests per ray | most slabs |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['mesh']} | {r['call']} | {'x'.join(str(g) for g in r['grid']) if r.get('grid') else ''}{' (default)' if r.get('default') else ''} | "
              f"{r.get('ms', r.get('refused', ''))} | {r.get('hit', '')} | {r.get('face_tests_per_ray', '')} | {r.get('max_slabs', '')} |")
    print(json.dumps({"size": H, "resolution": a.resolution, "level": a.level, "synthetic_weights": bool(a.synthetic), "bit_identical": same,
                      "meshes": {"A": [int(va.shape[0]), int(fa.shape[0])], "B": [int(vb.shape[0]), int(fb.shape[0])]}, "rows": rows}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

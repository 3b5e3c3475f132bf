#!/usr/bin/env python3
"""Sweep ``wave_min_pixels`` of the mesh rasteriser (``mesh.rasterize``) on the two workloads that pull it in opposite directions, at
``--size``^2: a marching-tetrahedra ball on a ``--grid``^3 lattice (sub-pixel faces: the one-lane-per-face path) and a 12-face box that
fills the frame (the one-wavefront-per-face path).  Per value: the frame time in microseconds between two events on the stream (median,
least and greatest of ``--frames`` frames after a warm-up) and the share of drawn faces on the wavefront path.  Every value must give the
same bits; the tool exits non-zero otherwise.  Prints a markdown table and one JSON line (profiles/mesh_raster.md keeps the table).

  python tools/raster_sweep.py --size 512 --grid 257
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import mesh  # noqa: E402
from mofanerf_amd.rays import pose_spherical  # noqa: E402


def ball_mesh(n, dev):
    res, lo, step = mesh.grid_spec(((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)), (n, n, n))
    pts = torch.empty(n ** 3, 3, dtype=torch.float32, device=dev)
    mesh.grid_points(res, lo, step, 0, n ** 3, pts)
    c = torch.tensor((0.1, -0.05, 0.2), dtype=torch.float32, device=dev)
    grid = (1.0 - ((pts - c) ** 2).sum(-1)).reshape(res).contiguous()
    del pts
    return mesh.iso_surface(grid, 0.0, lo, step)


def box_mesh(dev):
    v = torch.tensor([[x, y, z] for x in (-1., 1.) for y in (-1., 1.) for z in (-1., 1.)], dtype=torch.float32, device=dev)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = torch.tensor([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=torch.int32, device=dev)
    return v, f


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--grid", type=int, default=257)
    ap.add_argument("--values", default="0,16,64,256,1024,2147483647")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    H = a.size
    K = np.array([[1.1 * H, 0, H / 2], [0, 1.1 * H, H / 2], [0, 0, 1]], np.float32)
    loads = {"ball": (*ball_mesh(a.grid, dev), pose_spherical(25.0, -20.0, 4.0)[:3, :4]),
             "box": (*box_mesh(dev), pose_spherical(25.0, -20.0, 2.2)[:3, :4])}
    values = [int(v) for v in a.values.split(",")]
    rows, same = [], True
    for name, (verts, faces, pose) in loads.items():
        base = None
        for wmp in values:
            def frame():
                return mesh.rasterize(verts, faces, H, H, K, pose, normals=True, wave_min_pixels=wmp)
            for _ in range(a.warmup):
                out = frame()
            us = []
            for _ in range(a.frames):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = frame()
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            bits = torch.cat([out["depth"].view(torch.int32).reshape(-1), out["face"].reshape(-1), out["normal"].view(torch.int32).reshape(-1)])
            if base is None:
                base = bits
            same = same and bool(torch.equal(bits, base))
            drawn, culled, degenerate, wave = (int(v) for v in out["counts"].cpu())
            rows.append({"workload": name, "faces": int(faces.shape[0]), "wave_min_pixels": wmp, "us_median": round(statistics.median(us), 1),
                         "us_min": round(min(us), 1), "us_max": round(max(us), 1), "drawn": drawn, "culled": culled, "degenerate": degenerate,
                         "wave_path": wave, "covered": int(out["mask"].sum())})
    print("| workload | faces | wave_min_pixels | median us | least | greatest | drawn | wavefront path | covered pixels |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['workload']} | {r['faces']} | {r['wave_min_pixels']} | {r['us_median']} | {r['us_min']} | {r['us_max']} | {r['drawn']} | "
              f"{r['wave_path']} | {r['covered']} |")
    print(json.dumps({"size": H, "grid": a.grid, "frames": a.frames, "bit_identical": same, "rows": rows}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

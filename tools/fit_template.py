#!/usr/bin/env python3
"""Warp a template mesh onto a target mesh on the GPU without changing the template's topology (``mesh.warp``: non-rigid registration by
stiffness-regularised closest points with one translation per vertex) — meshes with triangulations of their own come out in
the template's vertex numbering.

  python tools/fit_template.py TEMPLATE.ply TARGET.ply --out WARPED.ply [--align rigid|similarity] [--handles FILE.npy]
                               [--stiffness a,b,c] [--iterations N] [--metric plane|point] [--max-distance D] [--spacing S]
                               [--stiffness-model displacement|arap]

``--align`` first registers the template onto the target (``mesh.register_meshes``): the stiffness acts on displacements and penalises a
rotation like a bend, so a template that is not in the target's frame should be aligned first.  ``--handles`` is a ``numpy.save`` file of
rows ``index, x, y, z[, weight]`` (weight 1 where the column is missing): landmark vertices of the template and where they belong.
``--stiffness-model arap`` replaces the stiffness on displacements by the as-rigid-as-possible one (a rotation per vertex): a
rotation of the template is then free and the edge lengths are kept; the tool then also prints ``arap_energy`` per iteration.
``--stiffness`` is the schedule, stiffest first (default 10,1,0.1), ``--iterations`` the closest-point iterations per level (default 5).
The tool prints the history of every iteration, the time per iteration split into query, system and solve, the rms relative change of
the template's edge lengths and the surface distance (``mesh.surface_distance``, template -> target and back) before and after, and writes the warped template with the template's faces.
Meshes extracted from seeded synthetic weights are noise: what the warp does on a trained face or a real scan has not been measured."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import mesh  # noqa: E402


def report(name, d):
    print(f"{name}: template -> target rms {d['a_to_b']['rms']:.6g} (max {d['a_to_b']['max']:.6g}), target -> template rms "
          f"{d['b_to_a']['rms']:.6g} (max {d['b_to_a']['max']:.6g}), chamfer {d['chamfer']:.6g}")


def edge_change(before, after, faces):
    """The rms relative change of the edge lengths (every face side counted once per face; degenerate sides left out)."""
    f = faces.long()
    ends = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    l0, l1 = ((v.double()[ends[:, 0]] - v.double()[ends[:, 1]]).norm(dim=1) for v in (before, after))
    ok = l0 > 0
    return float(torch.sqrt((((l1[ok] - l0[ok]) / l0[ok]) ** 2).mean())) if bool(ok.any()) else float("nan")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("template")
    ap.add_argument("target")
    ap.add_argument("--out", required=True, metavar="WARPED.ply")
    ap.add_argument("--align", choices=("rigid", "similarity"), default=None, help="register the template onto the target first")
    ap.add_argument("--handles", default=None, metavar="FILE.npy", help="rows index, x, y, z[, weight]")
    ap.add_argument("--stiffness", default="10,1,0.1", help="the schedule, stiffest first (default 10,1,0.1)")
    ap.add_argument("--iterations", type=int, default=5, help="closest-point iterations per level (default 5)")
    ap.add_argument("--metric", choices=("plane", "point"), default="plane")
    ap.add_argument("--stiffness-model", choices=("displacement", "arap"), default="displacement",
                    help="what the stiffness penalises: differences of displacements (default) or deviations from a rotation per vertex")
    ap.add_argument("--max-distance", type=float, default=None, help="bound of the closest-point search (default: unbounded)")
    ap.add_argument("--spacing", type=float, default=None, help="quadrature spacing of the distances (default: 1/256 of the larger box diagonal)")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    meshes = []
    for path in (a.template, a.target):
        rec = mesh.read_ply(path)
        v, f = torch.from_numpy(np.ascontiguousarray(rec[0])).to(dev), torch.from_numpy(np.ascontiguousarray(rec[1])).to(dev)
        print(f"{path}: V = {v.shape[0]}, F = {f.shape[0]}")
        meshes.append((v, f))
    (tv, tf), (pv, pf) = meshes
    spacing = a.spacing
    if spacing is None:
        spacing = max(float(torch.linalg.norm(v.amax(0) - v.amin(0))) for v, _ in meshes if v.shape[0]) / 256
        print(f"spacing {spacing:.6g} (1/256 of the larger box diagonal)")
    stiffness = tuple(float(s) for s in a.stiffness.split(","))
    handles = None
    if a.handles:
        rows = np.atleast_2d(np.asarray(np.load(a.handles), dtype=np.float64))
        if rows.ndim != 2 or rows.shape[1] not in (4, 5):
            raise SystemExit(f"{a.handles}: want rows index, x, y, z[, weight], got {rows.shape[1]} columns")
        handles = (torch.from_numpy(rows[:, 0].astype(np.int64)).to(dev), torch.from_numpy(rows[:, 1:4].astype(np.float32)).to(dev),
                   torch.from_numpy(np.ascontiguousarray(rows[:, 4] if rows.shape[1] == 5 else np.ones(len(rows)))).to(dev))
        print(f"{a.handles}: {len(rows)} handles")
    report("before", mesh.surface_distance(tv, tf, pv, pf, spacing))
    if a.align:
        res = mesh.register_meshes(tv, tf, pv, pf, spacing, model=a.align, max_distance=a.max_distance)
        print(f"{a.align} registration: {res['status']} after {res['iterations']} steps, scale {res['scale']:.9g}, last rms "
              f"{res['history'][-1]['rms'] if res['history'] else float('nan'):.6g}")
        tv = res["verts"]
        report("aligned", mesh.surface_distance(tv, tf, pv, pf, spacing))
    kw = dict(metric=a.metric, stiffness=stiffness, iterations=a.iterations, handles=handles, max_distance=a.max_distance)
    if a.stiffness_model != "displacement":
        kw["stiffness_model"] = a.stiffness_model
    mesh.warp(tv, tf, pv, pf, **dict(kw, stiffness=stiffness[:1], iterations=min(a.iterations, 1)))          # warm-up
    out = mesh.warp(tv, tf, pv, pf, timing=True, **kw)
    n = max(len(out["history"]), 1)
    print(f"warp ({a.metric} metric, {a.stiffness_model} stiffness {stiffness}): {out['status']} after {out['iterations']} solves (target grid {out['grid']})")
    for i, h in enumerate(out["history"]):
        print(f"  iteration {i}: stiffness {h['stiffness']:g}, rms {h['rms']:.6g}, {h['used']} used, rejected " +
              ", ".join(f"{k} {v}" for k, v in h["rejected"].items()) + f", {h['cg_steps']} CG steps ({h['stop']}, rho {h['rho']:.3g}), step {h['step']:.3g}" +
              (f", arap_energy {h['arap_energy']:.6g}" if "arap_energy" in h else ""))
    t = out["times"]
    print(f"  binning {t['bin'] * 1e3:.2f} ms once; per iteration query {t['query'] * 1e3 / n:.2f} ms, reject + system {t['system'] * 1e3 / n:.2f} ms, "
          f"solve {t['solve'] * 1e3 / n:.2f} ms" + (f", rotations + right-hand side {t['arap'] * 1e3 / n:.2f} ms" if "arap" in t else "") +
          " (each phase ended by a synchronisation)")
    print(f"  rms relative edge-length change of the template: {edge_change(tv, out['verts'], tf):.6g}")
    report("after", mesh.surface_distance(out["verts"], tf, pv, pf, spacing))
    mesh.write_ply(a.out, out["verts"], tf)
    print(f"wrote {a.out}: the warped template, V = {out['verts'].shape[0]}, with the template's {tf.shape[0]} faces")


if __name__ == "__main__":
    main()

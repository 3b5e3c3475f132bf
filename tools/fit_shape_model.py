#!/usr/bin/env python3
"""Fit a linear shape model (``tools/build_shape_model.py``) to a mesh with a triangulation of its own on the GPU (``mesh.shape_fit``:
model-based closest points, K coefficients and an optional pose).

  python tools/fit_shape_model.py MODEL.npz TARGET.ply --out FIT.ply [--pose rigid|similarity|translation] [--metric plane|point]
                                  [--regularize L] [--iterations N] [--max-distance D] [--spacing S] [--then-warp]

The model file must hold its faces.  The tool prints the history of every iteration, the time per iteration split into query, rows, Gram
and host solve, and the surface distance (``mesh.surface_distance``, fit -> target and back) of the mean and of the fit, and writes the
fitted mesh with the model's faces.  ``--then-warp`` hands the fit to ``mesh.warp`` as its template position and prints the distance after
the warp as well; FIT.ply then holds the warped fit.
Meshes extracted from seeded synthetic weights are noise: what the fit does on a trained face or a real scan has not been measured."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import mesh  # noqa: E402


def report(name, d):
    print(f"{name}: fit -> target rms {d['a_to_b']['rms']:.6g} (max {d['a_to_b']['max']:.6g}), target -> fit rms {d['b_to_a']['rms']:.6g} "
          f"(max {d['b_to_a']['max']:.6g}), chamfer {d['chamfer']:.6g}")


def entry_text(e):
    return f"rms {e['rms']:.6g}, {e['used']} used, rejected " + ", ".join(f"{k} {v}" for k, v in e["rejected"].items()) + f", step {e['step']:.3g}"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", metavar="MODEL.npz")
    ap.add_argument("target", metavar="TARGET.ply")
    ap.add_argument("--out", required=True, metavar="FIT.ply")
    ap.add_argument("--pose", choices=("rigid", "similarity", "translation"), default=None, help="also fit a pose (default: coefficients only)")
    ap.add_argument("--metric", choices=("plane", "point"), default="plane")
    ap.add_argument("--regularize", type=float, default=0.0, metavar="L", help="weight of |c|^2 (default 0)")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--max-distance", type=float, default=None, help="bound of the closest-point search (default: unbounded)")
    ap.add_argument("--spacing", type=float, default=None, help="quadrature spacing of the distances (default: 1/256 of the target's box diagonal)")
    ap.add_argument("--then-warp", action="store_true", help="warp the fit onto the target afterwards (mesh.warp's defaults)")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    model = mesh.read_shape_model(a.model, dev)
    if "faces" not in model:
        raise SystemExit(f"{a.model} holds no faces: build it with tools/build_shape_model.py")
    faces = model["faces"]
    rec = mesh.read_ply(a.target)
    pv, pf = torch.from_numpy(np.ascontiguousarray(rec[0])).to(dev), torch.from_numpy(np.ascontiguousarray(rec[1])).to(dev)
    print(f"{a.model}: V = {model['mean'].shape[0]}, K = {model['modes'].shape[0]} modes of {model['n_meshes']} meshes; {a.target}: V = {pv.shape[0]}, "
          f"F = {pf.shape[0]}")
    spacing = a.spacing if a.spacing is not None else float(torch.linalg.norm(pv.amax(0) - pv.amin(0))) / 256
    report("mean", mesh.surface_distance(model["mean"].to(torch.float32), faces, pv, pf, spacing))
    kw = dict(metric=a.metric, pose=a.pose, regularize=a.regularize, max_distance=a.max_distance)
    mesh.shape_fit(model, pv, pf, iterations=min(a.iterations, 1), **kw)                                   # warm-up
    out = mesh.shape_fit(model, pv, pf, iterations=a.iterations, timing=True, **kw)
    n = max(len(out["history"]), 1)
    print(f"fit ({a.metric} metric, pose {a.pose}, regularize {a.regularize:g}): {out['status']} after {out['iterations']} iterations (target grid "
          f"{out['grid']}), scale {out['scale']:.9g}")
    for i, h in enumerate(out["history"]):
        if h["pose"] is not None:
            print(f"  iteration {i} pose:  {entry_text(h['pose'])}")
        if h["shape"] is not None:
            print(f"  iteration {i} shape: {entry_text(h['shape'])}")
    print("  coefficients (standard deviations): " + " ".join(f"{c:.4f}" for c in out["coeffs"][:16]) + (" ..." if len(out["coeffs"]) > 16 else ""))
    t = out["times"]
    print(f"  binning {t['bin'] * 1e3:.2f} ms once; per iteration query {t['query'] * 1e3 / n:.2f} ms, rows {t['rows'] * 1e3 / n:.2f} ms, Gram "
          f"{t['gram'] * 1e3 / n:.2f} ms, host solve {t['host'] * 1e3 / n:.2f} ms (each phase ended by a synchronisation)")
    verts = out["verts"]
    report("fit", mesh.surface_distance(verts, faces, pv, pf, spacing))
    if a.then_warp:
        warped = mesh.warp(verts, faces, pv, pf, metric=a.metric, max_distance=a.max_distance)
        print(f"warp from the fit: {warped['status']} after {warped['iterations']} solves")
        verts = warped["verts"]
        report("fit + warp", mesh.surface_distance(verts, faces, pv, pf, spacing))
    mesh.write_ply(a.out, verts, faces)
    print(f"wrote {a.out}: V = {verts.shape[0]}, with the model's {faces.shape[0]} faces")


if __name__ == "__main__":
    main()

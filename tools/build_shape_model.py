#!/usr/bin/env python3
"""Build a linear shape model — a mean and modes of variation — from meshes that share one vertex numbering (outputs of ``mesh.warp`` /
``tools/fit_template.py``) on the GPU (``mesh.shape_model``: principal components by the M x M Gram matrix).

  python tools/build_shape_model.py MESH.ply [MESH.ply ...] --out MODEL.npz [--align rigid|similarity] [--components K] [--rank-tol T]

Between 2 and 256 meshes; meshes with differing vertex counts are refused (their rows would not correspond).  The faces of the first
mesh go into the file.  ``--align`` fits every mesh onto the running mean first (two rounds of ``mesh.fit_transform`` over all vertices).
The tool prints the spectrum, the explained variance and the time of each stage — reading, alignment, centre + Gram matrix, the host
Jacobi, the modes, writing — each ended by a device synchronisation, and writes
``MODEL.npz`` (``mesh.write_shape_model``: plain arrays, nothing pickled).
Meshes extracted from seeded synthetic weights are noise: what a model of trained faces or real scans looks like has not been measured."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import mesh  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("meshes", nargs="+", metavar="MESH.ply")
    ap.add_argument("--out", required=True, metavar="MODEL.npz")
    ap.add_argument("--align", choices=("rigid", "similarity"), default=None, help="fit every mesh onto the running mean first")
    ap.add_argument("--components", type=int, default=None, help="modes to keep (default: those above --rank-tol)")
    ap.add_argument("--rank-tol", type=float, default=1e-10, help="keep eigenvalues above this share of the largest (default 1e-10)")
    a = ap.parse_args(argv)
    if not 2 <= len(a.meshes) <= mesh.SHAPE_MAX_ROWS:
        raise SystemExit(f"{len(a.meshes)} meshes: want 2 .. {mesh.SHAPE_MAX_ROWS}")
    dev = torch.device("cuda", torch.cuda.current_device())
    t0 = time.perf_counter()
    verts, faces = [], None
    for path in a.meshes:
        rec = mesh.read_ply(path)
        v = np.ascontiguousarray(rec[0], dtype=np.float32)
        if verts and v.shape != verts[0].shape:
            raise SystemExit(f"{path}: {v.shape[0]} vertices, {a.meshes[0]} has {verts[0].shape[0]}: the meshes do not share a vertex numbering")
        if faces is None:
            faces = np.ascontiguousarray(rec[1], dtype=np.int32)
        verts.append(v)
    stack = torch.from_numpy(np.stack(verts)).to(dev)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    print(f"read {len(verts)} meshes of V = {stack.shape[1]} vertices, F = {len(faces)} faces: {(t1 - t0) * 1e3:.1f} ms")
    mesh.shape_model(stack[:2])                                                  # warm-up
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    model = mesh.shape_model(stack, components=a.components, rank_tol=a.rank_tol, align=a.align, timing=True)
    times = model.pop("times")
    torch.cuda.synchronize(dev)
    t2 = time.perf_counter()
    lam = model["eigenvalues"]
    print(f"model ({'no alignment' if a.align is None else a.align + ' alignment'}): {model['status']}, K = {len(model['sigma'])} modes of "
          f"{model['n_meshes']} meshes: {(t2 - t1) * 1e3:.1f} ms")
    print(f"  stages: alignment {times['align'] * 1e3:.1f} ms, centre + Gram matrix {times['gram'] * 1e3:.2f} ms, host Jacobi {times['jacobi'] * 1e3:.1f} ms, "
          f"modes {times['modes'] * 1e3:.2f} ms (each ended by a synchronisation)")
    print("  eigenvalues / largest: " + " ".join(f"{v / lam[0]:.3e}" for v in lam[:16]) + (" ..." if len(lam) > 16 else ""))
    print("  sigma: " + " ".join(f"{v:.6g}" for v in model["sigma"][:16]) + (" ..." if len(model["sigma"]) > 16 else ""))
    print("  explained variance: " + " ".join(f"{v:.4f}" for v in model["explained"][:16]) + f"  (sum {float(np.sum(model['explained'])):.6f})")
    mesh.write_shape_model(a.out, model, faces)
    print(f"wrote {a.out}: {(time.perf_counter() - t2) * 1e3:.1f} ms")


if __name__ == "__main__":
    main()

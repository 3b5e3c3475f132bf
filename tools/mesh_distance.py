#!/usr/bin/env python3
"""Surface distance between two triangle meshes on the GPU (``mesh.surface_distance``): for each direction the area-weighted mean, rms,
median and 95 % of the distance from a deterministic quadrature of one surface (plus its vertices, which count in the maximum only) to the
exact closest point of the other, the maximum, the Hausdorff distance (the larger maximum) and the chamfer distance (the sum of the means).

  python tools/mesh_distance.py A.ply B.ply [--spacing S] [--max-distance D] [--signed] [--heat OUT.ply]

``--spacing`` is the quadrature's spacing (default: 1/256 of the larger box diagonal); ``--max-distance`` bounds the search (samples
farther than it are counted, not averaged); ``--heat`` writes mesh A with vertex colours from its vertices' distance to B (black at 0 to
white at the largest).  The distances are unsigned unless ``--signed`` is given: every sample then also gets the other mesh's winding number
(``mesh.winding_number``; both meshes must be closed, the tool exits with the library's message otherwise) and each direction prints the
signed mean (negative inside the other mesh), the share of the surface that lies inside it and the largest distance on either side.
Meshes extracted from seeded synthetic weights (``tools/extract_mesh.py --synthetic``)
are noise: their distances say nothing about a trained face.

  python tools/mesh_distance.py A.ply B.ply --align rigid|similarity|translation [--metric plane|point] [--iterations N] [--trim T]
                                            [--tol E] [--init FILE.npy] [--write-aligned OUT.ply]

``--align`` first registers A onto B (``mesh.register_meshes``: iterated closest points from A's quadrature onto B) — two
meshes from different tools, a scan, or the same head in another unit are not in one frame, and no distance means anything until they
are.  The tool prints the distance before, the transform (scale, rotation, translation), every iteration's rms, used and rejected
correspondences and step, the time per iteration split into query, terms + reduce and host, and then its usual report on the aligned A.
``--init`` starts from a 4 x 4 matrix (``numpy.save``; e.g. ``mesh.fit_transform`` of a few landmarks): the method is local and finds the
nearest minimum.  ``--write-aligned`` writes the aligned A and the matrix found.  Without ``--align`` nothing changes.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import mesh  # noqa: E402
from extract_mesh import distance_report  # noqa: E402


def align(a, va, fa, vb, fb, spacing, kw):
    """``--align``: registers A onto B (``mesh.register_meshes``), prints the transform, the history and the distance before; returns A's
    vertices under the transform (the distance after is the tool's usual report)."""
    before = mesh.surface_distance(va, fa, vb, fb, spacing, **kw)
    print(f"before the alignment: A -> B rms {before['a_to_b']['rms']:.6g}, B -> A rms {before['b_to_a']['rms']:.6g}, Hausdorff "
          f"{before['hausdorff']:.6g}, chamfer {before['chamfer']:.6g}")
    rkw = dict(model=a.align, metric=a.metric, iterations=a.iterations, trim=a.trim, tol=a.tol, max_distance=a.max_distance,
               init=None if a.init is None else np.load(a.init))
    mesh.register_meshes(va, fa, vb, fb, spacing, **dict(rkw, iterations=min(a.iterations, 1)))          # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = mesh.register_meshes(va, fa, vb, fb, spacing, **rkw)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    n = max(len(res["history"]), 1)
    print(f"{a.align} registration ({a.metric} metric) of {res['n_samples']} samples of A onto B: {res['status']} after {res['iterations']} steps, "
          f"{t * 1e3:.2f} ms in all, {t * 1e3 / n:.2f} ms per iteration (target grid {res['grid']})")
    times = mesh.register_meshes(va, fa, vb, fb, spacing, timing=True, **rkw)["times"]
    print(f"  a further call, each phase ended by a synchronisation: binning {times['bin'] * 1e3:.2f} ms once; per iteration query "
          f"{times['query'] * 1e3 / n:.2f} ms, reject + terms + reduce {times['terms'] * 1e3 / n:.2f} ms, host solve {times['host'] * 1e3 / n:.3f} ms")
    print(f"  scale {res['scale']:.9g}\n  rotation\n" + "\n".join("    " + " ".join(f"{v: .9f}" for v in row) for row in res["rotation"]) +
          "\n  translation " + " ".join(f"{v:.9g}" for v in res["translation"]))
    for i, h in enumerate(res["history"]):
        print(f"  iteration {i}: rms {h['rms']:.6g}, {h['used']} used, step {h['step']:.3g}, rejected " +
              ", ".join(f"{k} {v}" for k, v in h["rejected"].items()))
    if a.write_aligned:
        mesh.write_ply(a.write_aligned, res["verts"], fa)
        np.save(os.path.splitext(a.write_aligned)[0] + "_matrix.npy", res["matrix"])
        print(f"wrote {a.write_aligned}: A under the transform (its 4 x 4 matrix next to it as .npy); the distance after the alignment follows")
    return res["verts"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--align", choices=("rigid", "similarity", "translation"), default=None, help="register A onto B first (mesh.register_meshes)")
    ap.add_argument("--metric", choices=("plane", "point"), default="plane", help="--align: the residual (default plane)")
    ap.add_argument("--iterations", type=int, default=30, help="--align: most iterations (default 30)")
    ap.add_argument("--trim", type=float, default=None, help="--align: keep this share of the closest correspondences (default: all)")
    ap.add_argument("--tol", type=float, default=1e-7, help="--align: stop when the step falls to this (default 1e-7)")
    ap.add_argument("--init", default=None, metavar="FILE.npy", help="--align: a 4 x 4 similarity matrix to start from")
    ap.add_argument("--write-aligned", default=None, metavar="OUT.ply", help="--align: write A under the transform found")
    ap.add_argument("--spacing", type=float, default=None, help="quadrature spacing (default: 1/256 of the larger box diagonal)")
    ap.add_argument("--max-distance", type=float, default=None, help="bound of the search (default: unbounded)")
    ap.add_argument("--no-vertices", action="store_true", help="leave the meshes' vertices out of the maxima")
    ap.add_argument("--signed", action="store_true", help="also print the signed statistics (both meshes must be closed)")
    ap.add_argument("--heat", default=None, metavar="OUT.ply", help="write A with vertex colours from its vertices' distance to B")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    meshes = []
    for path in (a.a, a.b):
        rec = mesh.read_ply(path)
        v, f = torch.from_numpy(np.ascontiguousarray(rec[0])).to(dev), torch.from_numpy(np.ascontiguousarray(rec[1])).to(dev)
        print(f"{path}: V = {v.shape[0]}, F = {f.shape[0]}")
        meshes.append((v, f))
    (va, fa), (vb, fb) = meshes
    spacing = a.spacing
    if spacing is None:
        spacing = max(float(torch.linalg.norm(v.amax(0) - v.amin(0))) for v, _ in meshes if v.shape[0]) / 256
        print(f"spacing {spacing:.6g} (1/256 of the larger box diagonal)")
    kw = dict(max_distance=a.max_distance, vertices=not a.no_vertices, signed=a.signed)
    if a.align:
        va = align(a, va, fa, vb, fb, spacing, kw)
    try:
        mesh.surface_distance(va, fa, vb, fb, spacing, **kw)          # warm-up
    except mesh.lib.MofaError as e:
        if not a.signed:
            raise
        raise SystemExit(str(e))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = mesh.surface_distance(va, fa, vb, fb, spacing, **kw)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    out["times"] = mesh.surface_distance(va, fa, vb, fb, spacing, timing=True, **kw)["times"]
    print(f"surface distance in {t * 1e3:.2f} ms (the phases below are a further call, each ended by a synchronisation):")
    distance_report(out, "A -> B", "B -> A")
    if a.signed:
        for d, name in (("a_to_b", "A -> B"), ("b_to_a", "B -> A")):
            e = out[d]
            print(f"  {name} signed: mean {e['signed_mean']:.6g} (negative inside the other mesh), {100 * e['inside_fraction']:.2f} % of the surface "
                  f"inside, largest distance inside {e['max_inside']:.6g}, outside {e['max_outside']:.6g}")
    if a.heat:
        res = mesh.closest_points(va, vb, fb, max_distance=a.max_distance)
        d = res["distance"]
        ok = torch.isfinite(d)
        top = float(d[ok].max()) if bool(ok.any()) else 0.0
        shade = torch.where(ok, d / top if top > 0 else torch.zeros_like(d), torch.ones_like(d))
        mesh.write_ply(a.heat, va, fa, shade[:, None].expand(-1, 3).contiguous())
        print(f"wrote {a.heat}: A with its vertices' distance to B as grey, white = {top:.6g}" +
              (f" ({int((~ok).sum())} vertices beyond the bound are white)" if not bool(ok.all()) else ""))


if __name__ == "__main__":
    main()

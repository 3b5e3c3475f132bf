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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
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

#!/usr/bin/env python3
"""Export the geometry of a MoFaNeRF face as a PLY mesh: the fine network's density on a grid (``Renderer.query_density``), marching
tetrahedra on the GPU (``Renderer.extract_mesh``), optional per-vertex colours from the full network.

Networks come from a checkpoint (``--ckpt DIR`` holding the ``*.tar`` files run_train.py writes, or one ``.tar``) or from seeded
synthetic weights (``--synthetic D W``); codes from a fit (``--fit saving_Parameters.tar`` as run_fit.py writes it: saving_bm,
saving_uv, saving_exp) or from ``synth.codes``.  ``--bounds`` and ``--level`` are required: no iso-level or box of a trained model has
been measured, so there are no defaults.

  python tools/extract_mesh.py --synthetic 10 1024 --bounds -1 -1 -1 1 1 1 --resolution 256 256 256 --level 0 --out face.ply --time
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mofanerf_amd import factory, mesh, synth  # noqa: E402


def load(a, dev):
    if a.synthetic:
        D, W = a.synthetic
        args = factory.default_args(netdepth_fine=D, netwidth_fine=W, no_reload=True, device=dev, basedir="/nonexistent")
    elif os.path.isdir(a.ckpt):
        path = os.path.abspath(a.ckpt)
        args = factory.default_args(basedir=os.path.dirname(path), expname=os.path.basename(path), device=dev)
    else:
        args = factory.default_args(ft_path=a.ckpt, device=dev)
    _, kw, _, _, _, _, render = factory.create_nerf(args)
    net = kw["network_fine"] if kw.get("network_fine") is not None else kw["network_fn"]
    if a.synthetic:
        net.load_state_dict(synth.nerf_state(a.synthetic[0], a.synthetic[1], a.seed, "fine"))
        render.idSpecificMod.load_state_dict(synth.style_state(a.seed))
        for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(a.seed)):
            dst.data[:] = src.to(dst.device)
    render.eval()
    net.eval()
    if a.fit:
        fit = torch.load(a.fit, map_location=dev)
        bm, uv, exp = fit["saving_bm"], fit["saving_uv"], fit["saving_exp"]
    else:
        bm, uv, exp = synth.codes(a.seed)
    return render, net, bm.reshape(1, -1).float().to(dev), uv.reshape(-1).float().to(dev), exp.reshape(1, -1).float().to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", help="checkpoint directory (the newest *.tar is used) or one .tar file")
    src.add_argument("--synthetic", type=int, nargs=2, metavar=("D", "W"), help="seeded synthetic fine network D x W")
    ap.add_argument("--fit", help="saving_Parameters.tar of run_fit.py (shape / texture / expression codes); default synth.codes")
    ap.add_argument("--seed", type=int, default=0, help="seed of the synthetic weights / codes")
    ap.add_argument("--bounds", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--resolution", type=int, nargs=3, default=[256, 256, 256], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--level", type=float, required=True, help="iso-level of the pre-ReLU density (no default)")
    ap.add_argument("--colors", action="store_true", help="per-vertex colours from the full network (needs the texture code)")
    ap.add_argument("--netchunk", type=int, default=None, help="points per density launch (default: the renderer's netchunk)")
    ap.add_argument("--out", default="mesh.ply")
    ap.add_argument("--time", action="store_true", help="after a warm-up: density and extraction times, density vs forward_points")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    render, net, bm, uv, exp = load(a, dev)
    bounds = (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
    res = tuple(a.resolution)
    kw = dict(bounds=bounds, resolution=res, shapeCodes=bm, expType=20, expCodes=exp, netchunk=a.netchunk)
    out = render.extract_mesh(net, level=a.level, uvCodes=uv if a.colors else None, colors=a.colors, **kw)
    verts, faces = out[0], out[1]
    mesh.write_ply(a.out, verts, faces, out[2] if a.colors else None)
    print(f"wrote {a.out}: V = {verts.shape[0]}, F = {faces.shape[0]}")
    if not a.time:
        return

    def timed(fn, reps=2):
        fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(reps):
            t = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t)
        return best, r

    n = res[0] * res[1] * res[2]
    t_density, grid = timed(lambda: render.query_density(net, **kw))
    # the same points through the full network (forward_points: texture stack, view layer, both heads) in the same chunks
    _, lo, step = mesh.grid_spec(bounds, res)
    pts = torch.empty(n, 3, dtype=torch.float32, device=dev)
    mesh.grid_points(res, lo, step, 0, n, pts)
    vd = torch.nn.functional.normalize(torch.ones(n, 3, device=dev), dim=-1).contiguous()
    render.decoding_texCodes = uv

    def full():
        with torch.no_grad():
            raw = render.run_network(pts[:, None, :], vd, net)
        render.check_launches(block=True)
        return raw

    t_full, raw = timed(full)
    if not torch.equal(raw[:, 0, 3], grid.reshape(-1)):
        raise SystemExit("density differs from forward_points' raw[..., 3]")
    t_iso, (v2, f2) = timed(lambda: mesh.iso_surface(grid, a.level, lo, step))
    print(f"grid {res[0]}x{res[1]}x{res[2]} = {n} points, network {net.D}x{net.W}, netchunk {a.netchunk or render.netchunk}")
    print(f"density (query_density):        {t_density * 1e3:9.2f} ms  {n / t_density / 1e6:9.2f} M points/s")
    print(f"full forward (forward_points):  {t_full * 1e3:9.2f} ms  {n / t_full / 1e6:9.2f} M points/s")
    print(f"density speed-up over the full forward: {t_full / t_density:.3f}x  (bit-identical sigma)")
    print(f"extraction (count + read + emit): {t_iso * 1e3:9.3f} ms  = {100 * t_iso / t_density:.3f} % of the density query")
    print(f"V = {v2.shape[0]}, F = {f2.shape[0]}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Export the geometry of a MoFaNeRF face as a PLY mesh: the fine network's density on a grid (``Renderer.query_density``), marching
tetrahedra on the GPU (``Renderer.extract_mesh``), optional per-vertex colours from the full network.

Networks come from a checkpoint (``--ckpt DIR`` holding the ``*.tar`` files run_train.py writes, or one ``.tar``) or from seeded
synthetic weights (``--synthetic D W``); codes from a fit (``--fit saving_Parameters.tar`` as run_fit.py writes it: saving_bm,
saving_uv, saving_exp) or from ``synth.codes``.  ``--bounds`` and ``--level`` are required: no iso-level or box of a trained model has
been measured, so there are no defaults.

  python tools/extract_mesh.py --synthetic 10 1024 --bounds -1 -1 -1 1 1 1 --resolution 256 256 256 --level 0 --out face.ply --time

``--brick B`` takes the narrow-band path (densities only in the bricks of B^3 cells the surface passes through; (n - 1) % B == 0 on
every axis), which reaches grids the dense path refuses; ``--compare-dense`` also runs the dense path and exits non-zero unless the two
meshes are equal after renumbering by edge id:

  python tools/extract_mesh.py --synthetic 10 1024 --bounds -1 -1 -1 1 1 1 --resolution 513 513 513 --level 0 --brick 8 \
      --compare-dense --time

``--refine K`` then moves every vertex along its lattice edge onto the level by K bisection steps on the network's density (the
placement of a grid 2^K times finer along each edge; faces unchanged), and ``--normals density|faces`` writes per-vertex normals
(``nx ny nz``) to the PLY.

``--components largest`` or ``--components N`` removes floaters before any of that: the mesh's connected components are labelled on the
GPU and only the one with the most faces, or every one with at least N faces, is kept; the tool prints the largest components (faces,
area, signed volume, box) and what was removed.  With ``--time`` it also prints the labelling's passes and the time of each stage next to
the extraction's.  ON SEEDED WEIGHTS THE COMPONENTS SAY NOTHING ABOUT THE FLOATERS OF A TRAINED FACE: a seeded network's density is noise.

``--simplify M`` simplifies the mesh by vertex clustering on cells of M grid steps with one quadric-error representative per cluster
(``mesh.simplify``; ``--placement mean`` is plain clustering, the baseline), after ``--components`` and ``--refine`` and before
``--normals`` and ``--colors``; the tool prints the counts before and after and how the representatives were placed.  The result is
closed where the input is, not necessarily manifold.  What the method does to a trained face has not been measured: seeded weights say
nothing about it.  ``--simplify-error`` measures the surface distance between the unsimplified and the simplified mesh, both ways
(``mesh.surface_distance`` sampled at one grid step), and prints it; on seeded weights it says nothing about a trained face either.

``--smooth N`` runs N iterations of Taubin smoothing over the vertices (``mesh.smooth``: lam 0.5, mu -0.53, the boundary fixed;
``--smooth-weights uniform|cotangent``) after all of the above and before ``--normals`` and ``--colors``; the tool prints the statistics
and the signed volume before and after (``mesh.components``; the mesh is extracted a second time without smoothing for it).  Smoothing
moves the vertices off the level set.  On seeded weights it says nothing about a trained face.
"""
import argparse
import itertools
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


def components_arg(text):
    if text == "largest":
        return text
    try:
        n = int(text)
    except ValueError:
        n = 0
    if n < 1:
        raise argparse.ArgumentTypeError(f"{text!r}: want 'largest' or a face count >= 1")
    return n


def components_report(st, top=8):
    """The largest components of the unfiltered mesh and what the filter removed (render.mesh_stats["components"])."""
    n_c = st["n_components"]
    n_faces, n_verts, kept = st["n_faces"].cpu(), st["n_verts"].cpu(), st["kept"].cpu()
    area, volume, bbox = st["area"].cpu(), st["volume"].cpu(), st["bbox"].cpu()
    print(f"components: {n_c} over {int(n_faces.sum())} faces, labelled in {st['passes']} passes; {st['unreferenced']} unreferenced vertices")
    print("  label      faces      verts          area        volume  kept  box")
    for c in torch.argsort(n_faces, descending=True, stable=True)[:top].tolist():
        lo, hi = bbox[c, 0].tolist(), bbox[c, 1].tolist()
        box = " ".join(f"[{a:.3f}, {b:.3f}]" for a, b in zip(lo, hi))
        print(f"  {c:5d} {int(n_faces[c]):10d} {int(n_verts[c]):10d} {float(area[c]):13.6g} {float(volume[c]):13.6g}  {'yes' if kept[c] else 'no ':4s} {box}")
    gone = ~kept
    print(f"removed {int(gone.sum())} components: {int(n_faces[gone].sum())} faces, {int(n_verts[gone].sum())} vertices, area "
          f"{float(area[gone].sum()):.6g}, volume {float(volume[gone].sum()):.6g}")


def simplify_arg(text):
    try:
        m = int(text)
    except ValueError:
        m = 0
    if m < 2:
        raise argparse.ArgumentTypeError(f"{text!r}: want an integer >= 2 (grid steps per cell)")
    return m


def simplify_report(st):
    """Counts before and after and the placement routes (render.mesh_stats["simplify"])."""
    print(f"simplified: {st['verts_in']} vertices / {st['faces_in']} faces -> {st['verts_out']} / {st['faces_out']} "
          f"({st['faces_in'] / max(st['faces_out'], 1):.1f}x fewer faces); {st['n_clusters']} clusters, {st['faces_degenerate']} faces collapsed, "
          f"{st['faces_cancelled']} cancelled as fins")
    print(f"  representatives: {st['placed_quadric']} at the quadric minimiser, {st['placed_mean']} at the cluster mean "
          f"({st['mean_requested']} of them requested), {st['placed_first']} at the first vertex; {st['edges_multiple']} directed edges are used "
          f"by more than one face (non-manifold there)")


def smooth_arg(text):
    try:
        n = int(text)
    except ValueError:
        n = 0
    if n < 1:
        raise argparse.ArgumentTypeError(f"{text!r}: want an integer >= 1 (Taubin iterations)")
    return n


def signed_volume(verts, faces):
    """The mesh's signed volume: the sum over its components (mesh.components)."""
    return float(mesh.components(verts.contiguous(), faces.contiguous())["volume"].sum())


def smooth_report(st, weights, volume_before, volume_after):
    """The statistics of mesh.smooth (render.mesh_stats["smooth"]) and the signed volume on both sides of it."""
    print(f"smoothed: {st['passes']} passes with {weights} weights; {st['n_pinned']} vertices pinned ({st['n_boundary']} on the boundary), "
          f"{st['n_isolated']} without neighbours, largest degree {st['degree_max']}, {st['edges_nonmanifold']} non-manifold edges")
    print(f"  displacement: max {st['max_displacement']:.6g}, mean {float(st['displacement'].mean()) if st['displacement'].numel() else 0.0:.6g}; "
          f"{st['flat_corners']} flat corners, {st['negative_weights']} negative weights clamped, {st['zero_weight']} vertices kept for a zero weight sum")
    print(f"  signed volume {volume_before:.6g} -> {volume_after:.6g} ({volume_after / volume_before if volume_before else float('nan'):.4f} x)")


def distance_report(err, what="unsimplified -> simplified", back="simplified -> unsimplified"):
    """The statistics of mesh.surface_distance, one line per direction."""
    for d, name in (("a_to_b", what), ("b_to_a", back)):
        e = err[d]
        print(f"  {name}: mean {e['mean']:.6g}, rms {e['rms']:.6g}, median {e['p50']:.6g}, 95 % {e['p95']:.6g}, max {e['max']:.6g} "
              f"({e['n_samples']} samples, {e['n_beyond']} beyond the bound; grid {e['grid']}, "
              f"{e['counts']['candidate_tests'] / max(e['n_samples'], 1):.1f} triangle tests per sample)")
    print(f"  Hausdorff {err['hausdorff']:.6g}, chamfer (sum of the two means) {err['chamfer']:.6g}")
    if "times" in err:
        print("  seconds: " + ", ".join(f"{k} {v:.4f}" for k, v in err["times"].items()))


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
    ap.add_argument("--time", action="store_true", help="after a warm-up: density and extraction times, density vs forward_points "
                    "(with --brick: the band's seed / density / growth / meshing split against the dense path)")
    ap.add_argument("--brick", type=int, default=None, help="narrow-band extraction with bricks of B^3 cells (4, 8 or 16)")
    ap.add_argument("--compare-dense", action="store_true", help="with --brick: also run the dense path and require equal meshes")
    ap.add_argument("--refine", type=int, default=0, metavar="K", help="move every vertex along its lattice edge onto the level by K "
                    "bisection steps on the density (0 .. 20; (2 + K) V more density evaluations, faces unchanged)")
    ap.add_argument("--normals", choices=("density", "faces"), default=None, help="write per-vertex normals to the PLY: the density "
                    "field's (central differences at half a grid step) or the area-weighted face normals")
    ap.add_argument("--components", type=components_arg, default=None, metavar="largest|N", help="remove floaters: keep the connected "
                    "component with the most faces, or every component with at least N faces (before --refine / --normals / --colors)")
    ap.add_argument("--simplify", type=simplify_arg, default=None, metavar="M", help="simplify by vertex clustering on cells of M grid steps "
                    "(after --components / --refine, before --normals / --colors)")
    ap.add_argument("--placement", choices=("quadric", "mean"), default="quadric", help="with --simplify: the quadric-error representative "
                    "or the cluster mean (plain clustering)")
    ap.add_argument("--simplify-error", action="store_true", help="with --simplify: measure and print the surface distance between the "
                    "unsimplified and the simplified mesh (mesh.surface_distance, sampled at one grid step)")
    ap.add_argument("--smooth", type=smooth_arg, default=None, metavar="N", help="N iterations of Taubin smoothing (mesh.smooth) after "
                    "--components / --refine / --simplify, before --normals / --colors")
    ap.add_argument("--smooth-weights", choices=("uniform", "cotangent"), default="uniform", help="with --smooth: the Laplacian's weights")
    a = ap.parse_args(argv)
    if a.compare_dense and a.smooth is not None:
        ap.error("--compare-dense compares the unsmoothed meshes: drop --smooth")
    if a.simplify_error and a.simplify is None:
        ap.error("--simplify-error needs --simplify")
    if a.compare_dense and a.simplify is not None:
        ap.error("--compare-dense compares the unsimplified meshes: drop --simplify")
    if a.compare_dense and a.components is not None:
        ap.error("--compare-dense compares the unfiltered meshes: drop --components")
    if a.compare_dense and a.brick is None:
        ap.error("--compare-dense needs --brick")
    if a.compare_dense and a.refine:
        ap.error("--compare-dense compares the unrefined meshes: drop --refine")
    dev = torch.device("cuda", torch.cuda.current_device())
    render, net, bm, uv, exp = load(a, dev)
    bounds = (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
    res = tuple(a.resolution)
    kw = dict(bounds=bounds, resolution=res, shapeCodes=bm, expType=20, expCodes=exp, netchunk=a.netchunk)
    out = render.extract_mesh(net, level=a.level, uvCodes=uv if a.colors else None, colors=a.colors, brick=a.brick, refine=a.refine,
                              normals=a.normals, components=a.components, simplify=a.simplify, placement=a.placement,
                              simplify_error=a.simplify_error, smooth=a.smooth, smooth_weights=a.smooth_weights, **kw)
    verts, faces = out[0], out[1]
    mesh.write_ply(a.out, verts, faces, out[2] if a.colors else None, normals=out[-1] if a.normals else None)
    print(f"wrote {a.out}: V = {verts.shape[0]}, F = {faces.shape[0]}")
    if a.components is not None:
        if a.synthetic:
            print("seeded synthetic weights: the components below say NOTHING about the floaters of a trained face")
        components_report(render.mesh_stats["components"])
    if a.refine:
        print(f"refined by {a.refine} bisection steps: {render.mesh_stats['refine']['evaluations']} density evaluations at the vertices' edges")
    if a.simplify is not None:
        if a.synthetic:
            print("seeded synthetic weights: the simplification below says NOTHING about what the method does to a trained face")
        simplify_report(render.mesh_stats["simplify"])
        if a.simplify_error:
            print("surface distance between the unsimplified and the simplified mesh" +
                  (" (seeded synthetic weights: NOTHING about a trained face)" if a.synthetic else "") + ":")
            distance_report(render.mesh_stats["simplify_error"])
    if a.smooth is not None:
        if a.synthetic:
            print("seeded synthetic weights: the smoothing below says NOTHING about what the method does to a trained face")
        stats = dict(render.mesh_stats)
        before = render.extract_mesh(net, level=a.level, brick=a.brick, refine=a.refine, components=a.components, simplify=a.simplify,
                                     placement=a.placement, **kw)
        smooth_report(stats["smooth"], a.smooth_weights, signed_volume(before[0], before[1]), signed_volume(verts, faces))
        render.mesh_stats = stats
    if a.normals == "density":
        print(f"density normals: {render.mesh_stats['zero_normals']} of {verts.shape[0]} vertices have a vanishing gradient")
    if a.brick is not None:
        return band_report(a, render, net, kw, verts, faces)
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
    if a.components is not None:
        ids = torch.arange(v2.shape[0], device=dev)
        t_cc, st = timed(lambda: mesh.components(v2, f2))
        _, st_t = timed(lambda: mesh.components(v2, f2, timing=True), reps=1)
        mask = mesh.select_components(st, a.components)
        t_keep, kept = timed(lambda: mesh.keep_components(v2, f2, st, mask, ids))
        phases = ", ".join(f"{k} {v * 1e3:.3f}" for k, v in st_t["times"].items())
        print(f"components: {st['n_components']} in {st['passes']} passes, {t_cc * 1e3:9.3f} ms = {100 * t_cc / t_iso:.1f} % of the extraction "
              f"(phases, each ended by a synchronisation, ms: {phases})")
        print(f"compaction to {kept[0].shape[0]} vertices / {kept[1].shape[0]} faces with one companion: {t_keep * 1e3:9.3f} ms")
    if a.simplify is not None:
        cell = (a.simplify * step).astype(step.dtype)                  # extract_mesh's cell: M grid steps, in float32
        t_simp, _ = timed(lambda: mesh.simplify(v2, f2, cell, origin=lo, placement=a.placement))
        _, (_, _, st_t) = timed(lambda: mesh.simplify(v2, f2, cell, origin=lo, placement=a.placement, timing=True), reps=1)
        phases = ", ".join(f"{k} {v * 1e3:.3f}" for k, v in st_t["times"].items())
        print(f"simplification of the unfiltered mesh at {a.simplify} steps: {t_simp * 1e3:9.3f} ms = {100 * t_simp / t_iso:.1f} % of the extraction "
              f"(phases, each ended by a synchronisation, ms: {phases})")


def renumbered(verts, faces, edge_ids):
    """The band mesh in the dense numbering (vertices by edge id) with its faces as a canonical multiset (each triangle rotated to start
    at its smallest index, orientation kept; rows sorted), on the GPU."""
    order = torch.argsort(edge_ids)
    new_of_old = torch.empty_like(order)
    new_of_old[order] = torch.arange(order.numel(), device=order.device)
    return verts[order], canonical(new_of_old[faces.long()])


def canonical(faces):
    f = faces.long()
    if f.shape[0] == 0:
        return f
    r = torch.argmin(f, dim=1, keepdim=True)
    f = torch.gather(f, 1, (r + torch.arange(3, device=f.device)) % 3)
    for c in (2, 1, 0):                                   # lexicographic: stable sorts from the last column to the first
        f = f[torch.sort(f[:, c], stable=True).indices]
    return f


def bricks_with_surface(grid, level, B):
    """[bx,by,bz] bool: the brick holds a cell whose 8 corners are not all on one side of the level (a cell with a triangle)."""
    inside = grid >= level
    nx, ny, nz = grid.shape
    n = torch.zeros(nx - 1, ny - 1, nz - 1, dtype=torch.uint8, device=grid.device)
    for dx, dy, dz in itertools.product((0, 1), repeat=3):
        n += inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    mixed = (n > 0) & (n < 8)
    bx, by, bz = (nx - 1) // B, (ny - 1) // B, (nz - 1) // B
    return mixed.reshape(bx, B, by, B, bz, B).any(dim=5).any(dim=3).any(dim=1)


def band_report(a, render, net, kw, verts, faces):
    """--brick: the band's statistics, with --time its time split against the dense path, with --compare-dense the equality check."""
    st = render.mesh_stats
    frac = st["bricks_active"] / max(st["bricks_total"], 1)
    print(f"bricks of {a.brick}^3 cells: {st['bricks_active']} of {st['bricks_total']} active ({100 * frac:.2f} %), "
          f"{st['bricks_seeded']} seeded, {st['rounds']} growth rounds")
    print(f"points evaluated: {st['points_evaluated']} of {st['points_dense']} dense "
          f"({100 * st['points_evaluated'] / st['points_dense']:.2f} %)")
    res = kw["resolution"]
    dense_ok = mesh.lib.load().mofa_iso_workspace_bytes(*res) != 0
    t_dense = None
    if a.time:
        # the band again (warm), phase by phase: each phase ends with a device synchronisation
        _, lo, step = mesh.grid_spec(kw["bounds"], res)
        render._set_codes(kw["shapeCodes"], kw["expType"], kw["expCodes"])
        h = render._hip(net)
        chunk = int(a.netchunk or render.netchunk)
        with torch.no_grad():
            folded = render._fold_codes(net, torch.zeros(h.ch_tex, device=verts.device)).clone()

            def density(pts):
                o = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)
                h.density_points(pts, o, folded)
                return o

            t0 = time.perf_counter()
            _, _, _, ts = mesh.band_surface(density, res, lo, step, a.level, a.brick, chunk, verify=lambda: render.check_launches(block=True),
                                         timing=True)
            t_band = time.perf_counter() - t0
        tm = ts["times"]
        other = tm["seed"] + tm["growth"] + tm["mesh"]
        print(f"band total {t_band * 1e3:9.2f} ms:  seed (corner density + flags) {tm['seed'] * 1e3:.2f} ms, band density "
              f"{tm['density'] * 1e3:.2f} ms, growth {tm['growth'] * 1e3:.2f} ms, meshing {tm['mesh'] * 1e3:.2f} ms")
        n_corner = ts["points_evaluated"] - ts["bricks_active"] * (a.brick + 1) ** 3
        print(f"  corner points {n_corner}, band points {ts['points_evaluated'] - n_corner}; "
              f"seed + growth + meshing = {100 * other / max(tm['density'], 1e-12):.2f} % of the band density time")
        if not dense_ok:
            print(f"dense path: grid {res[0]}x{res[1]}x{res[2]} is refused (7 nx ny nz >= 2^31)")
    if a.compare_dense and not dense_ok:
        raise SystemExit(f"--compare-dense: the dense path refuses grid {res[0]}x{res[1]}x{res[2]}")
    if not (a.compare_dense or (a.time and dense_ok)):
        return
    # the dense path (query_density + iso_surface, which is what extract_mesh runs), timed once
    _, lo, step = mesh.grid_spec(kw["bounds"], res)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    grid = render.query_density(net, **kw)
    with torch.no_grad():
        dv, df = mesh.iso_surface(grid, a.level, lo, step)
    torch.cuda.synchronize()
    t_dense = time.perf_counter() - t0
    bv, bf = renumbered(verts, faces, st["edge_ids"])
    same = bv.shape == dv.shape and torch.equal(bv.view(torch.int32), dv.view(torch.int32)) and torch.equal(bf, canonical(df))
    print(f"dense: V = {dv.shape[0]}, F = {df.shape[0]} (band: V = {verts.shape[0]}, F = {faces.shape[0]});  band == dense after "
          f"renumbering: {same}")
    if a.time:
        print(f"dense query_density + iso_surface {t_dense * 1e3:9.2f} ms;  band speed-up {t_dense / t_band:.2f}x"
              + ("" if same else "  (NOT like for like: the band mesh is a subset of the dense mesh)"))
    if not same:
        # what a band holding the whole dense surface would have cost: every brick with a surface cell, plus the bricks growth added
        need = bricks_with_surface(grid, a.level, a.brick).reshape(-1)
        need[torch.as_tensor(st["active_bricks"], device=need.device)] = True
        n_need = int(need.sum())
        pts = st["points_evaluated"] + (n_need - st["bricks_active"]) * (a.brick + 1) ** 3
        print(f"bricks holding the dense surface or active: {n_need} ({100 * n_need / st['bricks_total']:.2f} %), the band found "
              f"{st['bricks_active']}; a band over all of them evaluates {pts} points ({100 * pts / st['points_dense']:.2f} % of dense)")
        if a.time:
            t_full = tm["seed"] + tm["growth"] + tm["mesh"] + tm["density"] * (pts - n_corner) / max(st["points_evaluated"] - n_corner, 1)
            print(f"  at the measured band density rate that is about {t_full * 1e3:.0f} ms: a like-for-like speed-up of about "
                  f"{t_dense / t_full:.2f}x (estimate)")
    if a.compare_dense and not same:
        raise SystemExit("the band mesh differs from the dense mesh (a surface component without a seeded brick)")


if __name__ == "__main__":
    main()

"""Geometry export: the grid of a density query, the iso-surface of a density grid on the GPU (``mofa_iso_count`` / ``mofa_iso_emit``,
marching tetrahedra on the Freudenthal split), the same mesh from a narrow band of bricks around the surface (``band_surface``,
``mofa_band_*``), the refinement of that mesh's vertices onto the level by bisection along their lattice edges and central-difference
density normals (``refine_vertices``, ``density_normals``, ``mofa_edge_*`` / ``mofa_fd_*``), a binary PLY writer / reader, and the way back from a mesh to a camera: a GPU z-buffer rasteriser (``rasterize``,
``mofa_raster_*``) whose depth is comparable with ``Renderer.render_geometry``'s, and ``depth_agreement`` between the two.
``components`` labels a mesh's connected components (``mofa_cc_*``) with their sizes, areas, signed volumes and boxes;
``select_components`` / ``keep_components`` drop the floaters among them.
``simplify`` clusters a mesh's vertices (``mofa_simp_*``); ``closest_points`` finds the exact closest point of a mesh to every query,
``sample_faces`` samples a surface deterministically and ``surface_distance`` measures one mesh against another (``mofa_dist_*``).
``winding_number`` says which side of a closed mesh a point is on (``mofa_wind_*``); ``signed_distance`` and ``inside_grid`` sit on it.
``vertex_adjacency`` lists every vertex's neighbours in a fixed order and ``smooth`` filters the vertices over it (Taubin, ``mofa_smooth_*``).
``tsdf_volume`` / ``tsdf_integrate`` / ``tsdf_field`` / ``tsdf_surface`` fuse depth frames (``depth_frame``) into a truncated signed distance
volume and march its zero level: a mesh with no density level to choose (``mofa_tsdf_*``).
``register`` / ``register_meshes`` bring points or a mesh into another mesh's frame by rigid or similarity ICP over ``closest_points``' grid,
``fit_transform`` does it for explicit correspondences and ``transform_points`` applies the result (``mofa_icp_*``).
``shape_model`` builds a linear shape model (mean, modes, standard deviations) of meshes with one vertex numbering, ``shape_synthesize`` /
``shape_project`` evaluate and invert it, ``shape_fit`` fits it to a mesh with a triangulation of its own (``mofa_shape_*``).
``bake_state`` / ``bake_integrate`` / ``bake_colors`` project posed colour frames onto a mesh's vertices, occlusion-aware through a depth
frame per view, and ``fill_colors`` closes the holes over the vertex adjacency (``mofa_bake_*``).
``texel_map`` / ``texel_surface`` / ``texture_state`` / ``texture_image`` do the same onto the texels of a texture image through a UV
layout (``uv_locate``, ``dilate_texture``, ``sample_texture``: ``mofa_uv_*``); ``face_atlas`` gives a mesh without UVs a per-triangle
layout, and ``write_obj`` / ``read_obj`` carry mesh, layout and texture as OBJ + MTL + PNG.

``Renderer.query_density`` and ``Renderer.extract_mesh`` are the user-facing entry points; this module holds the pieces they share.
The mesh is watertight and consistently oriented (normals toward lower density); vertices and faces come out in a fixed order with
no atomics, so the same grid gives the same bytes every time.  CPU tensors raise ``MofaError``: there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
import time
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib


def grid_spec(bounds, resolution) -> Tuple[Tuple[int, int, int], np.ndarray, np.ndarray]:
    """``bounds = ((x0,y0,z0), (x1,y1,z1))``, ``resolution = (nx,ny,nz)`` -> (resolution, lo, step): ``step = (hi - lo) / (n - 1)`` in
    float32 on the host.  Every axis needs at least 2 samples and hi > lo."""
    lo, hi = (np.asarray(b, dtype=np.float32).reshape(3) for b in bounds)
    res = tuple(int(n) for n in resolution)
    if len(res) != 3 or min(res) < 2:
        raise lib.MofaError(f"resolution {resolution}: want three axes of at least 2 samples")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise lib.MofaError(f"bounds {bounds}: want finite (x0, y0, z0) < (x1, y1, z1)")
    step = ((hi - lo) / (np.asarray(res, dtype=np.float32) - np.float32(1))).astype(np.float32)
    return res, lo, step


def _f3(v) -> C.Array:
    a = np.asarray(v, dtype=np.float32).reshape(3)
    return (C.c_float * 3)(*[float(x) for x in a])


def grid_points(resolution, lo, step, first: int, n: int, out: torch.Tensor) -> torch.Tensor:
    """out[n,3] = the sample points ``first .. first+n-1`` of the grid (``mofa_grid_points``: idx = (i*ny + j)*nz + k,
    x = lo_x + (float)i * step_x, separately rounded)."""
    nx, ny, nz = resolution
    lib.check(lib.load().mofa_grid_points(nx, ny, nz, _f3(lo), _f3(step), int(first), int(n), lib.ptr(out), lib.stream()),
              "mofa_grid_points")
    return out


def iso_surface(grid: torch.Tensor, level: float, lo, step, edge_ids: bool = False):
    """Triangle mesh of ``{grid >= level}`` for a density grid ``[nx,ny,nz]`` whose sample (i,j,k) sits at lo + (i,j,k) * step:
    ``verts [V,3] float32``, ``faces [F,3] int32`` on the grid's device.  Count, one host read of (V, F), emit.  The grid must be
    finite (a non-finite sample next to the surface has no position).  ``edge_ids=True`` appends ``edge_ids [V] int64``, the lattice
    edge ``7 idx + dir`` each vertex sits on (``mofa_iso_edge_ids``; what :func:`refine_vertices` takes)."""
    if grid.dim() != 3:
        raise lib.MofaError(f"iso_surface: want a [nx,ny,nz] grid, got {tuple(grid.shape)}")
    level = float(level)
    if not np.isfinite(level):
        raise lib.MofaError(f"iso_surface: the level must be finite (got {level})")
    g = grid.detach()
    lib.ptr(g)                                            # (device / dtype / layout check)
    if not bool(torch.isfinite(g).all()):
        raise lib.MofaError("iso_surface: the density grid holds non-finite values")
    nx, ny, nz = (int(v) for v in g.shape)
    L = lib.load()
    nbytes = L.mofa_iso_workspace_bytes(nx, ny, nz)
    if nbytes == 0:
        raise lib.MofaError(f"iso_surface: grid {nx} x {ny} x {nz} is refused (>= 2 samples per axis, 7 nx ny nz < 2^31)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
    counts = torch.empty(2, dtype=torch.int64, device=g.device)
    lib.check(L.mofa_iso_count(lib.ptr(g), nx, ny, nz, level, ws.data_ptr(), counts.data_ptr(), lib.stream()), "mofa_iso_count")
    V, F = (int(v) for v in counts.cpu())
    if V > 2 ** 31 - 1 or F > 2 ** 31 - 1:
        raise lib.MofaError(f"iso_surface: {V} vertices / {F} faces exceed the int32 face indices (2^31 - 1)")
    verts = torch.empty(V, 3, dtype=torch.float32, device=g.device)
    faces = torch.empty(F, 3, dtype=torch.int32, device=g.device)
    if V and F:
        lib.check(L.mofa_iso_emit(lib.ptr(g), nx, ny, nz, _f3(lo), _f3(step), level, ws.data_ptr(), lib.ptr(verts), faces.data_ptr(),
                                  lib.stream()), "mofa_iso_emit")
    if not edge_ids:
        return verts, faces
    ids = torch.empty(V, dtype=torch.int64, device=g.device)
    if V:
        lib.check(L.mofa_iso_edge_ids(nx, ny, nz, ws.data_ptr(), ids.data_ptr(), lib.stream()), "mofa_iso_edge_ids")
    return verts, faces, ids


BRICKS = (4, 8, 16)


def band_surface(density_fn, resolution, lo, step, level, brick, chunk, verify=None, timing=False):
    """Narrow-band ("sparse brick") extraction of ``{density >= level}`` on the fine lattice of :func:`grid_points` (``mofa_band_*``):
    densities are asked for only at the brick-corner lattice and in the ``brick^3``-cell bricks the surface passes through, so the work
    follows the surface, not the volume.  ``density_fn(pts [n,3] float32 GPU) -> [n]`` is any GPU float32 function of the point (a point
    asked for twice must give the same bits); it is called with at most ``chunk`` points.  ``verify()``, if given, runs after each
    round's densities and before any kernel reads them (``Renderer.extract_mesh`` waits for its launch verdicts there).

    A brick is seeded when its 8 corners are not all on one side of the level; an outer-layer cell of a newly evaluated brick that holds a
    triangle activates every neighbour brick it touches, until nothing is added.  Every connected component of the surface that passes
    through a seeded brick comes out exactly as :func:`iso_surface` would give it on the dense grid; a component that lies inside
    bricks without a corner sign change is missed.

    Returns ``(verts [V,3] float32, faces [F,3] int32, edge_ids [V] int64, stats)``: vertices by brick, then edge id; faces by brick,
    cell, tet, triangle; ordering the vertices by ``edge_ids`` gives :func:`iso_surface`'s numbering.  ``stats``: ``bricks_total``,
    ``bricks_seeded``, ``bricks_active``, ``rounds`` (growth passes that added bricks), ``points_evaluated`` (corners + active bricks'
    points, apron included), ``points_dense`` (nx ny nz), ``active_bricks`` (int64 numpy, ascending) and, with ``timing=True``,
    ``times`` (seconds of the seed, band density, growth and meshing phases; each phase ends with a device synchronisation).  A
    non-finite density raises ``MofaError``."""
    nx, ny, nz = (int(v) for v in resolution)
    B = int(brick)
    level = float(level)
    if B not in BRICKS:
        raise lib.MofaError(f"band_surface: brick = {brick} (want one of {BRICKS})")
    if not np.isfinite(level):
        raise lib.MofaError(f"band_surface: the level must be finite (got {level})")
    chunk = int(chunk)
    if chunk < 1:
        raise lib.MofaError(f"band_surface: chunk = {chunk}")
    L = lib.load()
    nbytes = L.mofa_band_workspace_bytes(nx, ny, nz, B)
    if nbytes == 0:
        raise lib.MofaError(f"band_surface: grid {nx} x {ny} x {nz} with bricks of {B} is refused ((n - 1) % B == 0 and 2 <= n < 2^24 "
                            f"per axis, fewer than 2^31 brick corners)")
    lo3, st3 = _f3(lo), _f3(step)
    if not all(np.isfinite(v) for v in (*lo3, *st3)) or min(st3) <= 0:
        raise lib.MofaError(f"band_surface: lo = {list(lo3)}, step = {list(st3)} (want finite, step > 0)")
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = lib.stream()
    bx, by, bz = (nx - 1) // B, (ny - 1) // B, (nz - 1) // B
    P = (B + 1) ** 3
    times = {"seed": 0.0, "density": 0.0, "growth": 0.0, "mesh": 0.0}
    clock = [time.perf_counter()]

    def lap(phase):
        if timing:
            torch.cuda.synchronize()
            now = time.perf_counter()
            times[phase] += now - clock[0]
            clock[0] = now

    def evaluate(fill, n, out, what):
        buf = torch.empty(min(chunk, n), 3, dtype=torch.float32, device=dev)
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            fill(i, m, buf[:m])
            d = density_fn(buf[:m])
            if not torch.is_tensor(d) or d.shape != (m,) or d.dtype != torch.float32 or d.device != dev:
                raise lib.MofaError(f"band_surface: density_fn must return [{m}] float32 on {dev}, got "
                                    f"{getattr(d, 'shape', type(d))} {getattr(d, 'dtype', '')} {getattr(d, 'device', '')}")
            out[i:i + m] = d
        if verify is not None:
            verify()
        if not bool(torch.isfinite(out[:n]).all()):
            raise lib.MofaError(f"band_surface: density_fn returned non-finite values at the {what}")

    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    # seed: the brick-corner lattice
    n_corners = (bx + 1) * (by + 1) * (bz + 1)
    corner_sigma = torch.empty(n_corners, dtype=torch.float32, device=dev)
    evaluate(lambda i, m, buf: lib.check(L.mofa_band_corner_points(nx, ny, nz, B, lo3, st3, i, m, lib.ptr(buf), stream),
                                         "mofa_band_corner_points"), n_corners, corner_sigma, "brick corners")
    lib.check(L.mofa_band_seed(nx, ny, nz, B, lib.ptr(corner_sigma), level, ws.data_ptr(), counts.data_ptr(), stream), "mofa_band_seed")
    n_new, n_active = (int(v) for v in counts.cpu())
    seeded, rounds = n_new, 0
    del corner_sigma
    lap("seed")
    # rounds: evaluate the bricks just activated, grow from them
    sigma = torch.empty(max(n_active, 1) * P, dtype=torch.float32, device=dev)
    while n_new:
        base = n_active - n_new
        if sigma.numel() < n_active * P:                      # (slots of every earlier round stay where they are)
            grown = torch.empty(max(n_active, 2 * sigma.numel() // P) * P, dtype=torch.float32, device=dev)
            grown[:base * P] = sigma[:base * P]
            sigma = grown
        evaluate(lambda i, m, buf: lib.check(L.mofa_band_points(nx, ny, nz, B, lo3, st3, ws.data_ptr(), n_new, i, m, lib.ptr(buf), stream),
                                             "mofa_band_points"), n_new * P, sigma[base * P:n_active * P], "band points")
        lap("density")
        lib.check(L.mofa_band_grow(nx, ny, nz, B, lib.ptr(sigma), level, ws.data_ptr(), n_new, counts.data_ptr(), stream), "mofa_band_grow")
        n_new, n_active = (int(v) for v in counts.cpu())
        rounds += n_new > 0
        lap("growth")
    stats = {"bricks_total": bx * by * bz, "bricks_seeded": seeded, "bricks_active": n_active, "rounds": rounds,
             "points_evaluated": n_corners + n_active * P, "points_dense": nx * ny * nz}
    verts = torch.empty(0, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(0, 3, dtype=torch.int32, device=dev)
    edge_ids = torch.empty(0, dtype=torch.int64, device=dev)
    bricks = torch.empty(n_active, dtype=torch.int64, device=dev)
    if n_active:
        mws = torch.empty(L.mofa_band_mesh_bytes(B, n_active), dtype=torch.uint8, device=dev)
        lib.check(L.mofa_band_count(nx, ny, nz, B, lib.ptr(sigma), level, ws.data_ptr(), n_active, mws.data_ptr(), counts.data_ptr(),
                                    bricks.data_ptr(), stream), "mofa_band_count")
        V, F = (int(v) for v in counts.cpu())
        if V > 2 ** 31 - 1 or F > 2 ** 31 - 1:
            raise lib.MofaError(f"band_surface: {V} vertices / {F} faces exceed the int32 face indices (2^31 - 1)")
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        edge_ids = torch.empty(V, dtype=torch.int64, device=dev)
        if V and F:
            lib.check(L.mofa_band_emit(nx, ny, nz, B, lo3, st3, lib.ptr(sigma), level, ws.data_ptr(), n_active, mws.data_ptr(),
                                       lib.ptr(verts), edge_ids.data_ptr(), faces.data_ptr(), stream), "mofa_band_emit")
    stats["active_bricks"] = bricks.cpu().numpy()
    lap("mesh")
    if timing:
        stats["times"] = times
    return verts, faces, edge_ids, stats


MAX_REFINE = 20      # halvings of an edge: t_m = 0.5 (t_lo + t_hi) stays exact in float32 for 23
_COUNT_NAMES = ("no_straddle", "non_finite", "refused", "zero_normal")       # MOFA_REFINE_* of include/mofanerf_hip.h


def _density_chunks(who, density_fn, pts, out, chunk):
    """out[i] = density_fn(pts[i]), asked for in calls of at most ``chunk`` points."""
    for i in range(0, pts.shape[0], chunk):
        p = pts[i:i + chunk]
        d = density_fn(p)
        if not torch.is_tensor(d) or d.shape != (p.shape[0],) or d.dtype != torch.float32 or d.device != pts.device:
            raise lib.MofaError(f"{who}: density_fn must return [{p.shape[0]}] float32 on {pts.device}, got "
                                f"{getattr(d, 'shape', type(d))} {getattr(d, 'dtype', '')} {getattr(d, 'device', '')}")
        out[i:i + p.shape[0]] = d


def refine_vertices(density_fn, edge_ids: torch.Tensor, resolution, lo, step, level, iterations, chunk, verify=None):
    """Move every vertex of :func:`iso_surface` / :func:`band_surface` along its lattice edge onto ``{density = level}`` by bisection
    (``mofa_edge_*``): ``edge_ids [V] int64`` names the edges, ``density_fn`` is :func:`band_surface`'s (same point, same bits; at most
    ``chunk`` points per call).  The two ends of every edge are evaluated (they must reproduce the grid's densities: they straddle the
    level), then ``iterations`` (0 .. 20) times the midpoint of the bracket, which replaces the end on its side of the level; the vertex is
    the linear interpolation inside the final bracket, so ``iterations = 0`` gives the extraction's own vertices bit for bit and k
    iterations place a vertex as a grid ``2^k`` times finer along the edge would.  Faces, numbering and topology are untouched.
    ``verify()``, if given, runs after each round's densities and before a kernel reads them.

    Returns ``(verts [V,3] float32, stats)``; ``stats``: ``evaluations`` ((2 + iterations) V), the final brackets ``t_lo``, ``t_hi``,
    ``s_lo``, ``s_hi`` ([V] float32 GPU) and ``bracket_width`` (2^-iterations).  Raises ``MofaError`` when an edge's ends do not straddle
    the level (``density_fn`` did not reproduce the grid's bits), when a density is not finite, or when an edge id is not an edge of the
    grid."""
    who = "refine_vertices"
    nx, ny, nz = (int(v) for v in resolution)
    level, k, chunk = float(level), int(iterations), int(chunk)
    if not np.isfinite(level):
        raise lib.MofaError(f"{who}: the level must be finite (got {level})")
    if not 0 <= k <= MAX_REFINE or k != iterations:
        raise lib.MofaError(f"{who}: iterations = {iterations} (want an integer 0 .. {MAX_REFINE})")
    if chunk < 1:
        raise lib.MofaError(f"{who}: chunk = {chunk}")
    if not torch.is_tensor(edge_ids) or not edge_ids.is_cuda or edge_ids.dtype != torch.int64 or edge_ids.dim() != 1 or not edge_ids.is_contiguous():
        raise lib.MofaError(f"{who}: want contiguous int64 edge_ids [V] on the GPU; there is no CPU path")
    dev, V = edge_ids.device, int(edge_ids.shape[0])
    lo3, st3 = _f3(lo), _f3(step)
    L = lib.load()
    with torch.cuda.device(dev):
        stream = lib.stream()
        t_lo, t_hi, s_lo, s_hi, s_a, s_b = (torch.empty(V, dtype=torch.float32, device=dev) for _ in range(6))
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        stats = {"evaluations": (2 + k) * V, "t_lo": t_lo, "t_hi": t_hi, "s_lo": s_lo, "s_hi": s_hi, "bracket_width": 2.0 ** -k}
        if V == 0:
            return verts, stats
        counts = torch.zeros(len(_COUNT_NAMES), dtype=torch.int64, device=dev)
        buf = torch.zeros(min(chunk, V), 3, dtype=torch.float32, device=dev)      # (zeros: a refused edge's point is never written)

        def evaluate(mode, out):
            for i in range(0, V, chunk):
                m = min(chunk, V - i)
                lib.check(L.mofa_edge_points(nx, ny, nz, lo3, st3, edge_ids.data_ptr(), lib.ptr(t_lo), lib.ptr(t_hi), i, m, mode, lib.ptr(buf),
                                             counts.data_ptr(), stream), "mofa_edge_points")
                _density_chunks(who, density_fn, buf[:m], out[i:i + m], chunk)
            if verify is not None:
                verify()

        def verdict(what):
            c = dict(zip(_COUNT_NAMES, (int(v) for v in counts.cpu())))
            if c["refused"]:
                raise lib.MofaError(f"{who}: {c['refused']} edge ids are not edges of the {nx} x {ny} x {nz} grid")
            if c["non_finite"]:
                raise lib.MofaError(f"{who}: density_fn returned {c['non_finite']} non-finite values at the {what}")
            if c["no_straddle"]:
                raise lib.MofaError(f"{who}: the ends of {c['no_straddle']} of {V} edges do not straddle the level {level}: density_fn did "
                                    f"not reproduce the densities the mesh was extracted from")

        evaluate(0, s_a)
        evaluate(1, s_b)
        lib.check(L.mofa_edge_bracket_init(lib.ptr(s_a), lib.ptr(s_b), level, V, lib.ptr(t_lo), lib.ptr(t_hi), lib.ptr(s_lo), lib.ptr(s_hi),
                                           counts.data_ptr(), stream), "mofa_edge_bracket_init")
        verdict("edge ends")
        for _ in range(k):
            evaluate(2, s_a)
            lib.check(L.mofa_edge_bracket_update(lib.ptr(s_a), level, V, lib.ptr(t_lo), lib.ptr(t_hi), lib.ptr(s_lo), lib.ptr(s_hi),
                                                 counts.data_ptr(), stream), "mofa_edge_bracket_update")
        if k:
            verdict("bracket midpoints")
        lib.check(L.mofa_edge_place(nx, ny, nz, lo3, st3, edge_ids.data_ptr(), lib.ptr(t_lo), lib.ptr(t_hi), lib.ptr(s_lo), lib.ptr(s_hi), level,
                                    V, lib.ptr(verts), counts.data_ptr(), stream), "mofa_edge_place")
    return verts, stats


def density_normals(density_fn, verts: torch.Tensor, step, h_frac: float = 0.5, chunk: int = 1 << 16, verify=None):
    """Unit normals of the density field at ``verts [V,3]`` from central differences (``mofa_fd_points`` / ``mofa_fd_normals``):
    ``g_a = (density(v + h_a e_a) - density(v - h_a e_a)) / (2 h_a)`` with ``h = h_frac * step`` per axis (float32), ``n = -g / |g|`` —
    toward lower density, like the face normals.  ``density_fn`` as for :func:`refine_vertices` (6 V evaluations, at most ``chunk`` points
    per call); ``verify()`` runs after each group's densities.  Returns ``(normals [V,3] float32, n_zero)``: a vertex whose gradient is
    zero or not finite gets (0, 0, 0) and is counted."""
    who = "density_normals"
    lib.ptr(verts)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise lib.MofaError(f"{who}: want verts [V,3], got {tuple(verts.shape)}")
    chunk, h_frac = int(chunk), float(h_frac)
    if chunk < 1:
        raise lib.MofaError(f"{who}: chunk = {chunk}")
    h = (np.float32(h_frac) * np.asarray(step, dtype=np.float32).reshape(3)).astype(np.float32)
    if not (np.isfinite(h).all() and (h > 0).all()):
        raise lib.MofaError(f"{who}: h = h_frac * step = {h.tolist()} (want finite and > 0)")
    h3 = _f3(h)
    dev, V = verts.device, int(verts.shape[0])
    normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
    if V == 0:
        return normals, 0
    L = lib.load()
    with torch.cuda.device(dev):
        stream = lib.stream()
        counts = torch.zeros(len(_COUNT_NAMES), dtype=torch.int64, device=dev)
        group = min(max(chunk // 6, 1), V)                     # vertices per launch: 6 points each
        pts = torch.empty(6 * group, 3, dtype=torch.float32, device=dev)
        s = torch.empty(6 * group, dtype=torch.float32, device=dev)
        for i in range(0, V, group):
            m = min(group, V - i)
            lib.check(L.mofa_fd_points(lib.ptr(verts), h3, i, m, lib.ptr(pts), stream), "mofa_fd_points")
            _density_chunks(who, density_fn, pts[:6 * m], s[:6 * m], chunk)
            if verify is not None:
                verify()
            lib.check(L.mofa_fd_normals(lib.ptr(s), h3, m, lib.ptr(normals[i:i + m]), counts.data_ptr(), stream), "mofa_fd_normals")
        n_zero = int(counts.cpu()[_COUNT_NAMES.index("zero_normal")])
    return normals, n_zero


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Area-weighted unit vertex normals (the sum of the adjacent faces' cross products, normalised); a vertex whose faces all have
    zero area gets (0, 0, 0)."""
    f = faces.long()
    v0, v1, v2 = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    fn = torch.linalg.cross(v1 - v0, v2 - v0)
    n = torch.zeros_like(verts)
    for c in range(3):
        n.index_add_(0, f[:, c], fn)
    return torch.nn.functional.normalize(n, dim=-1)


INT32_MAX = 2 ** 31 - 1
# hook + compress passes of components() before it gives up: a guard against a faulty kernel, not a tuning knob (a 100,003-vertex strip
# with random numbering needs 12, lattice-ordered iso-surfaces 3-4: about 0.7 log2 V)
MAX_CC_PASSES = 64
CC_CHUNK = 1024      # elements per first-level reduction of a component's box (vertices) and area / volume (faces)


def _mesh_tensors(who, verts, faces):
    """(V, F, device) of a mesh on the GPU: contiguous float32 verts [V,3], contiguous int32 faces [F,3], V, F < 2^31."""
    lib.ptr(verts)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise lib.MofaError(f"{who}: want verts [V,3], got {tuple(verts.shape)}")
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got CPU faces); there is no CPU fallback")
    if faces.dtype != torch.int32 or not faces.is_contiguous() or faces.dim() != 2 or faces.shape[1] != 3:
        raise lib.MofaError(f"{who}: want contiguous int32 faces [F,3], got {faces.dtype} {tuple(faces.shape)} contiguous={faces.is_contiguous()}")
    if faces.device != verts.device:
        raise lib.MofaError(f"{who}: verts on {verts.device}, faces on {faces.device}")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if V > INT32_MAX or F > INT32_MAX:
        raise lib.MofaError(f"{who}: {V} vertices / {F} faces exceed the int32 indices (2^31 - 1)")
    return V, F, verts.device


def _cc_runs(counts, offset):
    """For elements sorted by label, ``counts [C]`` per label, the first label's run starting at ``offset``: (run [C+1], the run ends;
    first_chunk [C+1], the index of each label's first chunk of CC_CHUNK elements; chunks per label [C])."""
    n = counts.shape[0]
    run = torch.full((n + 1,), int(offset), dtype=torch.int64, device=counts.device)
    run[1:] += torch.cumsum(counts, 0)
    per_label = (counts + (CC_CHUNK - 1)) // CC_CHUNK
    first_chunk = torch.zeros(n + 1, dtype=torch.int64, device=counts.device)
    first_chunk[1:] = torch.cumsum(per_label, 0)
    return run, first_chunk, per_label


def _cc_chunks(run, first_chunk, per_label, n_chunks):
    """(start [n_chunks], end [n_chunks]) of every chunk: label l's j-th chunk is run[l] + CC_CHUNK j .. , cut at run[l + 1]."""
    i64 = dict(dtype=torch.int64, device=run.device)
    label_of = torch.repeat_interleave(torch.arange(per_label.shape[0], **i64), per_label, output_size=n_chunks)
    start = run[label_of] + CC_CHUNK * (torch.arange(n_chunks, **i64) - first_chunk[label_of])
    return start, torch.minimum(start + CC_CHUNK, run[label_of + 1])


def components(verts: torch.Tensor, faces: torch.Tensor, timing: bool = False) -> dict:
    """Connected components of a triangle mesh on the GPU (``mofa_cc_*``): two faces belong to one component when they share a vertex
    index (a degenerate face ``(a, a, b)`` still joins a and b).  Components are numbered 0 .. C-1 in the order of their smallest vertex
    index; a vertex no face references gets label -1 and belongs to none.  Returns a dict: ``n_components`` (int), ``vertex_labels [V]
    int32``, ``face_labels [F] int32`` (the label of the face's first vertex), ``n_verts`` / ``n_faces`` ``[C] int64``, ``area [C]
    float64`` (sum of 0.5 |(v1 - v0) x (v2 - v0)|), ``volume [C] float64`` (sum of v0 . (v1 x v2) / 6, signed: with the orientation of
    :func:`iso_surface` a solid blob is positive, a cavity negative), ``bbox [C,2,3] float32`` (exact min and max), ``unreferenced`` (int)
    and ``passes`` (hook + compress passes run, the last of which changed nothing).  Tensors are on the mesh's device.

    The face indices are validated first (one host read): an index outside [0, V) raises ``MofaError`` with the count and nothing else
    is launched.  Labels come from integer ``atomicMin`` only, the boxes and the sums from fixed-order two-level reductions over the vertices
    and the faces sorted by label, so the same mesh gives the same bytes every time.  ``V == 0`` or ``F == 0`` gives zero components without a launch.
    ``timing=True`` adds ``times``: seconds of the ``validate``, ``labels`` (the passes), ``number`` (dense labels and counts), ``bbox``
    (sort, the two-level min / max) and ``sums`` (terms, sort, the two-level sums) phases, each ended by a device synchronisation."""
    who = "components"
    V, F, dev = _mesh_tensors(who, verts, faces)
    if V == 0 or F == 0:
        return {"n_components": 0, "vertex_labels": torch.full((V,), -1, dtype=torch.int32, device=dev),
                "face_labels": torch.full((F,), -1, dtype=torch.int32, device=dev), "n_verts": torch.zeros(0, dtype=torch.int64, device=dev),
                "n_faces": torch.zeros(0, dtype=torch.int64, device=dev), "area": torch.zeros(0, dtype=torch.float64, device=dev),
                "volume": torch.zeros(0, dtype=torch.float64, device=dev), "bbox": torch.zeros(0, 2, 3, dtype=torch.float32, device=dev),
                "unreferenced": V, "passes": 0}
    L = lib.load()
    i64 = dict(dtype=torch.int64, device=dev)
    times, clock = {}, [time.perf_counter()]

    def lap(phase):
        if timing:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            times[phase] = now - clock[0]
            clock[0] = now

    with torch.cuda.device(dev):
        stream = lib.stream()
        lap("start")
        counts = torch.zeros(1, **i64)
        lib.check(L.mofa_cc_validate(faces.data_ptr(), F, V, counts.data_ptr(), stream), "mofa_cc_validate")
        bad = int(counts.cpu()[0])
        if bad:
            raise lib.MofaError(f"{who}: {bad} of the {3 * F} face indices lie outside [0, {V})")
        lap("validate")
        # labels: parent[v] = the smallest vertex index of v's component
        parent = torch.empty(V, dtype=torch.int32, device=dev)
        changed = torch.zeros(MAX_CC_PASSES, **i64)                  # one word per pass: nothing to zero in between
        lib.check(L.mofa_cc_init(parent.data_ptr(), V, stream), "mofa_cc_init")
        passes = 0
        while True:
            if passes == MAX_CC_PASSES:
                raise lib.MofaError(f"{who}: the labels of {V} vertices / {F} faces did not settle in {MAX_CC_PASSES} passes")
            lib.check(L.mofa_cc_hook(faces.data_ptr(), F, V, parent.data_ptr(), changed.data_ptr() + 8 * passes, stream), "mofa_cc_hook")
            lib.check(L.mofa_cc_compress(parent.data_ptr(), V, stream), "mofa_cc_compress")
            passes += 1
            if not int(changed[passes - 1].cpu()):                   # (one 8-byte read per pass)
                break
        lap("labels")
        # dense labels: rank of the root among the referenced roots
        referenced = torch.zeros(V, dtype=torch.bool, device=dev)
        referenced[faces.reshape(-1).long()] = True
        is_root = (parent == torch.arange(V, dtype=torch.int32, device=dev)) & referenced
        rank = torch.cumsum(is_root, 0, dtype=torch.int64) - 1
        n_c, n_ref = (int(v) for v in torch.stack([rank[-1] + 1, referenced.sum()]).cpu())
        vertex_labels = torch.where(referenced, rank[parent.long()], -1).to(torch.int32)
        face_labels = vertex_labels[faces[:, 0].long()].contiguous()
        n_verts = torch.bincount(vertex_labels[referenced].long(), minlength=n_c)
        n_faces = torch.bincount(face_labels.long(), minlength=n_c)
        lap("number")
        # statistics: the elements stably sorted by label, every label's run reduced in chunks of CC_CHUNK elements from its start, then
        # every label's chunks — one workgroup per chunk / per label, a fixed order inside each, no atomics
        f_run, f_first, f_count = _cc_runs(n_faces, 0)
        v_run, v_first, v_count = _cc_runs(n_verts, V - n_ref)                      # (sorted by label, the unreferenced -1 come first)
        nf_chunks, f_most, nv_chunks, v_most = (int(v) for v in torch.stack([f_first[-1], f_count.max(), v_first[-1], v_count.max()]).cpu())
        order = torch.sort(vertex_labels, stable=True).indices
        start, end = _cc_chunks(v_run, v_first, v_count, nv_chunks)
        boxes = torch.empty(nv_chunks, 2, 3, dtype=torch.float32, device=dev)
        lib.check(L.mofa_cc_seg_minmax(lib.ptr(verts), 0, order.data_ptr(), V, start.data_ptr(), end.data_ptr(), nv_chunks, CC_CHUNK,
                                       lib.ptr(boxes), stream), "mofa_cc_seg_minmax")
        bbox = torch.empty(n_c, 2, 3, dtype=torch.float32, device=dev)
        start, end = v_first[:-1].contiguous(), v_first[1:].contiguous()
        lib.check(L.mofa_cc_seg_minmax(lib.ptr(boxes), 1, None, nv_chunks, start.data_ptr(), end.data_ptr(), n_c, v_most, lib.ptr(bbox), stream),
                  "mofa_cc_seg_minmax")
        lap("bbox")
        terms = torch.empty(F, 2, dtype=torch.float64, device=dev)
        lib.check(L.mofa_cc_face_terms(lib.ptr(verts), faces.data_ptr(), F, V, terms.data_ptr(), stream), "mofa_cc_face_terms")
        order = torch.sort(face_labels, stable=True).indices
        start, end = _cc_chunks(f_run, f_first, f_count, nf_chunks)
        partial = torch.empty(nf_chunks, 2, dtype=torch.float64, device=dev)
        lib.check(L.mofa_cc_seg_sum(terms.data_ptr(), order.data_ptr(), F, start.data_ptr(), end.data_ptr(), nf_chunks, CC_CHUNK,
                                    partial.data_ptr(), stream), "mofa_cc_seg_sum")
        sums = torch.empty(n_c, 2, dtype=torch.float64, device=dev)
        start, end = f_first[:-1].contiguous(), f_first[1:].contiguous()
        lib.check(L.mofa_cc_seg_sum(partial.data_ptr(), None, nf_chunks, start.data_ptr(), end.data_ptr(), n_c, f_most, sums.data_ptr(), stream),
                  "mofa_cc_seg_sum")
        lap("sums")
    out = {"n_components": n_c, "vertex_labels": vertex_labels, "face_labels": face_labels, "n_verts": n_verts, "n_faces": n_faces,
           "area": sums[:, 0].contiguous(), "volume": sums[:, 1].contiguous(), "bbox": bbox, "unreferenced": V - n_ref, "passes": passes}
    if timing:
        times.pop("start")
        out["times"] = times
    return out


def select_components(stats: dict, keep) -> torch.Tensor:
    """A keep mask ``[C] bool`` over the components of :func:`components`: ``"largest"`` (most faces; a tie keeps the lowest label), an
    integer ``n`` (every component with ``n_faces >= n``), a callable ``keep(stats)`` that returns a mask, or the mask itself."""
    n_c, n_faces = int(stats["n_components"]), stats["n_faces"]
    dev = n_faces.device
    if isinstance(keep, str):
        if keep != "largest":
            raise lib.MofaError(f"select_components: keep = {keep!r} (want 'largest', a face count, a callable or a mask)")
        mask = torch.zeros(n_c, dtype=torch.bool, device=dev)
        if n_c:
            mask[torch.nonzero(n_faces == n_faces.max())[0, 0]] = True
        return mask
    if isinstance(keep, (int, np.integer)) and not isinstance(keep, (bool, np.bool_)):
        if keep < 0:
            raise lib.MofaError(f"select_components: keep = {keep} (a face count cannot be negative)")
        return n_faces >= int(keep)
    if callable(keep):
        keep = keep(stats)
    mask = torch.as_tensor(keep)
    if mask.dtype != torch.bool or mask.shape != (n_c,):
        raise lib.MofaError(f"select_components: want a bool mask [{n_c}], got {mask.dtype} {tuple(mask.shape)}")
    return mask.to(dev)


def keep_components(verts: torch.Tensor, faces: torch.Tensor, stats: dict, mask: torch.Tensor, *per_vertex: torch.Tensor):
    """Compact a mesh to the components ``mask [C] bool`` keeps (``stats`` of :func:`components` on the same mesh): the kept vertices in
    their old order (unreferenced vertices are dropped), the kept faces in their old order with their indices remapped
    (``mofa_cc_remap``), and any ``per_vertex`` tensors ``[V, ...]`` (edge ids, colours, normals) carried through the same map.
    Returns ``(verts, faces, *per_vertex)``; kept vertices keep their bits."""
    who = "keep_components"
    V, F, dev = _mesh_tensors(who, verts, faces)
    n_c, vl, fl = int(stats["n_components"]), stats["vertex_labels"], stats["face_labels"]
    if vl.shape != (V,) or fl.shape != (F,) or vl.device != dev:
        raise lib.MofaError(f"{who}: the statistics describe {tuple(vl.shape)} vertices / {tuple(fl.shape)} faces on {vl.device}, the mesh has "
                            f"{V} / {F} on {dev}")
    if not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.shape != (n_c,) or mask.device != dev:
        raise lib.MofaError(f"{who}: want a bool mask [{n_c}] on {dev} (select_components gives one)")
    for p in per_vertex:
        if not torch.is_tensor(p) or p.dim() < 1 or p.shape[0] != V or p.device != dev:
            raise lib.MofaError(f"{who}: want per-vertex tensors [{V}, ...] on {dev}, got {tuple(getattr(p, 'shape', ()))}")
    if n_c == 0:
        return (verts[:0], faces[:0]) + tuple(p[:0] for p in per_vertex)
    with torch.cuda.device(dev):
        vkeep = (vl >= 0) & mask[vl.clamp(min=0).long()]
        fkeep = mask[fl.long()]
        vmap = torch.where(vkeep, torch.cumsum(vkeep, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
        old = faces[fkeep].contiguous()
        new = torch.empty_like(old)
        if old.numel():
            lib.check(lib.load().mofa_cc_remap(old.data_ptr(), old.numel(), vmap.data_ptr(), V, new.data_ptr(), lib.stream()), "mofa_cc_remap")
        return (verts[vkeep], new) + tuple(p[vkeep] for p in per_vertex)


SIMP_MAX_CELLS = 2 ** 21                     # cells per axis a key can hold
_SIMP_COUNTS = ("bad_vertex", "placed_quadric", "placed_mean", "placed_first", "mean_requested", "bad_index")      # MOFA_SIMP_* of the header
_SIMP_PLACEMENTS = {"quadric": 0, "mean": 1}                                                                   # MOFA_SIMP_PLACE_*


def _simp_two_level(L, rows, ncols, perm, row_div, counts, offset, stream):
    """[C, ncols] float64: per label, the sum of its run of ``perm`` (elements sorted by label, ``counts [C]`` per label, the first run at
    ``offset``) over rows ``perm // row_div`` of ``rows [N, ncols]``: chunks of CC_CHUNK first, then each label's chunks
    (``mofa_simp_seg_sum`` twice: a fixed order and a fixed tree at both levels)."""
    run, first, per_label = _cc_runs(counts, offset)
    n_chunks, most = (int(v) for v in torch.stack([first[-1], per_label.max()]).cpu())
    start, end = _cc_chunks(run, first, per_label, n_chunks)
    partial = torch.empty(n_chunks, ncols, dtype=torch.float64, device=rows.device)
    lib.check(L.mofa_simp_seg_sum(rows.data_ptr(), ncols, perm.data_ptr(), row_div, rows.shape[0], start.data_ptr(), end.data_ptr(), n_chunks,
                                  CC_CHUNK, partial.data_ptr(), stream), "mofa_simp_seg_sum")
    out = torch.empty(counts.shape[0], ncols, dtype=torch.float64, device=rows.device)
    start, end = first[:-1].contiguous(), first[1:].contiguous()
    lib.check(L.mofa_simp_seg_sum(partial.data_ptr(), ncols, None, 1, n_chunks, start.data_ptr(), end.data_ptr(), counts.shape[0], most,
                                  out.data_ptr(), stream), "mofa_simp_seg_sum")
    return out


def _dense_ids(key):
    """Rank of every int64 key among the distinct keys (ascending), and how many there are, as a tensor."""
    uniq, inverse = torch.unique(key, sorted=True, return_inverse=True)
    return inverse, uniq.shape[0]


def simplify(verts: torch.Tensor, faces: torch.Tensor, cell, origin=None, regularize: float = 1e-3, placement: str = "quadric",
             timing: bool = False):
    """Simplify a triangle mesh on the GPU by vertex clustering with one quadric-error representative per cluster (``mofa_simp_*``;
    Rossignac-Borrel clustering, Lindstrom's placement).  ``cell`` (a float or three) is the cell size, ``origin`` the lattice's corner
    (default: the per-axis minimum of ``verts``).  Every vertex some face references falls into the cell ``floorf((x - origin) / cell)``
    (fp32); the clusters are the occupied cells, numbered by ascending key ``(q_x << 42) | (q_y << 21) | q_z``.  Each cluster sums, in
    fp64 and in a fixed order, the quadrics of the faces at its corners (un-normalised normals: area^2 weights; a face with two corners in
    a cluster counts twice there) and places its representative at the minimiser of that quadric plus ``w |x - mean|^2``,
    ``w = regularize * trace(A)``: the regularisation pulls the directions a flat or straight patch leaves free toward the cluster's
    mean and bounds the condition number by about ``1 / regularize``.  The representative is rounded to fp32 and must lie in its own cell
    (the key arithmetic on it gives the cluster's key); otherwise the mean is taken under the same test, otherwise the cluster's
    lowest-index vertex.  ``placement="mean"`` skips the solve: plain vertex clustering, the baseline.

    Faces are rewritten to cluster indices; a face with two equal indices is dropped, and among the faces with one vertex set, with p and
    q faces of the two orientations, the first ``|p - q|`` of the majority orientation are kept in face order ("fins" cancel).  That rule
    keeps ``count(a -> b) - count(b -> a)`` of every directed edge, so a closed, consistently oriented input gives a closed, consistently
    oriented output in that sense.  The output may be non-manifold and may intersect itself, as with every clustering method.  Clusters no
    kept face uses are dropped; kept vertices come in ascending key order, faces in their old order, each rotated so that its smallest
    index comes first.  No float atomics: the same mesh gives the same bytes every time.

    Returns ``(verts' [V',3] float32, faces' [F',3] int32, stats)``; ``stats``: ``n_clusters``, ``verts_in``, ``faces_in``, ``verts_out``,
    ``faces_out``, ``faces_degenerate``, ``faces_cancelled``, ``placed_quadric`` / ``placed_mean`` / ``placed_first`` (the route of every
    cluster), ``mean_requested``, ``edges_multiple`` (directed edges of the output more than one face uses), ``cluster_of [V] int32`` (the
    output vertex each input vertex went to, -1 if dropped) and, with ``timing=True``, ``times`` (seconds of the ``validate``, ``keys``,
    ``clusters``, ``sums``, ``place``, ``faces`` and ``compact`` phases, each ended by a device synchronisation).

    A face index outside the mesh raises ``MofaError`` after ``mofa_cc_validate`` and before any other kernel; a vertex that is not finite
    or lies outside the 2^21 cells per axis raises it after ``mofa_simp_keys``; so do CPU tensors and a ``cell`` or ``regularize`` that is
    not finite and positive.  ``V == 0`` or ``F == 0`` returns empty tensors without a launch.  What the method does to a trained face,
    and whether 1e-3 is the right ``regularize``, has not been measured."""
    who = "simplify"
    V, F, dev = _mesh_tensors(who, verts, faces)
    cell3 = np.asarray(cell, dtype=np.float32).reshape(-1)
    if cell3.size not in (1, 3) or not (np.isfinite(cell3).all() and (cell3 > 0).all()):
        raise lib.MofaError(f"{who}: cell = {cell} (want one or three finite sizes > 0)")
    cell3 = np.repeat(cell3, 3) if cell3.size == 1 else cell3
    regularize = float(regularize)
    if not (np.isfinite(regularize) and regularize > 0):
        raise lib.MofaError(f"{who}: regularize = {regularize} (want finite and > 0: the flat patches of any real mesh make A singular)")
    if placement not in _SIMP_PLACEMENTS:
        raise lib.MofaError(f"{who}: placement = {placement!r} (want 'quadric' or 'mean')")
    i64 = dict(dtype=torch.int64, device=dev)
    if V == 0 or F == 0:
        stats = dict.fromkeys(("n_clusters", "verts_out", "faces_out", "faces_degenerate", "faces_cancelled", "placed_quadric", "placed_mean",
                               "placed_first", "mean_requested", "edges_multiple"), 0)
        stats.update(verts_in=V, faces_in=F, cluster_of=torch.full((V,), -1, dtype=torch.int32, device=dev))
        return verts[:0], faces[:0], stats
    L = lib.load()
    times, clock = {}, [time.perf_counter()]

    def lap(phase):
        if timing:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            times[phase] = now - clock[0]
            clock[0] = now

    with torch.cuda.device(dev):
        stream = lib.stream()
        lap("start")
        bad = torch.zeros(1, **i64)
        lib.check(L.mofa_cc_validate(faces.data_ptr(), F, V, bad.data_ptr(), stream), "mofa_cc_validate")
        n_bad = int(bad.cpu()[0])
        if n_bad:
            raise lib.MofaError(f"{who}: {n_bad} of the {3 * F} face indices lie outside [0, {V})")
        lap("validate")
        org3 = verts.amin(0).cpu().numpy() if origin is None else np.asarray(origin, dtype=np.float32).reshape(-1)
        if org3.size != 3 or not np.isfinite(org3).all():
            raise lib.MofaError(f"{who}: origin = {org3.tolist()} (want three finite coordinates; the default is the vertices' minimum)")
        o3, c3 = _f3(org3), _f3(cell3)
        counts = torch.zeros(len(_SIMP_COUNTS), **i64)
        key = torch.empty(V, **i64)
        lib.check(L.mofa_simp_keys(lib.ptr(verts), V, o3, c3, key.data_ptr(), counts.data_ptr(), stream), "mofa_simp_keys")
        n_bad = int(counts.cpu()[0])
        if n_bad:
            raise lib.MofaError(f"{who}: {n_bad} of the {V} vertices are not finite or lie outside the {SIMP_MAX_CELLS} cells per axis from "
                                f"origin {org3.tolist()} with cell {cell3.tolist()}")
        lap("keys")
        # clusters: the occupied cells of the referenced vertices, numbered by ascending key
        flat = faces.reshape(-1).long()
        referenced = torch.zeros(V, dtype=torch.bool, device=dev)
        referenced[flat] = True
        cluster_keys, inverse = torch.unique(key[referenced], sorted=True, return_inverse=True)
        n_c = int(cluster_keys.shape[0])
        cluster = torch.full((V,), -1, **i64)
        cluster[referenced] = inverse
        cluster32 = cluster.to(torch.int32)
        lap("clusters")
        # sums: (x, y, z, 1) over each cluster's vertices and the quadrics over its corners, both stably sorted by cluster
        order = torch.sort(cluster, stable=True).indices                              # (the unreferenced -1 come first)
        n_verts = torch.bincount(inverse, minlength=n_c)
        n_ref = int(inverse.shape[0])
        rows = torch.cat([verts.double(), torch.ones(V, 1, dtype=torch.float64, device=dev)], 1).contiguous()
        vsum = _simp_two_level(L, rows, 4, order, 1, n_verts, V - n_ref, stream)
        first = order[(V - n_ref) + torch.cumsum(n_verts, 0) - n_verts].to(torch.int32)       # a stable sort: each run starts at its lowest index
        qsum = None
        if placement == "quadric":
            quadrics = torch.empty(F, 10, dtype=torch.float64, device=dev)
            lib.check(L.mofa_simp_corner_quadrics(lib.ptr(verts), faces.data_ptr(), F, V, quadrics.data_ptr(), counts.data_ptr(), stream),
                      "mofa_simp_corner_quadrics")
            corner = cluster[flat]
            perm = torch.sort(corner, stable=True).indices
            qsum = _simp_two_level(L, quadrics, 10, perm, 3, torch.bincount(corner, minlength=n_c), 0, stream)
            del quadrics, perm, corner
        lap("sums")
        rep = torch.empty(n_c, 3, dtype=torch.float32, device=dev)
        lib.check(L.mofa_simp_place(None if qsum is None else qsum.data_ptr(), vsum.data_ptr(), cluster_keys.data_ptr(), first.data_ptr(),
                                    lib.ptr(verts), V, n_c, o3, c3, regularize, _SIMP_PLACEMENTS[placement], lib.ptr(rep), counts.data_ptr(),
                                    stream), "mofa_simp_place")
        lap("place")
        # faces: cluster indices in canonical rotation; degenerate faces go, fins cancel
        rot = torch.empty(F, 3, dtype=torch.int32, device=dev)
        degenerate = torch.empty(F, dtype=torch.uint8, device=dev)
        lib.check(L.mofa_simp_faces(faces.data_ptr(), F, V, cluster32.data_ptr(), n_c, rot.data_ptr(), degenerate.data_ptr(), counts.data_ptr(),
                                    stream), "mofa_simp_faces")
        alive = torch.nonzero(degenerate == 0)[:, 0]
        tri = rot[alive].long()
        n_alive = int(tri.shape[0])
        keep = torch.ones(n_alive, dtype=torch.bool, device=dev)
        if n_alive:
            lo, hi = torch.minimum(tri[:, 1], tri[:, 2]), torch.maximum(tri[:, 1], tri[:, 2])
            pair, _ = _dense_ids(tri[:, 0] * (1 << 31) + lo)                         # (indices < 2^31: the products fit 62 bits)
            group, n_groups = _dense_ids(pair * (1 << 31) + hi)
            k = 2 * group + (tri[:, 1] > tri[:, 2]).long()                           # the vertex set and the orientation
            by_k = torch.sort(k, stable=True).indices
            count = torch.bincount(k, minlength=2 * n_groups)
            begin = torch.cumsum(count, 0) - count
            rank = torch.empty(n_alive, **i64)
            rank[by_k] = torch.arange(n_alive, **i64) - begin[k[by_k]]
            keep = rank < count[k] - count[k ^ 1]
        kept = rot[alive[keep]].contiguous()
        lap("faces")
        # compaction: the clusters a kept face uses, in key order
        used = torch.zeros(n_c, dtype=torch.bool, device=dev)
        used[kept.reshape(-1).long()] = True
        vmap = torch.where(used, torch.cumsum(used, 0, dtype=torch.int32) - 1, -1).to(torch.int32)
        out_f = torch.empty_like(kept)
        if kept.numel():
            lib.check(L.mofa_cc_remap(kept.data_ptr(), kept.numel(), vmap.data_ptr(), n_c, out_f.data_ptr(), stream), "mofa_cc_remap")
        out_v = rep[used]
        cluster_of = torch.where(referenced, vmap[cluster.clamp(min=0)], -1).to(torch.int32)
        multiple = 0
        if out_f.shape[0]:
            f2 = out_f.long()
            edges = torch.cat([f2[:, 0] * (1 << 31) + f2[:, 1], f2[:, 1] * (1 << 31) + f2[:, 2], f2[:, 2] * (1 << 31) + f2[:, 0]])
            multiple = (torch.unique(edges, return_counts=True)[1] > 1).sum()
        c = dict(zip(_SIMP_COUNTS, (int(v) for v in counts.cpu())))                  # the counters, read once
        lap("compact")
    if c["bad_index"]:
        raise lib.MofaError(f"{who}: {c['bad_index']} indices were out of range inside the passes (the mesh changed while it was simplified?)")
    stats = {"n_clusters": n_c, "verts_in": V, "faces_in": F, "verts_out": int(out_v.shape[0]), "faces_out": int(out_f.shape[0]),
             "faces_degenerate": F - n_alive, "faces_cancelled": n_alive - int(kept.shape[0]), "placed_quadric": c["placed_quadric"],
             "placed_mean": c["placed_mean"], "placed_first": c["placed_first"], "mean_requested": c["mean_requested"],
             "edges_multiple": int(multiple), "cluster_of": cluster_of}
    if timing:
        times.pop("start")
        stats["times"] = times
    return out_v, out_f, stats


# ---- surface distance ------------------------------------------------------------------------------------------------------------------
# closest_points' default grid: cells of DIST_GRID_FACTOR estimated face edges (edge^2 = the box's surface area / F), at most
# DIST_GRID_AUTO_CAP per axis; DIST_GRID_CAP is the most a caller may force.  The resolution changes no bit of the result;
# profiles/mesh_distance.md holds the sweep the numbers come from.
DIST_GRID_CAP = 256
DIST_GRID_AUTO_CAP = 128
DIST_GRID_FACTOR = 2.0
DIST_MAX_SUBDIV = 1024                                                                                     # MOFA_DIST_MAX_SUBDIV
_DIST_COUNTS = ("degenerate_faces", "non_finite_queries", "candidate_tests", "max_ring", "skipped_tests")       # MOFA_DIST_* of the header


def _d3(v) -> C.Array:
    return (C.c_double * 3)(*[float(x) for x in v])


def dist_grid(lo, hi, n):
    """(origin [3], cell [3], slack [3]) in float64 of closest_points' grid of ``n`` cells over the box ``lo .. hi``: ``cell = (hi - lo) / n``
    (1 on an axis of no extent: everything falls into its cell 0) and ``slack = 2^-40 (|origin| + n cell)``, what the query's termination
    bound gives away to the rounding of the cell arithmetic."""
    origin = np.asarray(lo, dtype=np.float64).reshape(3)
    extent = np.asarray(hi, dtype=np.float64).reshape(3) - origin
    nn = np.asarray(n, dtype=np.float64).reshape(3)
    cell = np.where(extent > 0, extent / nn, 1.0)
    return origin, cell, 2.0 ** -40 * (np.abs(origin) + nn * cell)


def default_dist_grid(lo, hi, F: int):
    """The resolution closest_points picks for ``F`` faces in the box ``lo .. hi``: ``ceil(extent / h)`` cells per axis, ``h`` =
    DIST_GRID_FACTOR sqrt(the box's surface area / F), clamped to 1 .. DIST_GRID_AUTO_CAP."""
    e = np.asarray(hi, dtype=np.float64).reshape(3) - np.asarray(lo, dtype=np.float64).reshape(3)
    area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2])
    if not (F > 0 and area > 0 and np.isfinite(area)):
        return (1, 1, 1)
    h = DIST_GRID_FACTOR * np.sqrt(area / F)
    return tuple(int(v) for v in np.clip(np.ceil(e / h), 1, DIST_GRID_AUTO_CAP))


def _query_points(who, points, dev):
    lib.ptr(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise lib.MofaError(f"{who}: want points [N,3], got {tuple(points.shape)}")
    if points.device != dev:
        raise lib.MofaError(f"{who}: points on {points.device}, the mesh on {dev}")
    if points.shape[0] > INT32_MAX:
        raise lib.MofaError(f"{who}: {points.shape[0]} points exceed the int32 indices (2^31 - 1)")
    return int(points.shape[0])


def _max_distance(who, max_distance) -> float:
    if max_distance is None:
        return float("inf")
    m = float(max_distance)
    if not m > 0:
        raise lib.MofaError(f"{who}: max_distance = {max_distance} (want > 0, or None for unbounded)")
    return m


def closest_points(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, grid=None, max_distance=None) -> dict:
    """The exact closest point of the triangle mesh ``(verts [V,3] float32, faces [F,3] int32)`` to every one of ``points [N,3] float32``, on
    the GPU (``mofa_dist_*``).  Returns a dict: ``distance [N] float32``, ``d2 [N] float64`` (squared), ``face [N] int32`` (the winning
    face), ``closest [N,3] float32``, ``bary [N,3] float32`` (barycentrics of the closest point on that face), ``counts`` (a dict:
    ``degenerate_faces``, ``non_finite_queries``, ``candidate_tests``, ``max_ring``, ``skipped_tests``) and ``grid`` (the resolution used).

    Point and triangle are widened to fp64 and go through Ericson's region tests in a fixed order of operations
    (include/mofanerf_hip.h); the smaller squared distance wins, among equal ones the lower face index.  The answer is therefore a function
    of the mesh and the point alone: the faces are binned into a uniform grid over the mesh's box and every query walks Chebyshev rings
    of cells around its own until a conservative bound shows that no unseen face can win or tie, and the resolution of that grid —
    ``grid``: ``None`` (``default_dist_grid``), an int or a triple, 1 .. DIST_GRID_CAP per axis — changes the time but no bit of the
    result; ``grid=1`` is brute force through the same kernel.  No float atomics: the same bytes every time.

    A face whose fp64 normal is exactly zero is degenerate: skipped and counted.  ``max_distance`` (> 0) bounds the search: a query whose
    closest face is farther gets face -1, distance ``inf`` (``closest`` / ``bary`` NaN); within the bound the bits are those of the
    unbounded call.  A query with a non-finite coordinate gets face -1 and NaN and is counted, not refused.  ``N == 0`` returns empty tensors
    without a launch; ``F == 0``, or only degenerate faces, gives face -1 and distance ``inf`` everywhere.

    Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, a face index outside the mesh (after ``mofa_cc_validate``, before any
    other kernel), a non-finite target vertex, ``max_distance`` not > 0 and a grid outside 1 .. DIST_GRID_CAP.  The distance has no sign
    here (one taken from the closest face's normal would be wrong at edges and vertices): :func:`signed_distance` adds it from the mesh's
    winding number."""
    who = "closest_points"
    V, F, dev = _mesh_tensors(who, verts, faces)
    N = _query_points(who, points, dev)
    maxd = _max_distance(who, max_distance)
    grid = _dist_grid_arg(who, grid)
    out = _dist_empty(N, dev, grid)
    if N == 0:
        return out
    if V == 0 or F == 0:
        bad = ~torch.isfinite(points).all(1)
        out["distance"][bad], out["d2"][bad] = float("nan"), float("nan")
        out["counts"]["non_finite_queries"] = int(bad.sum())
        return out
    with torch.cuda.device(dev):
        return _dist_query(points, N, verts, faces, V, F, _dist_lists(who, verts, faces, V, F, grid), maxd)


def _dist_grid_arg(who, grid):
    """closest_points' ``grid`` argument as None or a triple, checked."""
    if grid is None:
        return None
    g = np.asarray(grid).reshape(-1)
    if g.size not in (1, 3) or g.dtype.kind not in "iu" or (g < 1).any() or (g > DIST_GRID_CAP).any():
        raise lib.MofaError(f"{who}: grid = {grid!r} (want None, an integer or three, 1 .. {DIST_GRID_CAP} per axis)")
    return tuple(int(v) for v in (np.repeat(g, 3) if g.size == 1 else g))


def _dist_empty(N, dev, grid):
    return {"distance": torch.full((N,), float("inf"), dtype=torch.float32, device=dev),
            "d2": torch.full((N,), float("inf"), dtype=torch.float64, device=dev), "face": torch.full((N,), -1, dtype=torch.int32, device=dev),
            "closest": torch.full((N, 3), float("nan"), dtype=torch.float32, device=dev),
            "bary": torch.full((N, 3), float("nan"), dtype=torch.float32, device=dev), "counts": dict.fromkeys(_DIST_COUNTS, 0),
            "grid": grid if grid is not None else (1, 1, 1)}


def _dist_lists(who, verts, faces, V, F, grid):
    """The face lists of closest_points (V, F >= 1): the mesh validated, then binned at ``grid`` (None: default_dist_grid).  ``counts`` holds
    what the binning counted; every query starts from a copy of it."""
    L, dev = lib.load(), verts.device
    i64 = dict(dtype=torch.int64, device=dev)
    stream = lib.stream()
    bad = torch.zeros(1, **i64)
    lib.check(L.mofa_cc_validate(faces.data_ptr(), F, V, bad.data_ptr(), stream), "mofa_cc_validate")
    n_bad = int(bad.cpu()[0])
    if n_bad:
        raise lib.MofaError(f"{who}: {n_bad} of the {3 * F} face indices lie outside [0, {V})")
    bad.zero_()
    lib.check(L.mofa_dist_validate(lib.ptr(verts), V, bad.data_ptr(), stream), "mofa_dist_validate")
    n_bad = int(bad.cpu()[0])
    if n_bad:
        raise lib.MofaError(f"{who}: {n_bad} of the {3 * V} coordinates of the target mesh are not finite")
    box = torch.stack([verts.amin(0), verts.amax(0)]).cpu().numpy()
    if grid is None:
        grid = default_dist_grid(box[0], box[1], F)
    origin, cell, slack = dist_grid(box[0], box[1], grid)
    o3, c3, s3, n3 = _d3(origin), _d3(cell), _d3(slack), (C.c_int32 * 3)(*grid)
    n_cells = grid[0] * grid[1] * grid[2]
    counts = torch.zeros(len(_DIST_COUNTS), **i64)
    per_face = torch.empty(F, **i64)
    lib.check(L.mofa_dist_bin_count(lib.ptr(verts), faces.data_ptr(), F, V, o3, c3, s3, n3, per_face.data_ptr(), counts.data_ptr(), stream),
              "mofa_dist_bin_count")
    ends = torch.cumsum(per_face, 0)
    P = int(ends[-1].cpu())
    if P > INT32_MAX:
        raise lib.MofaError(f"{who}: the {F} faces enter {P} cells of the {grid} grid, more than 2^31 - 1: take a coarser grid")
    start = torch.zeros(n_cells + 1, dtype=torch.int32, device=dev)
    pair_face = torch.empty(P, dtype=torch.int32, device=dev)
    if P:
        offsets = (ends - per_face).contiguous()
        pair_cell = torch.empty(P, dtype=torch.int32, device=dev)
        lib.check(L.mofa_dist_bin_emit(lib.ptr(verts), faces.data_ptr(), F, V, o3, c3, s3, n3, offsets.data_ptr(), P, pair_cell.data_ptr(),
                                       pair_face.data_ptr(), stream), "mofa_dist_bin_emit")
        if n_cells > 1:
            by_cell = torch.sort(pair_cell, stable=True).indices
            pair_face = pair_face[by_cell].contiguous()
            del by_cell
        start[1:] = torch.cumsum(torch.bincount(pair_cell.long(), minlength=n_cells), 0).to(torch.int32)
        del pair_cell, offsets
    return {"grid": grid, "box": box, "origin": origin, "cell": cell, "args": (o3, c3, s3, n3), "start": start, "pair_face": pair_face, "P": P,
            "counts": counts, "n_cells": n_cells}


def _dist_query(points, N, verts, faces, V, F, b, maxd):
    """closest_points' result (N >= 1) through the lists ``b`` of :func:`_dist_lists`."""
    L, dev = lib.load(), verts.device
    out = _dist_empty(N, dev, b["grid"])
    grid, n_cells, P = b["grid"], b["n_cells"], b["P"]
    o3, c3, s3, n3 = b["args"]
    counts = b["counts"].clone()
    order = None
    if n_cells > 1:                          # queries of one cell next to each other: a wavefront's lanes walk the same neighbourhood
        t = torch.nan_to_num((points.double() - torch.from_numpy(b["origin"]).to(dev)) / torch.from_numpy(b["cell"]).to(dev), nan=0.0, posinf=0.0,
                             neginf=0.0).floor_()
        hi = torch.tensor([g - 1 for g in grid], dtype=torch.float64, device=dev)
        c = torch.minimum(torch.clamp_(t, min=0.0), hi).long()
        order = torch.argsort((c[:, 0] * grid[1] + c[:, 1]) * grid[2] + c[:, 2])
        del t, c
    lib.check(L.mofa_dist_query(lib.ptr(points), N, None if order is None else order.data_ptr(), lib.ptr(verts), V, faces.data_ptr(), F, o3, c3,
                                s3, n3, b["start"].data_ptr(), b["pair_face"].data_ptr() if P else None, P, maxd, lib.ptr(out["distance"]),
                                out["d2"].data_ptr(), out["face"].data_ptr(), lib.ptr(out["closest"]), lib.ptr(out["bary"]),
                                counts.data_ptr(), lib.stream()), "mofa_dist_query")
    out["counts"] = dict(zip(_DIST_COUNTS, (int(v) for v in counts.cpu())))
    return out


def sample_faces(verts: torch.Tensor, faces: torch.Tensor, spacing: float, max_subdiv: int = 64):
    """A deterministic quadrature of a mesh's surface (``mofa_dist_sample_*``; no random numbers): face f is cut into ``k_f^2`` congruent
    triangles, ``k_f = clamp(ceil(longest edge / spacing), 1, max_subdiv)``, and sampled at their centroids, each with weight
    ``area_f / k_f^2`` (fp64), so the weights of a face sum to its area.  Returns ``(points [S,3] float32, face_of [S] int32, weight [S]
    float64)``: the faces in their order, each face's sub-triangles in the order the header states.  Degenerate faces (a zero fp64 normal)
    emit nothing.  The same mesh gives the same bytes."""
    who = "sample_faces"
    V, F, dev = _mesh_tensors(who, verts, faces)
    spacing = float(spacing)
    if not (np.isfinite(spacing) and spacing > 0):
        raise lib.MofaError(f"{who}: spacing = {spacing} (want finite and > 0)")
    if isinstance(max_subdiv, (bool, np.bool_)) or max_subdiv != int(max_subdiv) or not 1 <= int(max_subdiv) <= DIST_MAX_SUBDIV:
        raise lib.MofaError(f"{who}: max_subdiv = {max_subdiv!r} (want an integer 1 .. {DIST_MAX_SUBDIV})")
    empty = (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
             torch.zeros(0, dtype=torch.float64, device=dev))
    if V == 0 or F == 0:
        return empty
    L = lib.load()
    with torch.cuda.device(dev):
        stream = lib.stream()
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        lib.check(L.mofa_cc_validate(faces.data_ptr(), F, V, bad.data_ptr(), stream), "mofa_cc_validate")
        n_bad = int(bad.cpu()[0])
        if n_bad:
            raise lib.MofaError(f"{who}: {n_bad} of the {3 * F} face indices lie outside [0, {V})")
        area = torch.empty(F, dtype=torch.float64, device=dev)
        k = torch.empty(F, dtype=torch.int32, device=dev)
        lib.check(L.mofa_dist_sample_count(lib.ptr(verts), faces.data_ptr(), F, V, spacing, int(max_subdiv), area.data_ptr(), k.data_ptr(), stream),
                  "mofa_dist_sample_count")
        k2 = k.long() ** 2
        ends = torch.cumsum(k2, 0)
        S = int(ends[-1].cpu())
        if S > INT32_MAX:
            raise lib.MofaError(f"{who}: spacing {spacing} asks for {S} samples, more than 2^31 - 1")
        if S == 0:
            return empty
        offsets = (ends - k2).contiguous()
        face_of = torch.repeat_interleave(torch.arange(F, dtype=torch.int32, device=dev), k2, output_size=S)
        pts = torch.empty(S, 3, dtype=torch.float32, device=dev)
        weight = torch.empty(S, dtype=torch.float64, device=dev)
        lib.check(L.mofa_dist_sample_emit(lib.ptr(verts), faces.data_ptr(), F, V, area.data_ptr(), k.data_ptr(), offsets.data_ptr(),
                                          face_of.data_ptr(), S, lib.ptr(pts), weight.data_ptr(), stream), "mofa_dist_sample_emit")
    return pts, face_of, weight


def _distance_stats(d: torch.Tensor, weight: torch.Tensor, found: torch.Tensor) -> dict:
    """mean / rms / p50 / p95 over the samples with a weight, max over all of them, of the distances ``d`` (float64) that were found."""
    nan = float("nan")
    out = {"mean": nan, "rms": nan, "max": nan, "p50": nan, "p95": nan}
    d, weight = d[found], weight[found]
    if d.numel():
        out["max"] = float(d.max())
    keep = weight > 0
    d, weight = d[keep], weight[keep]
    total = weight.sum()
    if d.numel() and float(total) > 0:
        out["mean"] = float((weight * d).sum() / total)
        out["rms"] = float(torch.sqrt((weight * (d * d)).sum() / total))
        ds, by = torch.sort(d, stable=True)
        cum = torch.cumsum(weight[by], 0)
        for name, q in (("p50", 0.5), ("p95", 0.95)):
            i = torch.searchsorted(cum, (q * total).reshape(1)).clamp_(max=ds.numel() - 1)
            out[name] = float(ds[i])
    return out


def _signed_stats(d: torch.Tensor, weight: torch.Tensor, found: torch.Tensor, inside: torch.Tensor) -> dict:
    """signed_mean / inside_fraction over the samples with a weight, max_inside / max_outside over all of them, of the distances ``d``
    (float64) that were found; ``inside`` says which of them count as negative."""
    nan = float("nan")
    out = {"signed_mean": nan, "inside_fraction": nan, "max_inside": nan, "max_outside": nan}
    d, weight, inside = d[found], weight[found], inside[found]
    if bool(inside.any()):
        out["max_inside"] = float(d[inside].max())
    if not bool(inside.all()):
        out["max_outside"] = float(d[~inside].max())
    keep = weight > 0
    d, weight, inside = d[keep], weight[keep], inside[keep]
    total = weight.sum()
    if d.numel() and float(total) > 0:
        out["signed_mean"] = float((weight * torch.where(inside, -d, d)).sum() / total)
        out["inside_fraction"] = float((weight * inside.to(torch.float64)).sum() / total)
    return out


def surface_distance(verts_a: torch.Tensor, faces_a: torch.Tensor, verts_b: torch.Tensor, faces_b: torch.Tensor, spacing: float,
                     max_distance=None, vertices: bool = True, timing: bool = False, samples: bool = False, max_subdiv: int = 64,
                     signed: bool = False) -> dict:
    """Surface distance between two triangle meshes on the GPU, both ways.  For ``a_to_b``: the quadrature samples of mesh a
    (:func:`sample_faces` with ``spacing`` and ``max_subdiv``) plus, with ``vertices=True``, the vertices a's faces reference with weight 0
    — they count in ``max`` and not in the means: a Hausdorff distance is often attained at a vertex, which no centroid reaches —
    are sent through :func:`closest_points` against mesh b.  Each direction gives ``mean`` and ``rms`` (area-weighted, fp64), ``max``,
    the weighted ``p50`` / ``p95``, ``n_samples`` and ``n_beyond`` (queries farther than ``max_distance``: left out of the statistics and
    counted) and ``counts`` (closest_points' counters); ``samples=True`` adds ``points``, ``weight``, ``distance`` (fp64, sqrt of ``d2``)
    and ``face``.  The dict also holds ``hausdorff`` (the larger of the two maxima) and ``chamfer`` (the sum of the two means), and with
    ``timing=True`` ``times``: seconds of ``sample``, ``query`` and ``stats`` per direction, each ended by a device synchronisation.
    A direction without samples, or with every sample beyond the bound, has NaN statistics.

    The distances are unsigned unless ``signed=True``: every sample then also goes through :func:`winding_number` of the other mesh (which
    must be closed: ``MofaError`` otherwise) and each direction additionally carries ``signed_mean`` (area-weighted, fp64, the distance
    counted negative where the sample lies inside the other mesh), ``inside_fraction`` (the share of the weight that lies inside),
    ``max_inside`` / ``max_outside`` (the largest distance on either side, the weight-0 vertices included; NaN when a side has no sample),
    ``open_edges`` of the target mesh (0) and, with ``samples=True``, ``inside``; ``times`` gains ``winding`` per direction.  With
    ``signed=False`` nothing new is launched and the dict is what it always was."""
    who = "surface_distance"
    _mesh_tensors(who, verts_a, faces_a)
    _mesh_tensors(who, verts_b, faces_b)
    _max_distance(who, max_distance)
    out, times = {}, {}

    def lap(name, since):
        if timing:
            torch.cuda.synchronize(verts_a.device)
            times[name] = time.perf_counter() - since
        return time.perf_counter()

    for name, (va, fa, vb, fb) in (("a_to_b", (verts_a, faces_a, verts_b, faces_b)), ("b_to_a", (verts_b, faces_b, verts_a, faces_a))):
        clock = lap("start", 0.0)
        pts, _, weight = sample_faces(va, fa, spacing, max_subdiv)
        if vertices and fa.numel():
            ref = torch.zeros(va.shape[0], dtype=torch.bool, device=va.device)
            ref[fa.reshape(-1).long()] = True
            pts = torch.cat([pts, va[ref]]).contiguous()
            weight = torch.cat([weight, torch.zeros(pts.shape[0] - weight.shape[0], dtype=torch.float64, device=va.device)])
        clock = lap(name + ".sample", clock)
        res = closest_points(pts, vb, fb, max_distance=max_distance)
        clock = lap(name + ".query", clock)
        found = res["face"] >= 0
        d = torch.sqrt(res["d2"])
        st = _distance_stats(d, weight, found)
        if signed:
            wind = winding_number(pts, vb, fb)
            clock = lap(name + ".winding", clock)
            st.update(_signed_stats(d, weight, found, wind["inside"]))
            st["open_edges"] = wind["open_edges"]
            if samples:
                st["inside"] = wind["inside"]
        st["n_samples"] = int(pts.shape[0])
        st["n_beyond"] = int((~found).sum()) - res["counts"]["non_finite_queries"]
        st["counts"], st["grid"] = res["counts"], res["grid"]
        if samples:
            st.update(points=pts, weight=weight, distance=d, face=res["face"])
        out[name] = st
        lap(name + ".stats", clock)
    out["hausdorff"] = max(out["a_to_b"]["max"], out["b_to_a"]["max"]) if not (np.isnan(out["a_to_b"]["max"]) or np.isnan(out["b_to_a"]["max"])) \
        else float("nan")
    out["chamfer"] = out["a_to_b"]["mean"] + out["b_to_a"]["mean"]
    if timing:
        times.pop("start", None)
        out["times"] = times
    return out


# winding_number's 2-D grid of face lists over the plane across the ray: cells of about WIND_GRID_FACTOR face sizes (the face size estimated
# as for closest_points), at most WIND_GRID_AUTO_CAP per axis; WIND_GRID_CAP is the most a caller may force.  The resolution changes no
# bit of the result; profiles/mesh_winding.md holds what is known about the numbers.
WIND_GRID_CAP = 2048
WIND_GRID_AUTO_CAP = 256
WIND_GRID_FACTOR = 2.0
_WIND_COUNTS = ("non_finite_queries", "flat_faces", "face_tests", "max_column")       # MOFA_WIND_* of the header


def _wind_axes(axis: int):
    return (axis + 1) % 3, (axis + 2) % 3


def wind_grid(lo, hi, n, axis: int = 2):
    """(origin [2], cell [2]) in float64 of winding_number's grid of ``n = (nu, nv)`` cells over the (u, v) sides of the box ``lo .. hi``
    (three coordinates each), ``u = (axis + 1) % 3``, ``v = (axis + 2) % 3``: ``cell = extent / n``, 1 on a side of no extent."""
    uv = list(_wind_axes(int(axis)))
    origin = np.asarray(lo, dtype=np.float64).reshape(3)[uv]
    extent = np.asarray(hi, dtype=np.float64).reshape(3)[uv] - origin
    return origin, np.where(extent > 0, extent / np.asarray(n, dtype=np.float64).reshape(2), 1.0)


def default_wind_grid(lo, hi, F: int, axis: int = 2):
    """The resolution winding_number picks for ``F`` faces in the box ``lo .. hi``: ``ceil(extent / h)`` cells on the u and on the v side,
    ``h`` = WIND_GRID_FACTOR sqrt(the box's surface area / F), clamped to 1 .. WIND_GRID_AUTO_CAP."""
    e = np.asarray(hi, dtype=np.float64).reshape(3) - np.asarray(lo, dtype=np.float64).reshape(3)
    area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2])
    if not (F > 0 and area > 0 and np.isfinite(area)):
        return (1, 1)
    h = WIND_GRID_FACTOR * np.sqrt(area / F)
    return tuple(int(v) for v in np.clip(np.ceil(e[list(_wind_axes(int(axis)))] / h), 1, WIND_GRID_AUTO_CAP))


def _open_edges(faces: torch.Tensor, V: int) -> int:
    """The directed edges (a, b) of ``faces`` (validated) with count(a -> b) != count(b -> a); 0 for a closed, consistently oriented mesh."""
    f = faces.long()
    key = torch.cat([f[:, 0] * V + f[:, 1], f[:, 1] * V + f[:, 2], f[:, 2] * V + f[:, 0]])
    uniq, count = torch.unique(key, return_counts=True)
    back = (uniq % V) * V + torch.div(uniq, V, rounding_mode="floor")
    at = torch.searchsorted(uniq, back).clamp_(max=uniq.numel() - 1)
    return int((torch.where(uniq[at] == back, count[at], torch.zeros_like(count)) != count).sum())


def _wind_args(who, axis, grid):
    if isinstance(axis, (bool, np.bool_)) or not isinstance(axis, (int, np.integer)) or not 0 <= int(axis) <= 2:
        raise lib.MofaError(f"{who}: axis = {axis!r} (want 0, 1 or 2)")
    if grid is not None:
        g = np.asarray(grid).reshape(-1)
        if g.size not in (1, 2) or g.dtype.kind not in "iu" or (g < 1).any() or (g > WIND_GRID_CAP).any():
            raise lib.MofaError(f"{who}: grid = {grid!r} (want None, an integer or two, 1 .. {WIND_GRID_CAP} per side)")
        grid = tuple(int(v) for v in (np.repeat(g, 2) if g.size == 1 else g))
    return int(axis), grid


def _wind_lists(who, verts, faces, V, F, axis, grid, require_closed):
    """Validate the mesh, count its open edges and bin its faces: what every batch of queries against it shares."""
    L = lib.load()
    dev = verts.device
    i64 = dict(dtype=torch.int64, device=dev)
    stream = lib.stream()
    bad = torch.zeros(1, **i64)
    lib.check(L.mofa_cc_validate(faces.data_ptr(), F, V, bad.data_ptr(), stream), "mofa_cc_validate")
    n_bad = int(bad.cpu()[0])
    if n_bad:
        raise lib.MofaError(f"{who}: {n_bad} of the {3 * F} face indices lie outside [0, {V})")
    bad.zero_()
    lib.check(L.mofa_dist_validate(lib.ptr(verts), V, bad.data_ptr(), stream), "mofa_dist_validate")
    n_bad = int(bad.cpu()[0])
    if n_bad:
        raise lib.MofaError(f"{who}: {n_bad} of the {3 * V} coordinates of the mesh are not finite")
    n_open = _open_edges(faces, V)
    if n_open and require_closed:
        raise lib.MofaError(f"{who}: the mesh is not closed: {n_open} directed edges have no matching opposite edge (require_closed=False "
                            "returns the ray's count, which then depends on the axis)")
    box = torch.stack([verts.amin(0), verts.amax(0)]).cpu().numpy()
    if grid is None:
        grid = default_wind_grid(box[0], box[1], F, axis)
    origin, cell = wind_grid(box[0], box[1], grid, axis)
    o2, c2, n2 = (C.c_double * 2)(*origin), (C.c_double * 2)(*cell), (C.c_int32 * 2)(*grid)
    n_cells = grid[0] * grid[1]
    counts = torch.zeros(len(_WIND_COUNTS), **i64)
    per_face = torch.empty(F, **i64)
    lib.check(L.mofa_wind_bin_count(lib.ptr(verts), faces.data_ptr(), F, V, axis, o2, c2, n2, per_face.data_ptr(), counts.data_ptr(), stream),
              "mofa_wind_bin_count")
    ends = torch.cumsum(per_face, 0)
    P = int(ends[-1].cpu())
    if P > INT32_MAX:
        raise lib.MofaError(f"{who}: the {F} faces enter {P} cells of the {grid} grid, more than 2^31 - 1: take a coarser grid")
    start = torch.zeros(n_cells + 1, dtype=torch.int32, device=dev)
    pair_face = torch.empty(P, dtype=torch.int32, device=dev)
    if P:
        offsets = (ends - per_face).contiguous()
        pair_cell = torch.empty(P, dtype=torch.int32, device=dev)
        lib.check(L.mofa_wind_bin_emit(lib.ptr(verts), faces.data_ptr(), F, V, axis, o2, c2, n2, offsets.data_ptr(), P, pair_cell.data_ptr(),
                                       pair_face.data_ptr(), stream), "mofa_wind_bin_emit")
        if n_cells > 1:
            by_cell = torch.sort(pair_cell, stable=True).indices
            pair_face = pair_face[by_cell].contiguous()
            del by_cell
        start[1:] = torch.cumsum(torch.bincount(pair_cell.long(), minlength=n_cells), 0).to(torch.int32)
        del pair_cell, offsets
    return dict(grid=grid, origin=origin, cell=cell, o2=o2, c2=c2, n2=n2, start=start, pair_face=pair_face, P=P,
                flat_faces=int(counts.cpu()[_WIND_COUNTS.index("flat_faces")]), open_edges=n_open, axis=axis)


def _wind_query(points, N, verts, faces, V, F, b):
    """(winding [N] int32, crossings [N] int32, counts) of one batch of queries against the lists ``b`` of :func:`_wind_lists`."""
    L = lib.load()
    dev = verts.device
    grid, axis = b["grid"], b["axis"]
    winding = torch.empty(N, dtype=torch.int32, device=dev)
    crossings = torch.empty(N, dtype=torch.int32, device=dev)
    counts = torch.zeros(len(_WIND_COUNTS), dtype=torch.int64, device=dev)
    order = None
    if grid[0] * grid[1] > 1:                    # queries of one column next to each other: a wavefront's lanes walk the same list
        uv = list(_wind_axes(axis))
        t = torch.nan_to_num((points[:, uv].double() - torch.from_numpy(b["origin"]).to(dev)) / torch.from_numpy(b["cell"]).to(dev), nan=0.0,
                             posinf=0.0, neginf=0.0).floor_()
        hi = torch.tensor([g - 1 for g in grid], dtype=torch.float64, device=dev)
        c = torch.minimum(torch.clamp_(t, min=0.0), hi).long()
        order = torch.argsort(c[:, 0] * grid[1] + c[:, 1])
        del t, c
    lib.check(L.mofa_wind_query(lib.ptr(points), N, None if order is None else order.data_ptr(), lib.ptr(verts), V, faces.data_ptr(), F, axis,
                                b["o2"], b["c2"], b["n2"], b["start"].data_ptr(), b["pair_face"].data_ptr() if b["P"] else None, b["P"],
                                winding.data_ptr(), crossings.data_ptr(), counts.data_ptr(), lib.stream()), "mofa_wind_query")
    c = dict(zip(_WIND_COUNTS, (int(v) for v in counts.cpu())))
    c["flat_faces"] = b["flat_faces"]
    return winding, crossings, c


def winding_number(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, axis: int = 2, grid=None, require_closed: bool = True) -> dict:
    """The integer winding number of the closed triangle mesh ``(verts [V,3] float32, faces [F,3] int32)`` around every one of ``points
    [N,3] float32``, on the GPU (``mofa_wind_*``): the signed count of the faces that the ray from the point along ``+axis`` crosses.
    Returns a dict: ``winding [N] int32``, ``crossings [N] int32`` (the faces crossed, whatever their sign), ``inside [N] bool``
    (``winding != 0``), ``counts`` (a dict: ``non_finite_queries``, ``flat_faces``, ``face_tests``, ``max_column``), ``grid`` (the
    resolution used) and ``open_edges``.

    With the orientation of the extracted meshes (normals toward lower density, a positive signed volume) a point inside a solid has
    winding +1, one in a cavity of a solid or outside 0, one inside two overlapping solids 2, one inside an inward-oriented mesh -1.  The
    arithmetic is fixed (include/mofanerf_hip.h): a ray that passes through a vertex or an edge is decided by comparisons that come out the
    same in every face sharing it, so the count is right for every point that is not within rounding of the surface itself, where the
    answer is arbitrary.  The faces are binned into a 2-D grid over the plane across the ray and a query tests the faces of its own cell
    only; the resolution — ``grid``: ``None`` (``default_wind_grid``), an int or a pair, 1 .. WIND_GRID_CAP per side — changes the time
    but no bit of the result, and ``grid=1`` is brute force through the same kernel.  No float atomics: the same bytes every time.

    ``open_edges`` is the number of directed edges (a, b) whose count differs from that of (b, a): 0 for a closed, consistently oriented
    mesh.  With ``require_closed=True`` anything else raises ``MofaError`` with the count; with ``False`` the ray's count is returned as it
    is, and for an open mesh it then depends on ``axis`` (there is no fractional winding number here).  A query with a non-finite
    coordinate gets 0 and is counted, not refused.  ``N == 0``, ``F == 0`` and ``V == 0`` return without a launch of the library: the
    winding is then 0 everywhere.

    Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, an axis outside 0 .. 2, a grid outside 1 .. WIND_GRID_CAP, a face
    index outside the mesh (after ``mofa_cc_validate``, before any other kernel) and a non-finite vertex."""
    who = "winding_number"
    V, F, dev = _mesh_tensors(who, verts, faces)
    N = _query_points(who, points, dev)
    axis, grid = _wind_args(who, axis, grid)
    out = {"winding": torch.zeros(N, dtype=torch.int32, device=dev), "crossings": torch.zeros(N, dtype=torch.int32, device=dev),
           "inside": torch.zeros(N, dtype=torch.bool, device=dev), "counts": dict.fromkeys(_WIND_COUNTS, 0),
           "grid": grid if grid is not None else (1, 1), "open_edges": 0}
    if N == 0:
        return out
    if V == 0 or F == 0:
        out["counts"]["non_finite_queries"] = int((~torch.isfinite(points).all(1)).sum())
        return out
    with torch.cuda.device(dev):
        b = _wind_lists(who, verts, faces, V, F, axis, grid, require_closed)
        out["winding"], out["crossings"], out["counts"] = _wind_query(points, N, verts, faces, V, F, b)
    out["inside"] = out["winding"] != 0
    out["grid"], out["open_edges"] = b["grid"], b["open_edges"]
    return out


def signed_distance(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, grid=None, max_distance=None, axis: int = 2) -> dict:
    """:func:`closest_points` with a sign from :func:`winding_number`: the dict of ``closest_points(points, verts, faces, grid,
    max_distance)`` — every key of it with that call's bits — plus ``winding [N] int32``, ``inside [N] bool`` (of the ray along ``axis``)
    and ``signed_distance [N] float32``: ``-distance`` where the point is inside, ``distance`` elsewhere.  A non-finite query keeps its NaN
    (and counts as outside); a query beyond ``max_distance`` gets ``-inf`` inside and ``+inf`` outside.  The mesh must be closed
    (``MofaError`` otherwise).  Within rounding of the surface the sign is arbitrary and the distance is 0 to that rounding."""
    out = closest_points(points, verts, faces, grid=grid, max_distance=max_distance)
    wind = winding_number(points, verts, faces, axis=axis)
    out["winding"], out["inside"] = wind["winding"], wind["inside"]
    out["signed_distance"] = torch.where(wind["inside"], -out["distance"], out["distance"])
    return out


def inside_grid(verts: torch.Tensor, faces: torch.Tensor, resolution, lo, step, axis: int = 2, chunk: int = 1 << 22) -> torch.Tensor:
    """``bool [nx, ny, nz]``: which sample points of the lattice ``lo + (i, j, k) * step`` (``grid_points``) lie inside the closed mesh
    (:func:`winding_number` ``!= 0`` along ``axis``), ``chunk`` points at a time against one binning of the faces: a mesh that was edited,
    simplified or scanned, back to a volume.  ``occupancy.occupancy_from_grid(inside.float(), 0.5, lo, step, dilate)`` turns the mask
    into an occupancy grid for the culled renderer: a cell is occupied when one of its eight corners is inside.  What that grid misses are
    parts of the mesh thinner than a cell that hold no lattice point; ``dilate >= 1`` covers those next to an occupied cell, nothing covers
    a thin part on its own.  A mesh that is not closed raises ``MofaError``; an empty one gives all ``False``."""
    who = "inside_grid"
    V, F, dev = _mesh_tensors(who, verts, faces)
    axis, _ = _wind_args(who, axis, None)
    res = tuple(int(n) for n in resolution)
    if len(res) != 3 or min(res) < 1 or res[0] * res[1] * res[2] > INT32_MAX:
        raise lib.MofaError(f"{who}: resolution = {resolution!r} (want three positive sizes, fewer than 2^31 points in all)")
    chunk = int(chunk)
    if chunk < 1:
        raise lib.MofaError(f"{who}: chunk = {chunk} (want >= 1)")
    total = res[0] * res[1] * res[2]
    inside = torch.zeros(total, dtype=torch.bool, device=dev)
    if V == 0 or F == 0:
        return inside.reshape(res)
    with torch.cuda.device(dev):
        b = _wind_lists(who, verts, faces, V, F, axis, None, True)
        pts = torch.empty(min(chunk, total), 3, dtype=torch.float32, device=dev)
        for first in range(0, total, chunk):
            n = min(chunk, total - first)
            grid_points(res, lo, step, first, n, pts[:n])
            inside[first:first + n] = _wind_query(pts[:n], n, verts, faces, V, F, b)[0] != 0
    return inside.reshape(res)


# ---- ray casting ------------------------------------------------------------------------------------------------------------------------
# ray_cast walks closest_points' grid (dist_grid / default_dist_grid as they are; profiles/mesh_raycast.md holds the sweep that keeps the
# default).  The resolution changes the time and the walk's counters but no bit of the result.
_RAY_COUNTS = ("degenerate_faces", "bad_rays", "face_tests", "max_slabs", "off_box")       # MOFA_RAY_* of the header
_RAY_WHICH = {"first": 0, "last": 1}                                                       # MOFA_RAY_FIRST / MOFA_RAY_LAST
_RAY_CULL = {None: 0, "back": 1, "front": 2}                                               # MOFA_RAY_CULL_*


def _ray_args(who, origins, dirs, dev, t_min, t_max, grid):
    """(N, t_min, t_max, grid) of a cast, everything checked that needs no GPU."""
    N = _query_points(who, origins, dev)
    if _query_points(who, dirs, dev) != N:
        raise lib.MofaError(f"{who}: {N} origins, {dirs.shape[0]} directions")
    t_min, t_max = float(t_min), float("inf") if t_max is None else float(t_max)
    if not t_min <= t_max:
        raise lib.MofaError(f"{who}: t_min = {t_min}, t_max = {t_max} (want t_min <= t_max, neither NaN)")
    if grid is not None:
        g = np.asarray(grid).reshape(-1)
        if g.size not in (1, 3) or g.dtype.kind not in "iu" or (g < 1).any() or (g > DIST_GRID_CAP).any():
            raise lib.MofaError(f"{who}: grid = {grid!r} (want None, an integer or three, 1 .. {DIST_GRID_CAP} per axis)")
        grid = tuple(int(v) for v in (np.repeat(g, 3) if g.size == 1 else g))
    return N, t_min, t_max, grid


def _ray_lists(who, verts, faces, V, F, grid):
    """The face lists of a cast: the mesh validated, then closest_points' binning at ``grid`` (None: default_dist_grid)."""
    L, dev = lib.load(), verts.device
    i64 = dict(dtype=torch.int64, device=dev)
    stream = lib.stream()
    bad = torch.zeros(1, **i64)
    lib.check(L.mofa_cc_validate(faces.data_ptr(), F, V, bad.data_ptr(), stream), "mofa_cc_validate")
    n_bad = int(bad.cpu()[0])
    if n_bad:
        raise lib.MofaError(f"{who}: {n_bad} of the {3 * F} face indices lie outside [0, {V})")
    bad.zero_()
    lib.check(L.mofa_dist_validate(lib.ptr(verts), V, bad.data_ptr(), stream), "mofa_dist_validate")
    n_bad = int(bad.cpu()[0])
    if n_bad:
        raise lib.MofaError(f"{who}: {n_bad} of the {3 * V} coordinates of the mesh are not finite")
    box = torch.stack([verts.amin(0), verts.amax(0)]).cpu().numpy()
    if grid is None:
        grid = default_dist_grid(box[0], box[1], F)
    origin, cell, slack = dist_grid(box[0], box[1], grid)
    o3, c3, s3, n3 = _d3(origin), _d3(cell), _d3(slack), (C.c_int32 * 3)(*grid)
    n_cells = grid[0] * grid[1] * grid[2]
    counts = torch.zeros(len(_RAY_COUNTS), **i64)
    per_face = torch.empty(F, **i64)
    lib.check(L.mofa_dist_bin_count(lib.ptr(verts), faces.data_ptr(), F, V, o3, c3, s3, n3, per_face.data_ptr(), counts.data_ptr(), stream),
              "mofa_dist_bin_count")
    ends = torch.cumsum(per_face, 0)
    P = int(ends[-1].cpu())
    if P > INT32_MAX:
        raise lib.MofaError(f"{who}: the {F} faces enter {P} cells of the {grid} grid, more than 2^31 - 1: take a coarser grid")
    start = torch.zeros(n_cells + 1, dtype=torch.int32, device=dev)
    pair_face = torch.empty(P, dtype=torch.int32, device=dev)
    if P:
        offsets = (ends - per_face).contiguous()
        pair_cell = torch.empty(P, dtype=torch.int32, device=dev)
        lib.check(L.mofa_dist_bin_emit(lib.ptr(verts), faces.data_ptr(), F, V, o3, c3, s3, n3, offsets.data_ptr(), P, pair_cell.data_ptr(),
                                       pair_face.data_ptr(), stream), "mofa_dist_bin_emit")
        if n_cells > 1:
            pair_face = pair_face[torch.sort(pair_cell, stable=True).indices].contiguous()
        start[1:] = torch.cumsum(torch.bincount(pair_cell.long(), minlength=n_cells), 0).to(torch.int32)
    return {"grid": grid, "origin": origin, "cell": cell, "args": (o3, c3, s3, n3), "start": start, "pair_face": pair_face, "P": P,
            "degenerate": int(counts.cpu()[0]), "n_cells": n_cells}


def _ray_order(origins, dirs, b, t_min):
    """A permutation that puts rays of one major axis, sign and entry cell next to each other (it changes no result)."""
    dev = origins.device
    o, d = origins.double(), dirs.double()
    kz = d.abs().argmax(1, keepdim=True)
    dz = torch.gather(d, 1, kz)
    lo = torch.from_numpy(b["origin"]).to(dev)
    size = torch.from_numpy(b["cell"] * np.asarray(b["grid"], dtype=np.float64)).to(dev)
    plane = torch.where(dz > 0, lo[kz], (lo + size)[kz])
    t_in = torch.clamp((plane - torch.gather(o, 1, kz)) / dz, min=t_min)
    p = torch.nan_to_num((o + t_in * d - lo) / torch.from_numpy(b["cell"]).to(dev), nan=0.0, posinf=0.0, neginf=0.0).floor_()
    hi = torch.tensor([g - 1 for g in b["grid"]], dtype=torch.float64, device=dev)
    c = torch.minimum(torch.clamp_(p, min=0.0), hi).long()
    key = (kz[:, 0] * 2 + (dz[:, 0] > 0)) * b["n_cells"] + (c[:, 0] * b["grid"][1] + c[:, 1]) * b["grid"][2] + c[:, 2]
    return torch.argsort(key)


def _ray_empty(N, dev, grid):
    return {"t": torch.full((N,), float("inf"), dtype=torch.float32, device=dev), "t64": torch.full((N,), float("inf"), dtype=torch.float64, device=dev),
            "face": torch.full((N,), -1, dtype=torch.int32, device=dev), "hit": torch.zeros(N, dtype=torch.bool, device=dev),
            "front": torch.zeros(N, dtype=torch.bool, device=dev), "bary": torch.full((N, 3), float("nan"), dtype=torch.float32, device=dev),
            "point": torch.full((N, 3), float("nan"), dtype=torch.float32, device=dev), "counts": dict.fromkeys(_RAY_COUNTS, 0),
            "grid": grid if grid is not None else (1, 1, 1)}


def _ray_query(origins, dirs, N, verts, faces, V, F, b, order, t_min, t_max, which, cull):
    L, dev = lib.load(), verts.device
    out = _ray_empty(N, dev, b["grid"])
    front = torch.zeros(N, dtype=torch.uint8, device=dev)
    counts = torch.zeros(len(_RAY_COUNTS), dtype=torch.int64, device=dev)
    o3, c3, s3, n3 = b["args"]
    lib.check(L.mofa_ray_query(lib.ptr(origins), lib.ptr(dirs), N, None if order is None else order.data_ptr(), lib.ptr(verts), V, faces.data_ptr(),
                               F, o3, c3, s3, n3, b["start"].data_ptr(), b["pair_face"].data_ptr() if b["P"] else None, b["P"], t_min, t_max,
                               _RAY_WHICH[which], _RAY_CULL[cull], lib.ptr(out["t"]), out["t64"].data_ptr(), out["face"].data_ptr(),
                               front.data_ptr(), lib.ptr(out["bary"]), lib.ptr(out["point"]), counts.data_ptr(), lib.stream()), "mofa_ray_query")
    out["hit"], out["front"] = out["face"] >= 0, front != 0
    out["counts"] = dict(zip(_RAY_COUNTS, (int(v) for v in counts.cpu())))
    out["counts"]["degenerate_faces"] = b["degenerate"]
    return out


def _ray_no_mesh(out, origins, dirs):
    """The result without a face to hit: misses everywhere, a bad ray NaN and counted."""
    bad = ~(torch.isfinite(origins).all(1) & torch.isfinite(dirs).all(1) & (dirs != 0).any(1))
    out["t"][bad], out["t64"][bad] = float("nan"), float("nan")
    out["counts"]["bad_rays"] = int(bad.sum())
    return out


def ray_cast(origins: torch.Tensor, dirs: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, t_min: float = 0.0, t_max=None,
             which: str = "first", cull=None, grid=None) -> dict:
    """The first or the last hit of the rays ``origins [N,3] + t dirs [N,3]`` (float32; ``dirs`` is NOT normalised, the convention of
    ``get_rays`` and of the rasteriser's depth) on the triangle mesh ``(verts [V,3] float32, faces [F,3] int32)``, on the GPU
    (``mofa_ray_query``).  Returns a dict: ``t [N] float32`` (the ray parameter: the hit is ``o + t d``), ``t64 [N] float64``, ``face [N]
    int32`` (-1: no hit), ``hit [N] bool``, ``front [N] bool`` (the ray runs against the face normal ``(b - a) x (c - a)``), ``bary [N,3]
    float32``, ``point [N,3] float32``, ``counts`` (a dict: ``degenerate_faces``, ``bad_rays``, ``face_tests``, ``max_slabs``, ``off_box``) and
    ``grid`` (the resolution used).  A miss has face -1, ``t`` / ``t64`` +inf and NaN in ``bary`` / ``point``.

    Ray and triangle are widened to fp64 and go through the watertight test of Woop, Benthin and Wald in a fixed order of operations
    (include/mofanerf_hip.h): the edge functions of a shared edge are the same bits in both faces, zeros count as inside, so no ray
    passes between two faces.  A hit counts when ``t_min <= t <= t_max`` (both ends included; ``t_max=None``: unbounded).
    ``which="first"``: the smaller ``t`` wins, ``"last"``: the larger; among equal ``t`` the lower face index.  ``cull="back"`` ignores
    hits from behind (``front`` False), ``cull="front"`` those from the front.  The box rule: a hit whose point leaves the face's own box by
    more than 2^-42 of the pair's scale is no hit (a ray nearly in the face's plane, whose weights are rounding noise); ``off_box`` counts
    the tested pairs it refused.  The answer is a function of the mesh and the ray alone: the faces are binned into closest_points' grid
    and every ray walks the slabs of cells along its major axis until a conservative bound shows that no unseen face can win or tie
    (DESIGN 3.20), and the resolution — ``grid``: ``None`` (``default_dist_grid``), an int or a triple, 1 .. DIST_GRID_CAP per axis —
    changes the time, ``face_tests``, ``max_slabs`` and ``off_box`` but no bit of the result; ``grid=1`` is brute force through the same
    kernel.  No float atomics: the same bytes every time.

    A degenerate face (fp64 normal exactly zero) is skipped and counted.  A ray with a non-finite origin or direction, or a zero
    direction, gets face -1 and NaN in ``t`` and is counted in ``bad_rays``, not refused.  ``N == 0`` returns empty tensors without a
    launch; ``V == 0``, ``F == 0`` or only degenerate faces give misses everywhere.

    Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, an unknown ``which`` / ``cull``, a grid outside 1 .. DIST_GRID_CAP,
    ``t_min > t_max`` or a NaN bound (all before anything touches the GPU), a face index outside the mesh (after ``mofa_cc_validate``,
    before any other kernel) and a non-finite vertex."""
    who = "ray_cast"
    V, F, dev = _mesh_tensors(who, verts, faces)
    N, t_min, t_max, grid = _ray_args(who, origins, dirs, dev, t_min, t_max, grid)
    if which not in _RAY_WHICH:
        raise lib.MofaError(f"{who}: which = {which!r} (want 'first' or 'last')")
    if cull not in _RAY_CULL:
        raise lib.MofaError(f"{who}: cull = {cull!r} (want None, 'back' or 'front')")
    if N == 0:
        return _ray_empty(0, dev, grid)
    if V == 0 or F == 0:
        return _ray_no_mesh(_ray_empty(N, dev, grid), origins, dirs)
    with torch.cuda.device(dev):
        b = _ray_lists(who, verts, faces, V, F, grid)
        order = _ray_order(origins, dirs, b, t_min) if b["n_cells"] > 1 else None
        return _ray_query(origins, dirs, N, verts, faces, V, F, b, order, t_min, t_max, which, cull)


def ray_bounds(origins: torch.Tensor, dirs: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, near: float, far: float, margin: float,
               grid=None) -> dict:
    """Per-ray sampling bounds that hug a mesh: two casts over ``[near, far]`` (:func:`ray_cast`, first and last, through one binning)
    and, in float32 on the returned ``t``,

        ``near [N] = max(near, t_first - margin)``,  ``far [N] = min(far, t_last + margin)``,  ``hit [N] bool``

    (``near``, ``far`` and ``margin`` rounded to float32 first, every operation a float32 one).  A ray that misses keeps the scalar
    ``near`` / ``far``.  ``counts`` holds the two casts' counters, ``grid`` the resolution.  Raises ``MofaError`` like :func:`ray_cast`, and
    for ``margin < 0`` or ``far <= near`` (or a NaN among the three)."""
    who = "ray_bounds"
    V, F, dev = _mesh_tensors(who, verts, faces)
    near, far, margin = float(near), float(far), float(margin)
    if not margin >= 0 or not far > near or not (np.isfinite(near) and np.isfinite(far) and np.isfinite(margin)):
        raise lib.MofaError(f"{who}: near = {near}, far = {far}, margin = {margin} (want finite, far > near, margin >= 0)")
    N, t_min, t_max, grid = _ray_args(who, origins, dirs, dev, near, far, grid)
    f32 = dict(dtype=torch.float32, device=dev)
    n32, f32_, m32 = torch.tensor(near, **f32), torch.tensor(far, **f32), torch.tensor(margin, **f32)
    out = {"near": n32.repeat(N), "far": f32_.repeat(N), "hit": torch.zeros(N, dtype=torch.bool, device=dev), "counts": {},
           "grid": grid if grid is not None else (1, 1, 1)}
    if N == 0 or V == 0 or F == 0:
        return out
    with torch.cuda.device(dev):
        b = _ray_lists(who, verts, faces, V, F, grid)
        order = _ray_order(origins, dirs, b, t_min) if b["n_cells"] > 1 else None
        first = _ray_query(origins, dirs, N, verts, faces, V, F, b, order, t_min, t_max, "first", None)
        last = _ray_query(origins, dirs, N, verts, faces, V, F, b, order, t_min, t_max, "last", None)
        hit = first["hit"]
        out["near"] = torch.where(hit, torch.maximum(first["t"] - m32, n32), n32)
        out["far"] = torch.where(hit, torch.minimum(last["t"] + m32, f32_), f32_)
        out["hit"], out["grid"] = hit, b["grid"]
        out["counts"] = {"first": first["counts"], "last": last["counts"]}
    return out


_TSDF_COUNTS = ("observed", "filled_inside", "filled_outside", "border")       # MOFA_TSDF_* of the header
_TSDF_UNOBSERVED = {"auto": 0, "outside": 1, "inside": 2}                      # MOFA_TSDF_UNOBSERVED_*
_TSDF_STATE = (("acc", torch.float64), ("wsum", torch.float64), ("front", torch.int32), ("behind", torch.int32))


def _tsdf_trunc(who, trunc) -> float:
    trunc = float(trunc)
    if not (np.isfinite(trunc) and trunc > 0):
        raise lib.MofaError(f"{who}: trunc = {trunc} (want finite and > 0)")
    return trunc


def tsdf_volume(resolution, lo, step, trunc, device="cuda") -> dict:
    """An empty truncated-signed-distance volume on the lattice of :func:`grid_points` (``resolution``, ``lo``, ``step`` as
    :func:`grid_spec` returns them): the state :func:`tsdf_integrate` updates frame by frame.  A dict of four zeroed GPU tensors of
    ``nx ny nz`` elements — ``acc`` (float64, the weighted sum of the truncated distances), ``wsum`` (float64, the sum of the weights),
    ``front`` (int32, the observations that entered ``acc``), ``behind`` (int32, the views in which the voxel lay behind the seen surface by
    more than ``trunc``) — plus ``resolution``, ``lo``, ``step``, ``trunc`` and ``frames`` (the frames integrated so far).  ``trunc``, the
    truncation distance in scene units, is fixed for the life of the volume.  24 bytes per voxel; refused for fewer than 2 samples on an
    axis, ``nx ny nz >= 2^31``, a ``trunc`` that is not finite and positive, or a device that is no GPU."""
    who = "tsdf_volume"
    res = tuple(int(n) for n in resolution)
    if len(res) != 3:
        raise lib.MofaError(f"{who}: resolution {resolution}: want three axes")
    lo32, step32 = (np.asarray(v, dtype=np.float32).reshape(3).copy() for v in (lo, step))
    if not (np.isfinite(lo32).all() and np.isfinite(step32).all() and (step32 > 0).all()):
        raise lib.MofaError(f"{who}: lo = {lo}, step = {step} (want finite values and step > 0)")
    trunc = _tsdf_trunc(who, trunc)
    if max(abs(n) for n in res) > INT32_MAX or lib.load().mofa_tsdf_state_bytes(*res) == 0:
        raise lib.MofaError(f"{who}: lattice {res[0]} x {res[1]} x {res[2]} is refused (>= 2 samples per axis, nx ny nz < 2^31)")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise lib.MofaError(f"{who}: the HIP path needs a GPU (got device {dev}); there is no CPU fallback")
    n = res[0] * res[1] * res[2]
    state = {name: torch.zeros(n, dtype=dtype, device=dev) for name, dtype in _TSDF_STATE}
    state.update(resolution=res, lo=lo32, step=step32, trunc=trunc, frames=0)
    return state


def _tsdf_state(who, state):
    """(resolution, device) of a volume, its tensors checked."""
    if not isinstance(state, dict) or any(k not in state for k in ("acc", "wsum", "front", "behind", "resolution", "lo", "step", "trunc")):
        raise lib.MofaError(f"{who}: want the state dict of tsdf_volume")
    res = state["resolution"]
    n = res[0] * res[1] * res[2]
    dev = state["acc"].device
    for name, dtype in _TSDF_STATE:
        t = state[name]
        if not t.is_cuda:
            raise lib.MofaError(f"the HIP path needs tensors on the GPU (got a CPU tensor as the volume's {name}); there is no CPU fallback")
        if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != (n,) or t.device != dev:
            raise lib.MofaError(f"{who}: the volume's {name} is {t.dtype} {tuple(t.shape)} on {t.device} (want contiguous {dtype} [{n}] on {dev})")
    return res, dev


def _tsdf_cameras(who, K, c2w, n_views):
    """float32 [n_cams,16] on the host: fx, fy, cx, cy and the 3 x 4 pose of one camera, or of one per frame."""
    host = lambda v: np.asarray(v.detach().cpu() if torch.is_tensor(v) else v)
    Ks, poses = host(K).astype(np.float64), host(c2w).astype(np.float32)
    Ks, poses = (Ks[None] if Ks.ndim == 2 else Ks), (poses[None] if poses.ndim == 2 else poses)
    if Ks.ndim != 3 or Ks.shape[1] < 2 or Ks.shape[2] < 3 or poses.ndim != 3 or poses.shape[1] < 3 or poses.shape[2] != 4:
        raise lib.MofaError(f"{who}: K {tuple(Ks.shape)}, c2w {tuple(poses.shape)} (want [3,3] and [3,4] / [4,4], or one of each per frame)")
    if len(Ks) not in (1, n_views) or len(poses) not in (1, n_views):
        raise lib.MofaError(f"{who}: {len(Ks)} intrinsics and {len(poses)} poses for {n_views} frames (want one, or one per frame)")
    n_cams = max(len(Ks), len(poses))
    cams = np.empty((n_cams, 16), dtype=np.float32)
    for v in range(n_cams):
        k, p = Ks[v % len(Ks)], poses[v % len(poses)]
        cams[v, :4] = (k[0, 0], k[1, 1], k[0, 2], k[1, 2])
        cams[v, 4:] = p[:3, :4].reshape(-1)
    if not np.isfinite(cams).all():
        raise lib.MofaError(f"{who}: the cameras hold non-finite values")
    return cams


def depth_frame(depth: torch.Tensor, mask: torch.Tensor, background: str = "empty") -> torch.Tensor:
    """A depth frame in the encoding :func:`tsdf_integrate` reads: ``depth`` (float32, any shape, the ray parameter of ``get_rays``) where
    ``mask`` (bool, the same shape) holds, and elsewhere ``+inf`` for ``background="empty"`` — nothing lies on that ray: the space along it
    is carved — or NaN for ``"unknown"`` — the pixel says nothing.  :func:`rasterize` marks its misses with depth 0, :func:`ray_cast`
    with ``t`` = +inf (NaN for a bad ray) and a renderer with a low ``acc``: all of them go through here with their mask.  A depth <= 0
    or NaN inside the mask stays and reads as unknown."""
    if not torch.is_tensor(depth) or not depth.is_cuda:
        raise lib.MofaError("the HIP path needs tensors on the GPU (got a CPU depth); there is no CPU fallback")
    if depth.dtype != torch.float32:
        raise lib.MofaError(f"depth_frame: want a float32 depth, got {depth.dtype}")
    if background not in ("empty", "unknown"):
        raise lib.MofaError(f"depth_frame: background = {background!r} (want 'empty' or 'unknown')")
    if not torch.is_tensor(mask) or not mask.is_cuda:
        raise lib.MofaError("the HIP path needs tensors on the GPU (got a CPU mask); there is no CPU fallback")
    if mask.dtype != torch.bool or mask.shape != depth.shape or mask.device != depth.device:
        raise lib.MofaError(f"depth_frame: depth {tuple(depth.shape)} on {depth.device}, mask {mask.dtype} {tuple(mask.shape)} on {mask.device} "
                            "(want a bool mask of the depth's shape on its device)")
    fill = float("inf") if background == "empty" else float("nan")
    return torch.where(mask, depth.detach(), torch.full((), fill, dtype=torch.float32, device=depth.device)).contiguous()


def tsdf_integrate(state: dict, depth: torch.Tensor, K, c2w, weight: Optional[torch.Tensor] = None, carve: bool = True, trunc=None) -> dict:
    """Integrate depth frames into a volume of :func:`tsdf_volume` (``mofa_tsdf_integrate``; Curless and Levoy's weighted running
    average of truncated signed distances, with silhouette carving).  ``depth`` is ``[n,H,W]`` or ``[H,W]`` float32 on the volume's device,
    in the encoding of :func:`depth_frame`: a finite positive value is the RAY PARAMETER of the pixel's ``get_rays`` ray at the surface —
    what ``Renderer.render_geometry`` (non-NDC), :func:`rasterize` and :func:`ray_cast` return —, ``+inf`` is background, and NaN, ``-inf``
    and values <= 0 are unknown.  ``K`` / ``c2w`` are one camera (``[3,3]``, ``[3,4]`` or ``[4,4]``) or one per frame; the pose is assumed
    orthonormal.  ``weight`` (the depth's shape, finite and >= 0; ``None``: 1) weighs every pixel's observation, and a zero switches it off.

    Per voxel and view, in the order of the frames and in fp64 (include/mofanerf_hip.h has every operation): the voxel is taken into the
    camera, ``t`` = its ray parameter, and the nearest pixel ``(floor(u + 0.5), floor(v + 0.5))`` is read; behind the camera or out of the
    frame the view says nothing.  With ``D`` the pixel's depth: ``sdf = D - t``; ``sdf < -trunc`` only counts the view in ``behind``;
    otherwise ``s = min(sdf / trunc, 1)`` is observed with the pixel's weight.  A background pixel observes ``s = 1`` when ``carve`` (the
    whole ray is empty) and nothing otherwise.  No atomics and a fixed order: the same frames give the same bytes, and frames streamed in
    several calls give the bytes of one call with all of them — nothing needs to hold all frames at once.  Returns ``state`` (updated in
    place; ``state["frames"]`` counts the frames).

    Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, a frame or a weight map on another device than the volume, camera counts
    that match neither 1 nor ``n``, a weight that is negative or not finite, ``H W >= 2^31`` and a ``trunc`` that differs from the
    volume's (it is fixed when the volume is made; ``None``: the volume's)."""
    who = "tsdf_integrate"
    res, dev = _tsdf_state(who, state)
    if trunc is not None and _tsdf_trunc(who, trunc) != state["trunc"]:
        raise lib.MofaError(f"{who}: trunc = {float(trunc)}, the volume was made with trunc = {state['trunc']} (it is fixed for the life of a volume)")
    lib.ptr(depth)
    if depth.dim() not in (2, 3):
        raise lib.MofaError(f"{who}: want depth [n,H,W] or [H,W], got {tuple(depth.shape)}")
    if depth.device != dev:
        raise lib.MofaError(f"{who}: the volume is on {dev}, the frames on {depth.device}")
    frames = depth.detach().reshape((-1,) + tuple(depth.shape[-2:]))
    n, H, W = (int(v) for v in frames.shape)
    if n < 1 or H < 1 or W < 1 or H * W > INT32_MAX:
        raise lib.MofaError(f"{who}: {n} frames of H = {H}, W = {W} are refused (n, H, W >= 1, H W < 2^31)")
    if weight is not None:
        lib.ptr(weight)
        if weight.device != dev or tuple(weight.shape) not in (tuple(depth.shape), (n, H, W)):
            raise lib.MofaError(f"{who}: weight {tuple(weight.shape)} on {weight.device} (want the depth's {tuple(depth.shape)} on {dev})")
        weight = weight.detach().reshape(n, H, W)
    cams = _tsdf_cameras(who, K, c2w, n)
    with torch.cuda.device(dev):
        if weight is not None and not bool((torch.isfinite(weight) & (weight >= 0)).all()):
            raise lib.MofaError(f"{who}: the weight map holds negative or non-finite values")
        table = torch.from_numpy(cams).to(dev)
        lib.check(lib.load().mofa_tsdf_integrate(*res, _f3(state["lo"]), _f3(state["step"]), state["trunc"], lib.ptr(frames), lib.ptr(weight), n, H, W,
                                                 lib.ptr(table), int(cams.shape[0]), int(bool(carve)), state["acc"].data_ptr(),
                                                 state["wsum"].data_ptr(), state["front"].data_ptr(), state["behind"].data_ptr(), lib.stream()),
                  "mofa_tsdf_integrate")
    state["frames"] = int(state.get("frames", 0)) + n
    return state


def tsdf_field(state: dict, unobserved: str = "auto", close_border: bool = True):
    """The marchable field of a volume (``mofa_tsdf_field``): ``(field [nx,ny,nz] float32, stats)``.  ``field = -(acc / wsum)`` where a
    voxel was observed — positive inside, ``{field >= 0}`` is the solid, the zero level the surface the frames show — and elsewhere by
    ``unobserved``: ``"auto"`` fills ``+1`` (inside) where the voxel was only ever seen behind a surface (``behind > 0``) and ``-1`` where
    no view saw it at all, ``"outside"`` fills ``-1`` and ``"inside"`` ``+1``.  ``close_border=True`` then sets the outermost lattice layer
    to ``-1``, so the mesh is closed where the solid reaches the volume's edge (a frontal-only capture of a head).  The field is finite,
    as :func:`iso_surface` demands.  ``stats``: ``observed``, ``filled_inside``, ``filled_outside`` (the three classes partition the
    lattice), ``border`` (the voxels the border overwrote), ``voxels`` and ``frames``; reading them is the call's one host read."""
    who = "tsdf_field"
    res, dev = _tsdf_state(who, state)
    if unobserved not in _TSDF_UNOBSERVED:
        raise lib.MofaError(f"{who}: unobserved = {unobserved!r} (want 'auto', 'outside' or 'inside')")
    L = lib.load()
    with torch.cuda.device(dev):
        field = torch.empty(res, dtype=torch.float32, device=dev)
        ws = torch.empty(L.mofa_tsdf_workspace_bytes(*res), dtype=torch.uint8, device=dev)
        counts = torch.empty(len(_TSDF_COUNTS), dtype=torch.int64, device=dev)
        lib.check(L.mofa_tsdf_field(*res, state["acc"].data_ptr(), state["wsum"].data_ptr(), state["behind"].data_ptr(), _TSDF_UNOBSERVED[unobserved],
                                    int(bool(close_border)), lib.ptr(field), ws.data_ptr(), counts.data_ptr(), lib.stream()), "mofa_tsdf_field")
        stats = dict(zip(_TSDF_COUNTS, (int(v) for v in counts.cpu())))
    stats.update(voxels=res[0] * res[1] * res[2], frames=int(state.get("frames", 0)))
    return field, stats


def tsdf_surface(state: dict, unobserved: str = "auto", close_border: bool = True):
    """``(verts [V,3] float32, faces [F,3] int32)``: :func:`iso_surface` of :func:`tsdf_field` at level 0 — the surface the integrated
    frames show, with no density level to choose.  Watertight and consistently oriented like every extraction, normals toward the
    outside: :func:`components`, :func:`simplify`, :func:`smooth`, :func:`surface_distance`, :func:`winding_number` and
    :func:`ray_cast` take it as it is."""
    field, _ = tsdf_field(state, unobserved, close_border)
    return iso_surface(field, 0.0, state["lo"], state["step"])


BAKE_MAX_CHANNELS = 16      # the channel and power limits of mofa_bake_integrate
BAKE_MAX_POWER = 8
BAKE_MAX_FILL = 10000
_BAKE_COUNTS = ("colored", "occluded", "grazing", "unseen")       # MOFA_BAKE_* of the header
_BAKE_BLEND = {"mean": 0, "best": 1}                               # MOFA_BAKE_MEAN / _BEST
_BAKE_STATE = (("csum", torch.float64, True), ("wsum", torch.float64, False), ("wbest", torch.float64, False), ("cbest", torch.float32, True),
               ("seen", torch.int32, False), ("occluded", torch.int32, False), ("grazing", torch.int32, False))


def bake_state(V: int, channels: int = 3, device="cuda") -> dict:
    """An empty colour-baking state for a mesh of ``V`` vertices: what :func:`bake_integrate` updates frame by frame.  A dict of seven
    zeroed GPU tensors — ``csum [V,C]`` (float64, the weighted colour sum), ``wsum [V]`` (float64, the weight sum), ``wbest [V]`` (float64,
    the largest weight so far), ``cbest [V,C]`` (float32, the colour of the view with the largest weight so far), ``seen``, ``occluded``
    and ``grazing [V]`` (int32: the views that entered, those in which the vertex failed the depth test, those the angle test rejected) —
    plus ``V``, ``channels`` and ``frames``.  20 C + 28 bytes per vertex; refused for ``V`` outside 0 .. 2^31 - 1, ``channels`` outside
    1 .. 16 or a device that is no GPU."""
    who = "bake_state"
    if isinstance(V, (bool, np.bool_)) or not isinstance(V, (int, np.integer)) or not 0 <= int(V) <= INT32_MAX:
        raise lib.MofaError(f"{who}: V = {V!r} (want an integer 0 .. 2^31 - 1)")
    if isinstance(channels, (bool, np.bool_)) or not isinstance(channels, (int, np.integer)) or not 1 <= int(channels) <= BAKE_MAX_CHANNELS:
        raise lib.MofaError(f"{who}: channels = {channels!r} (want an integer 1 .. {BAKE_MAX_CHANNELS})")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise lib.MofaError(f"{who}: the HIP path needs a GPU (got device {dev}); there is no CPU fallback")
    V, C_ = int(V), int(channels)
    state = {name: torch.zeros((V, C_) if per_channel else (V,), dtype=dtype, device=dev) for name, dtype, per_channel in _BAKE_STATE}
    state.update(V=V, channels=C_, frames=0)
    return state


def _bake_state(who, state):
    """(V, C, device) of a baking state, its tensors checked."""
    if not isinstance(state, dict) or any(k not in state for k in ("V", "channels") + tuple(n for n, _, _ in _BAKE_STATE)):
        raise lib.MofaError(f"{who}: want the state dict of bake_state")
    V, C_ = int(state["V"]), int(state["channels"])
    if not (0 <= V <= INT32_MAX and 1 <= C_ <= BAKE_MAX_CHANNELS):
        raise lib.MofaError(f"{who}: the state has V = {V}, channels = {C_} (want 0 .. 2^31 - 1 and 1 .. {BAKE_MAX_CHANNELS})")
    dev = state["csum"].device if torch.is_tensor(state["csum"]) else None
    for name, dtype, per_channel in _BAKE_STATE:
        t = state[name]
        if not torch.is_tensor(t) or not t.is_cuda:
            raise lib.MofaError(f"the HIP path needs tensors on the GPU (got a CPU tensor as the state's {name}); there is no CPU fallback")
        shape = (V, C_) if per_channel else (V,)
        if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != shape or t.device != dev:
            raise lib.MofaError(f"{who}: the state's {name} is {t.dtype} {tuple(t.shape)} on {t.device} (want contiguous {dtype} {list(shape)} on {dev})")
    return V, C_, dev


def _bake_params(who, depth_tol, cos_min, power):
    """bake_integrate's parameters, checked before anything touches the GPU."""
    try:
        depth_tol, cos_min = float(depth_tol), float(cos_min)
    except (TypeError, ValueError):
        raise lib.MofaError(f"{who}: depth_tol = {depth_tol!r}, cos_min = {cos_min!r} (want numbers)") from None
    if not (np.isfinite(depth_tol) and depth_tol >= 0):
        raise lib.MofaError(f"{who}: depth_tol = {depth_tol} (want finite and >= 0)")
    if not 0.0 <= cos_min < 1.0:                                              # (NaN fails both comparisons)
        raise lib.MofaError(f"{who}: cos_min = {cos_min} (want 0 <= cos_min < 1)")
    if isinstance(power, (bool, np.bool_)) or not isinstance(power, (int, np.integer)) or not 0 <= int(power) <= BAKE_MAX_POWER:
        raise lib.MofaError(f"{who}: power = {power!r} (want an integer 0 .. {BAKE_MAX_POWER})")
    return depth_tol, cos_min, int(power)


def bake_integrate(state: dict, verts: torch.Tensor, images: torch.Tensor, depth: torch.Tensor, K, c2w, normals: Optional[torch.Tensor] = None,
                   *, depth_tol, cos_min: float = 0.0, power: int = 2) -> dict:
    """Project posed colour frames onto the vertices of a mesh and add what they show to a state of :func:`bake_state`
    (``mofa_bake_integrate``).  ``verts [V,3]`` float32; ``images`` ``[n,H,W,C]`` or ``[H,W,C]`` float32 with the state's ``C``; ``depth``
    ``[n,H,W]`` or ``[H,W]`` float32 in the encoding of :func:`depth_frame` — the RAY PARAMETER of ``get_rays`` at the surface the view
    sees (normally :func:`rasterize` of the mesh itself through :func:`depth_frame`), ``+inf`` background, NaN or <= 0 unknown; ``K`` /
    ``c2w`` one camera or one per frame as in :func:`tsdf_integrate`; ``normals [V,3]`` (:func:`vertex_normals`) or ``None``.

    Per vertex and view, in the order of the frames and in fp64 (include/mofanerf_hip.h has every operation): the vertex is taken into the
    camera with :func:`tsdf_integrate`'s projection; its footprint is the 2 x 2 pixels around ``(u, v)`` and must lie inside the frame.  A
    background or unknown depth at any corner skips the view (the silhouette erodes by a pixel, which is wanted: a pixel on it mixes face
    and background); ``t - D > depth_tol`` at any corner counts the view in ``occluded`` and skips it.  With normals, ``cosv`` is the cosine
    between the normal and the direction to the camera: not ``> cos_min`` counts the view in ``grazing`` and skips it, otherwise the view
    weighs ``cosv ** power`` (repeated products); without normals every view weighs 1.  The colour is the bilinear interpolation of the
    four texels; a non-finite texel skips the view.  ``csum += w colour``, ``wsum += w``, and the colour of the view with the strictly
    largest weight so far is kept in ``cbest``.  No atomics and a fixed order: the same frames give the same bytes, and frames streamed in
    several calls give the bytes of one call with all of them.  Returns ``state`` (updated in place; ``state["frames"]`` counts).

    ``depth_tol`` (scene units) is required: none has been measured for a trained face; it must exceed the depth's own error (the
    rasteriser snaps vertices to 1/256 pixel) and stay below the thickness of what may not shine through.  ``cos_min`` and ``power`` are
    untuned defaults.  Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, tensors on different devices, frames smaller than
    2 x 2 or with ``H W >= 2^31``, camera counts that match neither 1 nor ``n``, and parameters out of range."""
    who = "bake_integrate"
    V, C_, dev = _bake_state(who, state)
    depth_tol, cos_min, power = _bake_params(who, depth_tol, cos_min, power)
    for name, t, cols in (("verts", verts, 3), ("normals", normals, 3)):
        if t is None:
            continue
        lib.ptr(t)
        if tuple(t.shape) != (V, cols) or t.device != dev:
            raise lib.MofaError(f"{who}: {name} {tuple(t.shape)} on {t.device} (want [{V},{cols}] on {dev}, the state's)")
    lib.ptr(images), lib.ptr(depth)
    if images.dim() not in (3, 4) or depth.dim() != images.dim() - 1 or tuple(images.shape[:-1]) != tuple(depth.shape) or images.shape[-1] != C_:
        raise lib.MofaError(f"{who}: images {tuple(images.shape)}, depth {tuple(depth.shape)} (want [n,H,W,{C_}] and [n,H,W], or [H,W,{C_}] and [H,W])")
    if images.device != dev or depth.device != dev:
        raise lib.MofaError(f"{who}: the state is on {dev}, the images on {images.device}, the depth on {depth.device}")
    frames = depth.detach().reshape((-1,) + tuple(depth.shape[-2:]))
    n, H, W = (int(v) for v in frames.shape)
    if n < 1 or H < 2 or W < 2 or H * W > INT32_MAX:
        raise lib.MofaError(f"{who}: {n} frames of H = {H}, W = {W} are refused (n >= 1, H, W >= 2, H W < 2^31)")
    cams = _tsdf_cameras(who, K, c2w, n)
    if V:
        with torch.cuda.device(dev):
            table = torch.from_numpy(cams).to(dev)
            lib.check(lib.load().mofa_bake_integrate(lib.ptr(verts.detach()), lib.ptr(None if normals is None else normals.detach()), V,
                                                     lib.ptr(images.detach()), lib.ptr(frames), n, H, W, C_, lib.ptr(table), int(cams.shape[0]),
                                                     depth_tol, cos_min, power, state["csum"].data_ptr(), state["wsum"].data_ptr(),
                                                     state["wbest"].data_ptr(), state["cbest"].data_ptr(), state["seen"].data_ptr(),
                                                     state["occluded"].data_ptr(), state["grazing"].data_ptr(), lib.stream()), "mofa_bake_integrate")
    state["frames"] = int(state.get("frames", 0)) + n
    return state


def bake_colors(state: dict, blend: str = "mean", fill: float = 0.0) -> dict:
    """The vertex colours of a baking state (``mofa_bake_resolve``).  ``blend="mean"``: the weighted mean ``csum / wsum`` of the views that
    entered, where ``wsum > 0``; ``"best"``: the colour of the single view with the largest weight (the earliest among equals), where
    ``seen > 0`` — sharper, with seams where the best view changes.  Everywhere else the colour is ``fill`` and the vertex is not valid.
    Returns ``colors [V,C]`` float32, ``valid [V]`` bool, ``seen [V]`` int32 (the state's) and ``counts``: ``colored``, then the uncoloured
    vertices by reason — ``occluded`` (some view saw something in front of them), ``grazing`` (only the angle test rejected them) and
    ``unseen`` (no view held them in a footprint with a known surface) — plus ``vertices`` and ``frames``; the four classes partition the
    vertices, and reading them is the call's one host read.  :func:`fill_colors` closes the holes."""
    who = "bake_colors"
    V, C_, dev = _bake_state(who, state)
    if blend not in _BAKE_BLEND:
        raise lib.MofaError(f"{who}: blend = {blend!r} (want 'mean' or 'best')")
    try:
        fill = float(fill)
    except (TypeError, ValueError):
        raise lib.MofaError(f"{who}: fill = {fill!r} (want a number)") from None
    colors = torch.empty((V, C_), dtype=torch.float32, device=dev)
    valid = torch.empty(V, dtype=torch.uint8, device=dev)
    counts = dict.fromkeys(_BAKE_COUNTS, 0)
    if V:
        with torch.cuda.device(dev):
            ws = torch.empty(16 * ((V + 255) // 256), dtype=torch.uint8, device=dev)
            n = torch.empty(len(_BAKE_COUNTS), dtype=torch.int64, device=dev)
            lib.check(lib.load().mofa_bake_resolve(V, C_, state["csum"].data_ptr(), state["wsum"].data_ptr(), state["cbest"].data_ptr(),
                                                   state["seen"].data_ptr(), state["occluded"].data_ptr(), state["grazing"].data_ptr(),
                                                   _BAKE_BLEND[blend], fill, lib.ptr(colors), valid.data_ptr(), ws.data_ptr(), n.data_ptr(),
                                                   lib.stream()), "mofa_bake_resolve")
            counts = dict(zip(_BAKE_COUNTS, (int(v) for v in n.cpu())))
    counts.update(vertices=V, frames=int(state.get("frames", 0)))
    return {"colors": colors, "valid": valid.bool(), "counts": counts, "seen": state["seen"]}


def fill_colors(colors: torch.Tensor, valid: torch.Tensor, faces: torch.Tensor, iterations: int):
    """Fill the holes of baked vertex colours from their neighbours (``mofa_bake_fill``): ``iterations`` Jacobi steps over
    :func:`vertex_adjacency`'s lists, double-buffered.  In a step every invalid vertex with at least one valid neighbour takes the mean of
    its valid neighbours' colours OF THE STEP'S INPUT (an fp64 sum in the adjacency's ascending order, one division, rounded to float32
    once) and turns valid; everything else is copied — the front advances one edge per step, and a colour that was baked never changes.
    ``colors [V,C]`` float32, ``valid [V]`` bool, ``faces [F,3]`` int32.  Returns ``(colors, valid, remaining)``: new tensors and the
    number of vertices still invalid (the call's host read) — not 0 when ``iterations`` is too small, or for a component with no valid
    vertex at all.  A face index outside [0, V) raises ``MofaError`` before any step runs; so do CPU tensors."""
    who = "fill_colors"
    lib.ptr(colors)
    if colors.dim() != 2 or not 1 <= colors.shape[1] <= BAKE_MAX_CHANNELS:
        raise lib.MofaError(f"{who}: want colors [V,C] with 1 <= C <= {BAKE_MAX_CHANNELS}, got {tuple(colors.shape)}")
    V, C_, dev = int(colors.shape[0]), int(colors.shape[1]), colors.device
    if not torch.is_tensor(valid) or not valid.is_cuda:
        raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got a CPU valid); there is no CPU fallback")
    if valid.dtype != torch.bool or tuple(valid.shape) != (V,) or valid.device != dev:
        raise lib.MofaError(f"{who}: valid is {valid.dtype} {tuple(valid.shape)} on {valid.device} (want bool [{V}] on {dev})")
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= BAKE_MAX_FILL:
        raise lib.MofaError(f"{who}: iterations = {iterations!r} (want an integer 0 .. {BAKE_MAX_FILL})")
    if V > INT32_MAX:
        raise lib.MofaError(f"{who}: {V} vertices exceed the int32 indices (2^31 - 1)")
    adj = vertex_adjacency(faces, V)                                          # validates the faces first
    if faces.device != dev:
        raise lib.MofaError(f"{who}: colors on {dev}, faces on {faces.device}")
    cur, ok = colors.detach().clone(), valid.to(torch.uint8).contiguous()
    if ok is valid:
        ok = ok.clone()
    if V and int(iterations):
        E = int(adj["neighbours"].shape[0])
        with torch.cuda.device(dev):
            nxt, ok_nxt = torch.empty_like(cur), torch.empty_like(ok)
            for _ in range(int(iterations)):
                lib.check(lib.load().mofa_bake_fill(lib.ptr(cur), ok.data_ptr(), V, C_, adj["offsets"].data_ptr(), adj["neighbours"].data_ptr(), E,
                                                    lib.ptr(nxt), ok_nxt.data_ptr(), lib.stream()), "mofa_bake_fill")
                cur, nxt, ok, ok_nxt = nxt, cur, ok_nxt, ok
    ok = ok.bool()
    remaining = int((~ok).sum().cpu()) if V else 0
    return cur, ok, remaining


# UV texture baking (mofa_uv_*).  A UV layout is OBJ-style and per corner: uvs [T,2] float32, uv_faces [F,3] int32,
# uv_faces[f, k] the UV of corner k of faces[f].  A texture is [Ht,Wt,C] float32, row 0 at the top: texel (i, j) has its centre at
# u = (j + 0.5) / Wt, v = 1 - (i + 0.5) / Ht.  uv_locate's grid of face lists is mofa_wind_bin_*'s over (u, v); its resolution changes
# no bit of the result.
UV_GRID_CAP = WIND_GRID_CAP
UV_GRID_AUTO_CAP = 256
_UV_COUNTS = ("degenerate", "non_finite_queries", "face_tests", "multi")       # MOFA_UV_* of the header


def default_uv_grid(F: int):
    """The resolution uv_locate picks for ``F`` UV faces: ``ceil(sqrt(F / 4))`` cells per side, 1 .. UV_GRID_AUTO_CAP."""
    g = int(min(max(math.ceil(math.sqrt(max(int(F), 0) / 4.0)), 1), UV_GRID_AUTO_CAP))
    return (g, g)


def _uv_layout(who, uvs, uv_faces):
    """(T, F, device) of a UV layout on the GPU: contiguous float32 uvs [T,2], contiguous int32 uv_faces [F,3]."""
    if not torch.is_tensor(uvs):
        raise lib.MofaError(f"{who}: want uvs as a float32 tensor [T,2] on the GPU, got {type(uvs).__name__}")
    lib.ptr(uvs)
    if uvs.dim() != 2 or uvs.shape[1] != 2:
        raise lib.MofaError(f"{who}: want uvs [T,2], got {tuple(uvs.shape)}")
    if not torch.is_tensor(uv_faces) or not uv_faces.is_cuda:
        raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got CPU uv_faces); there is no CPU fallback")
    if uv_faces.dtype != torch.int32 or not uv_faces.is_contiguous() or uv_faces.dim() != 2 or uv_faces.shape[1] != 3:
        raise lib.MofaError(f"{who}: want contiguous int32 uv_faces [F,3], got {uv_faces.dtype} {tuple(uv_faces.shape)}")
    if uv_faces.device != uvs.device:
        raise lib.MofaError(f"{who}: uvs on {uvs.device}, uv_faces on {uv_faces.device}")
    T, F = int(uvs.shape[0]), int(uv_faces.shape[0])
    if T > INT32_MAX or F > INT32_MAX:
        raise lib.MofaError(f"{who}: {T} UVs / {F} faces exceed the int32 indices (2^31 - 1)")
    return T, F, uvs.device


def _uv_grid_arg(who, grid):
    if grid is not None:
        g = np.asarray(grid).reshape(-1)
        if g.size not in (1, 2) or g.dtype.kind not in "iu" or (g < 1).any() or (g > UV_GRID_CAP).any():
            raise lib.MofaError(f"{who}: grid = {grid!r} (want None, an integer or two, 1 .. {UV_GRID_CAP} per side)")
        grid = tuple(int(v) for v in (np.repeat(g, 2) if g.size == 1 else g))
    return grid


def _texture_size(who, size):
    s = np.asarray(size).reshape(-1)
    if isinstance(size, (bool, np.bool_)) or s.size not in (1, 2) or s.dtype.kind not in "iu" or (s < 1).any():
        raise lib.MofaError(f"{who}: size = {size!r} (want a positive integer or (Ht, Wt))")
    Ht, Wt = (int(v) for v in (np.repeat(s, 2) if s.size == 1 else s))
    if Ht * Wt > INT32_MAX:
        raise lib.MofaError(f"{who}: a texture of {Ht} x {Wt} texels exceeds the int32 indices (Ht Wt < 2^31)")
    return Ht, Wt


def _uv_validate(who, uvs, uv_faces, T, F):
    """The layout's indices (mofa_cc_validate) and coordinates, before any other launch; returns the zero-padded [T,3] copy of the UVs."""
    L = lib.load()
    dev = uvs.device
    stream = lib.stream()
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    lib.check(L.mofa_cc_validate(uv_faces.data_ptr(), F, T, bad.data_ptr(), stream), "mofa_cc_validate")
    n_bad = int(bad.cpu()[0])
    if n_bad:
        raise lib.MofaError(f"{who}: {n_bad} of the {3 * F} UV indices lie outside [0, {T})")
    padded = torch.zeros((T, 3), dtype=torch.float32, device=dev)
    padded[:, :2] = uvs.detach()
    bad.zero_()
    lib.check(L.mofa_dist_validate(lib.ptr(padded), T, bad.data_ptr(), stream), "mofa_dist_validate")
    n_bad = int(bad.cpu()[0])
    if n_bad:
        raise lib.MofaError(f"{who}: {n_bad} of the {2 * T} UV coordinates are not finite")
    return padded


def _uv_lists(who, uvs, uv_faces, T, F, grid):
    """Validate a UV layout and bin its faces over (u, v) with mofa_wind_bin_count / _emit (the UVs as a zero-padded [T,3] copy, axis 2):
    every cell a face's closed UV box touches lists it, which is all a containment test needs.  What every batch of queries shares."""
    L = lib.load()
    dev = uvs.device
    i64 = dict(dtype=torch.int64, device=dev)
    stream = lib.stream()
    padded = _uv_validate(who, uvs, uv_faces, T, F)
    box = torch.stack([padded.amin(0), padded.amax(0)]).cpu().numpy()
    if grid is None:
        grid = default_uv_grid(F)
    origin, cell = wind_grid(box[0], box[1], grid, 2)
    o2, c2, n2 = (C.c_double * 2)(*origin), (C.c_double * 2)(*cell), (C.c_int32 * 2)(*grid)
    n_cells = grid[0] * grid[1]
    scratch = torch.zeros(len(_WIND_COUNTS), **i64)
    per_face = torch.empty(F, **i64)
    lib.check(L.mofa_wind_bin_count(lib.ptr(padded), uv_faces.data_ptr(), F, T, 2, o2, c2, n2, per_face.data_ptr(), scratch.data_ptr(), stream),
              "mofa_wind_bin_count")
    ends = torch.cumsum(per_face, 0)
    P = int(ends[-1].cpu())
    if P > INT32_MAX:
        raise lib.MofaError(f"{who}: the {F} UV faces enter {P} cells of the {grid} grid, more than 2^31 - 1: take a coarser grid")
    start = torch.zeros(n_cells + 1, dtype=torch.int32, device=dev)
    pair_face = torch.empty(P, dtype=torch.int32, device=dev)
    if P:
        offsets = (ends - per_face).contiguous()
        pair_cell = torch.empty(P, dtype=torch.int32, device=dev)
        lib.check(L.mofa_wind_bin_emit(lib.ptr(padded), uv_faces.data_ptr(), F, T, 2, o2, c2, n2, offsets.data_ptr(), P, pair_cell.data_ptr(),
                                       pair_face.data_ptr(), stream), "mofa_wind_bin_emit")
        if n_cells > 1:
            by_cell = torch.sort(pair_cell, stable=True).indices
            pair_face = pair_face[by_cell].contiguous()
        start[1:] = torch.cumsum(torch.bincount(pair_cell.long(), minlength=n_cells), 0).to(torch.int32)
    return dict(grid=grid, origin=origin, cell=cell, o2=o2, c2=c2, n2=n2, start=start, pair_face=pair_face, P=P)


def _uv_query(queries, N, uvs, uv_faces, T, F, b):
    """(face [N] int32, bary [N,3] float64, counts) of one batch of queries against the lists ``b`` of :func:`_uv_lists`."""
    dev = uvs.device
    grid = b["grid"]
    face = torch.empty(N, dtype=torch.int32, device=dev)
    bary = torch.empty((N, 3), dtype=torch.float64, device=dev)
    counts = torch.zeros(len(_UV_COUNTS), dtype=torch.int64, device=dev)
    order = None
    if grid[0] * grid[1] > 1:                    # queries of one cell next to each other: a wavefront's lanes walk the same list
        t = torch.nan_to_num((queries - torch.from_numpy(b["origin"]).to(dev)) / torch.from_numpy(b["cell"]).to(dev), nan=0.0, posinf=0.0,
                             neginf=0.0).floor_()
        hi = torch.tensor([g - 1 for g in grid], dtype=torch.float64, device=dev)
        c = torch.minimum(torch.clamp_(t, min=0.0), hi).long()
        order = torch.argsort(c[:, 0] * grid[1] + c[:, 1])
        del t, c
    lib.check(lib.load().mofa_uv_locate(queries.data_ptr(), N, None if order is None else order.data_ptr(), lib.ptr(uvs.detach()), T,
                                        uv_faces.data_ptr(), F, b["o2"], b["c2"], b["n2"], b["start"].data_ptr(),
                                        b["pair_face"].data_ptr() if b["P"] else None, b["P"], face.data_ptr(), bary.data_ptr(), counts.data_ptr(),
                                        lib.stream()), "mofa_uv_locate")
    return face, bary, dict(zip(_UV_COUNTS, (int(v) for v in counts.cpu())))


def _uv_locate(who, queries, N, uvs, uv_faces, T, F, grid):
    dev = uvs.device
    if N == 0 or T == 0 or F == 0:
        counts = dict.fromkeys(_UV_COUNTS, 0)
        if N:
            counts["non_finite_queries"] = int((~torch.isfinite(queries).all(1)).sum())
        return (torch.full((N,), -1, dtype=torch.int32, device=dev), torch.full((N, 3), float("nan"), dtype=torch.float64, device=dev), counts,
                grid if grid is not None else (1, 1))
    with torch.cuda.device(dev):
        b = _uv_lists(who, uvs, uv_faces, T, F, grid)
        face, bary, counts = _uv_query(queries, N, uvs, uv_faces, T, F, b)
    return face, bary, counts, b["grid"]


def uv_locate(queries: torch.Tensor, uvs: torch.Tensor, uv_faces: torch.Tensor, grid=None) -> dict:
    """The UV triangle that holds each of ``queries [N,2] float64`` (u, v), on the GPU (``mofa_uv_locate``).  Returns a dict: ``face [N]
    int32`` (-1: none), ``bary [N,3] float64`` (NaN where none; ``bary[:, k]`` weighs corner ``k``), ``counts`` (``degenerate``: the UV
    faces with no area, which hold nothing; ``non_finite_queries``; ``face_tests``; ``multi``: the queries strictly inside two or more
    faces, which marks overlapping charts) and ``grid``.

    The arithmetic is fixed (include/mofanerf_hip.h): an edge function is evaluated on the edge's endpoints in COORDINATE order, so the two
    faces of an edge — also across a seam, where the edge has other UV indices but equal coordinates — see the same bits up to an exact
    sign; zeros count as inside and the lowest face wins, so a point on a shared edge never falls between two faces.  Mirrored charts
    (``D < 0``) are located like any other.  ``grid`` — ``None`` (``default_uv_grid``), an int or a pair, 1 .. UV_GRID_CAP per side —
    changes the time but no bit of the result; ``grid=1`` is brute force through the same kernel.  There is no wrap-around: a query outside
    every chart gets -1.  ``N``, ``T`` or ``F`` of 0 return without a launch.

    Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, tensors on different devices, a grid out of range, a UV index outside
    ``[0, T)`` (``mofa_cc_validate``) and a non-finite UV coordinate, all before the query runs."""
    who = "uv_locate"
    T, F, dev = _uv_layout(who, uvs, uv_faces)
    if not torch.is_tensor(queries) or not queries.is_cuda:
        raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got CPU queries); there is no CPU fallback")
    if queries.dtype != torch.float64 or not queries.is_contiguous() or queries.dim() != 2 or queries.shape[1] != 2:
        raise lib.MofaError(f"{who}: want contiguous float64 queries [N,2], got {queries.dtype} {tuple(queries.shape)}")
    if queries.device != dev:
        raise lib.MofaError(f"{who}: uvs on {dev}, queries on {queries.device}")
    N = int(queries.shape[0])
    if N > INT32_MAX:
        raise lib.MofaError(f"{who}: {N} queries exceed the int32 indices (2^31 - 1)")
    grid = _uv_grid_arg(who, grid)
    face, bary, counts, grid = _uv_locate(who, queries.detach(), N, uvs, uv_faces, T, F, grid)
    return {"face": face, "bary": bary, "counts": counts, "grid": grid}


def texel_centres(size, device="cuda") -> torch.Tensor:
    """float64 [Ht Wt, 2]: the (u, v) of every texel centre, row-major: ``u = (j + 0.5) / Wt``, ``v = 1 - (i + 0.5) / Ht``."""
    Ht, Wt = _texture_size("texel_centres", size)
    f64 = dict(dtype=torch.float64, device=device)          # (a tensor divisor: dividing by a Python scalar multiplies by its reciprocal on the GPU)
    u = (torch.arange(Wt, **f64) + 0.5) / torch.full((Wt,), float(Wt), **f64)
    v = 1.0 - (torch.arange(Ht, **f64) + 0.5) / torch.full((Ht,), float(Ht), **f64)
    return torch.stack([u[None, :].expand(Ht, Wt), v[:, None].expand(Ht, Wt)], -1).reshape(-1, 2).contiguous()


def texel_map(uvs: torch.Tensor, uv_faces: torch.Tensor, size, grid=None) -> dict:
    """The map from the texels of a ``size`` (an int or ``(Ht, Wt)``) texture to the surface: :func:`uv_locate` of every texel centre.
    Returns a dict: ``face [Ht,Wt] int32`` (-1: the texel lies in no chart), ``bary [Ht,Wt,3] float64``, ``covered [Ht,Wt] bool``,
    ``index [M] int64`` (the covered texels' flat indices, row-major), ``counts`` (``covered`` = M; ``multi``: texels strictly inside two
    or more faces — overlapping charts, of which the lowest face wins; ``degenerate``: UV faces without area; ``faces_without_texels``:
    faces that own no texel — degenerate, hidden under a lower-numbered chart, outside [0, 1]^2 or thinner than the texel grid;
    ``face_tests``), ``size`` = ``(Ht, Wt)``, ``grid`` and ``n_faces``.  Refusals as :func:`uv_locate`; ``Ht Wt >= 2^31`` is refused."""
    who = "texel_map"
    T, F, dev = _uv_layout(who, uvs, uv_faces)
    Ht, Wt = _texture_size(who, size)
    grid = _uv_grid_arg(who, grid)
    with torch.cuda.device(dev):
        face, bary, counts, grid = _uv_locate(who, texel_centres((Ht, Wt), dev), Ht * Wt, uvs, uv_faces, T, F, grid)
        covered = face >= 0
        index = torch.nonzero(covered).reshape(-1)
        owners = int(torch.unique(face[index]).numel())
    out_counts = {"covered": int(index.numel()), "multi": counts["multi"], "degenerate": counts["degenerate"], "faces_without_texels": F - owners,
                  "face_tests": counts["face_tests"]}
    return {"face": face.reshape(Ht, Wt), "bary": bary.reshape(Ht, Wt, 3), "covered": covered.reshape(Ht, Wt), "index": index,
            "counts": out_counts, "size": (Ht, Wt), "grid": grid, "n_faces": F}


def _texel_map_arg(who, tmap):
    """((Ht, Wt), M, device) of a texel map, its tensors checked."""
    keys = ("face", "bary", "covered", "index", "size", "n_faces")
    if not isinstance(tmap, dict) or any(k not in tmap for k in keys):
        raise lib.MofaError(f"{who}: want the dict of texel_map")
    Ht, Wt = _texture_size(who, tmap["size"])
    face, bary, index = tmap["face"], tmap["bary"], tmap["index"]
    for name, t, dtype, shape in (("face", face, torch.int32, (Ht, Wt)), ("bary", bary, torch.float64, (Ht, Wt, 3)),
                                  ("index", index, torch.int64, None)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got a CPU tensor as the map's {name}); there is no CPU fallback")
        if t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape) or t.device != face.device:
            raise lib.MofaError(f"{who}: the map's {name} is {t.dtype} {tuple(t.shape)} on {t.device} (want contiguous {dtype} on {face.device})")
    if index.dim() != 1:
        raise lib.MofaError(f"{who}: the map's index is {tuple(index.shape)} (want [M])")
    return (Ht, Wt), int(index.numel()), face.device


def texel_surface(tmap: dict, verts: torch.Tensor, faces: torch.Tensor, normals: Optional[torch.Tensor] = None):
    """``(points [M,3], normals [M,3])`` float32: the surface point and the unit normal of every covered texel of :func:`texel_map`, in the
    order of its ``index`` (``mofa_uv_surface``): the barycentric interpolation of the face's vertices in fp64, rounded to float32 once,
    and the interpolation of ``normals [V,3]`` normalised — or, with ``normals=None``, the face's flat normal ``(X1 - X0) x (X2 - X0)``,
    which follows the faces' winding (a mesh wound with its normals inward needs ``normals=``: :func:`bake_integrate` calls every view of
    an inward normal grazing).  A normal without length is (0, 0, 0).  These are the ``verts`` and ``normals`` :func:`bake_integrate` takes.
    ``faces`` must be the mesh the layout belongs to (``F`` equal to the layout's); a face index outside ``[0, V)`` raises ``MofaError``."""
    who = "texel_surface"
    (Ht, Wt), M, dev = _texel_map_arg(who, tmap)
    V, F, mdev = _mesh_tensors(who, verts, faces)
    if mdev != dev:
        raise lib.MofaError(f"{who}: the map is on {dev}, the mesh on {mdev}")
    if F != int(tmap["n_faces"]):
        raise lib.MofaError(f"{who}: the mesh has {F} faces, the UV layout of the map {int(tmap['n_faces'])}")
    if normals is not None:
        lib.ptr(normals)
        if tuple(normals.shape) != (V, 3) or normals.device != dev:
            raise lib.MofaError(f"{who}: normals {tuple(normals.shape)} on {normals.device} (want [{V},3] on {dev})")
    points = torch.empty((M, 3), dtype=torch.float32, device=dev)
    out_normals = torch.empty((M, 3), dtype=torch.float32, device=dev)
    if M == 0:
        return points, out_normals
    if V == 0 or F == 0:
        raise lib.MofaError(f"{who}: {M} covered texels, but the mesh has {V} vertices and {F} faces")
    with torch.cuda.device(dev):
        L = lib.load()
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        lib.check(L.mofa_cc_validate(faces.data_ptr(), F, V, bad.data_ptr(), lib.stream()), "mofa_cc_validate")
        n_bad = int(bad.cpu()[0])
        if n_bad:
            raise lib.MofaError(f"{who}: {n_bad} of the {3 * F} face indices lie outside [0, {V})")
        index = tmap["index"]
        face = tmap["face"].reshape(-1)[index].contiguous()
        bary = tmap["bary"].reshape(-1, 3)[index].contiguous()
        bad.zero_()
        lib.check(L.mofa_uv_surface(face.data_ptr(), bary.data_ptr(), M, lib.ptr(verts.detach()), V, faces.data_ptr(), F,
                                    lib.ptr(None if normals is None else normals.detach()), lib.ptr(points), lib.ptr(out_normals), bad.data_ptr(),
                                    lib.stream()), "mofa_uv_surface")
    return points, out_normals


def texture_state(tmap: dict, channels: int = 3) -> dict:
    """``bake_state(M, channels)`` for the ``M`` covered texels of a :func:`texel_map`: frames go in through :func:`bake_integrate` with
    :func:`texel_surface`'s points and normals — the integration kernel, its streaming and its bit-for-bit properties are the vertices'."""
    _, M, dev = _texel_map_arg("texture_state", tmap)
    return bake_state(M, channels, dev)


def dilate_texture(texture: torch.Tensor, valid: torch.Tensor, iterations: int):
    """Fill the gutters around the charts of a texture (``mofa_uv_dilate``): ``iterations`` steps on the image grid, double-buffered.  In a
    step every invalid texel with at least one valid texel among its 8 neighbours (inside the image: no wrap-around) takes the mean of their
    colours OF THE STEP'S INPUT (an fp64 sum in row-major order of the 3 x 3 window, one division, rounded to float32 once) and turns
    valid; everything else is copied — the front advances one texel per step and a baked texel never changes.  This is what a bilinear
    lookup at a chart's border reads.  ``texture [Ht,Wt,C]`` float32, ``valid [Ht,Wt]`` bool.  Returns ``(texture, valid, remaining)``: new
    tensors and the texels still invalid (the call's host read)."""
    who = "dilate_texture"
    lib.ptr(texture)
    if texture.dim() != 3 or not 1 <= texture.shape[2] <= BAKE_MAX_CHANNELS or texture.shape[0] < 1 or texture.shape[1] < 1:
        raise lib.MofaError(f"{who}: want texture [Ht,Wt,C] with 1 <= C <= {BAKE_MAX_CHANNELS}, got {tuple(texture.shape)}")
    Ht, Wt, C_ = (int(v) for v in texture.shape)
    dev = texture.device
    if Ht * Wt > INT32_MAX:
        raise lib.MofaError(f"{who}: a texture of {Ht} x {Wt} texels exceeds the int32 indices (Ht Wt < 2^31)")
    if not torch.is_tensor(valid) or not valid.is_cuda:
        raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got a CPU valid); there is no CPU fallback")
    if valid.dtype != torch.bool or tuple(valid.shape) != (Ht, Wt) or valid.device != dev:
        raise lib.MofaError(f"{who}: valid is {valid.dtype} {tuple(valid.shape)} on {valid.device} (want bool [{Ht},{Wt}] on {dev})")
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= BAKE_MAX_FILL:
        raise lib.MofaError(f"{who}: iterations = {iterations!r} (want an integer 0 .. {BAKE_MAX_FILL})")
    cur, ok = texture.detach().clone(), valid.to(torch.uint8).contiguous()
    if int(iterations):
        with torch.cuda.device(dev):
            nxt, ok_nxt = torch.empty_like(cur), torch.empty_like(ok)
            for _ in range(int(iterations)):
                lib.check(lib.load().mofa_uv_dilate(lib.ptr(cur), ok.data_ptr(), Ht, Wt, C_, lib.ptr(nxt), ok_nxt.data_ptr(), lib.stream()),
                          "mofa_uv_dilate")
                cur, nxt, ok, ok_nxt = nxt, cur, ok_nxt, ok
    ok = ok.bool()
    return cur, ok, int((~ok).sum().cpu())


def texture_image(state: dict, tmap: dict, blend: str = "mean", fill: float = 0.0, dilate: int = 0) -> dict:
    """The texture image of a baking state over the covered texels of ``tmap``: :func:`bake_colors` (``blend``, ``fill``), scattered
    through the map's ``index`` into ``[Ht,Wt,C]`` (``fill`` everywhere else), then ``dilate`` steps of :func:`dilate_texture`.  Returns a
    dict: ``texture [Ht,Wt,C]`` float32, ``valid [Ht,Wt]`` bool, ``counts`` (:func:`bake_colors`' — ``colored``, ``occluded``, ``grazing``,
    ``unseen``, ``vertices`` = the covered texels, ``frames`` — taken BEFORE dilation) and ``remaining`` (the texels invalid at the end:
    everything farther than ``dilate`` texels from a coloured one)."""
    who = "texture_image"
    (Ht, Wt), M, dev = _texel_map_arg(who, tmap)
    V, C_, sdev = _bake_state(who, state)
    if V != M or sdev != dev:
        raise lib.MofaError(f"{who}: the state holds {V} points on {sdev}, the map {M} covered texels on {dev}")
    if isinstance(dilate, (bool, np.bool_)) or not isinstance(dilate, (int, np.integer)) or not 0 <= int(dilate) <= BAKE_MAX_FILL:
        raise lib.MofaError(f"{who}: dilate = {dilate!r} (want an integer 0 .. {BAKE_MAX_FILL})")
    baked = bake_colors(state, blend, fill)
    with torch.cuda.device(dev):
        texture = torch.full((Ht * Wt, C_), float(fill), dtype=torch.float32, device=dev)
        valid = torch.zeros(Ht * Wt, dtype=torch.bool, device=dev)
        texture[tmap["index"]] = baked["colors"]
        valid[tmap["index"]] = baked["valid"]
        texture, valid = texture.reshape(Ht, Wt, C_), valid.reshape(Ht, Wt)
        if int(dilate):
            texture, valid, remaining = dilate_texture(texture, valid, int(dilate))
        else:
            remaining = int((~valid).sum().cpu())
    return {"texture": texture, "valid": valid, "counts": baked["counts"], "remaining": remaining}


def sample_texture(texture: torch.Tensor, face: torch.Tensor, bary: torch.Tensor, uvs: torch.Tensor, uv_faces: torch.Tensor,
                   background: float = 0.0) -> torch.Tensor:
    """The texture lookup of a rasterised view (``mofa_uv_sample``): ``face [H,W] int32`` and ``bary [H,W,3] float32`` exactly as
    ``rasterize(bary=True)`` returns them, ``texture [Ht,Wt,C]`` float32.  Per pixel the UV is the barycentric interpolation of the
    corners' UVs in fp64 (never rounded to float32), the lookup bilinear between the four texel centres around it with clamp-to-edge, in
    :func:`bake_integrate`'s order, rounded once.  Returns ``[H,W,C]`` float32; a pixel that hit nothing (``face < 0``) is ``background``.
    Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, different devices, a UV index outside ``[0, T)`` and a non-finite UV."""
    who = "sample_texture"
    T, F, dev = _uv_layout(who, uvs, uv_faces)
    lib.ptr(texture), lib.ptr(bary)
    if texture.dim() != 3 or not 1 <= texture.shape[2] <= BAKE_MAX_CHANNELS or texture.shape[0] < 1 or texture.shape[1] < 1:
        raise lib.MofaError(f"{who}: want texture [Ht,Wt,C] with 1 <= C <= {BAKE_MAX_CHANNELS}, got {tuple(texture.shape)}")
    Ht, Wt, C_ = (int(v) for v in texture.shape)
    if Ht * Wt > INT32_MAX:
        raise lib.MofaError(f"{who}: a texture of {Ht} x {Wt} texels exceeds the int32 indices (Ht Wt < 2^31)")
    if not torch.is_tensor(face) or not face.is_cuda:
        raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got a CPU face map); there is no CPU fallback")
    if face.dtype != torch.int32 or not face.is_contiguous() or face.dim() != 2:
        raise lib.MofaError(f"{who}: want a contiguous int32 face map [H,W], got {face.dtype} {tuple(face.shape)}")
    H, W = (int(v) for v in face.shape)
    if tuple(bary.shape) != (H, W, 3):
        raise lib.MofaError(f"{who}: bary {tuple(bary.shape)} (want [{H},{W},3], the face map's)")
    if any(t.device != dev for t in (texture, face, bary)):
        raise lib.MofaError(f"{who}: uvs on {dev}, texture on {texture.device}, face on {face.device}, bary on {bary.device}")
    if H * W > INT32_MAX:
        raise lib.MofaError(f"{who}: {H} x {W} pixels exceed the int32 indices (H W < 2^31)")
    try:
        background = float(background)
    except (TypeError, ValueError):
        raise lib.MofaError(f"{who}: background = {background!r} (want a number)") from None
    out = torch.full((H, W, C_), background, dtype=torch.float32, device=dev)
    if H * W == 0 or T == 0 or F == 0:
        return out
    with torch.cuda.device(dev):
        _uv_validate(who, uvs, uv_faces, T, F)
        n = torch.zeros(1, dtype=torch.int64, device=dev)
        lib.check(lib.load().mofa_uv_sample(face.data_ptr(), lib.ptr(bary.detach()), H * W, lib.ptr(uvs.detach()), T, uv_faces.data_ptr(), F,
                                            lib.ptr(texture.detach()), Ht, Wt, C_, background, lib.ptr(out), n.data_ptr(), lib.stream()),
                  "mofa_uv_sample")
    return out


def face_atlas(n_faces: int, size, padding: float = 1.0):
    """A deterministic per-triangle UV atlas for a mesh that has no UVs (an extraction, a simplification): ``(uvs [3 F, 2] float32,
    uv_faces [F,3] int32, info)`` as NumPy arrays, closed-form in fp64 on the host.  Faces ``2k`` and ``2k + 1`` share the cell ``k``
    (row-major from the top left) of an ``n x n`` grid over the texture, ``n = ceil(sqrt(ceil(F / 2)))``; each is a right triangle with the
    winding of its face (``D > 0``), its legs ``padding`` texels inside the cell's border and its hypotenuse ``padding`` texels from the
    cell's diagonal, face ``2k`` toward the cell's top-left corner, ``2k + 1`` toward its bottom-right.  Every edge is a seam and charts
    are ``2 padding`` texels apart, so nothing bleeds between faces (``texel_map(...)["counts"]["multi"] == 0``).  ``size`` (an int or
    ``(Ht, Wt)``) is refused, with the size that would do, when a cell cannot hold the insets plus legs of one texel.  ``info``: ``n``,
    ``cell`` (``(h, w)`` in texels), ``padding``, ``size`` and ``min_size``.  The area is spent evenly per face, not per surface area."""
    who = "face_atlas"
    if isinstance(n_faces, (bool, np.bool_)) or not isinstance(n_faces, (int, np.integer)) or not 0 <= int(n_faces) <= INT32_MAX // 3:
        raise lib.MofaError(f"{who}: n_faces = {n_faces!r} (want an integer 0 .. (2^31 - 1) / 3)")
    Ht, Wt = _texture_size(who, size)
    try:
        p = float(padding)
    except (TypeError, ValueError):
        raise lib.MofaError(f"{who}: padding = {padding!r} (want a number)") from None
    if not (np.isfinite(p) and p >= 0):
        raise lib.MofaError(f"{who}: padding = {padding!r} (want finite and >= 0)")
    F = int(n_faces)
    n = max(int(math.ceil(math.sqrt(math.ceil(F / 2)))), 1)
    while n * n * 2 < F:                                                          # (sqrt rounded down on a perfect square)
        n += 1
    h, w = Ht / n, Wt / n
    d = p * math.sqrt(1.0 / (w * w) + 1.0 / (h * h))                              # the hypotenuse's offset from the diagonal x / w + y / h = 1
    leg_x, leg_y = w * (1.0 - d - p / h) - p, h * (1.0 - d - p / w) - p
    min_size = n * int(math.ceil(1.0 + (2.0 + math.sqrt(2.0)) * p))
    if not (leg_x >= 1.0 and leg_y >= 1.0):
        raise lib.MofaError(f"{who}: {F} faces in {n} x {n} cells of {h:g} x {w:g} texels leave legs of {leg_y:g} x {leg_x:g} texels inside a "
                            f"padding of {p:g}: want legs of at least one texel, which size = {min_size} gives")
    k = np.arange(F, dtype=np.int64) // 2
    x0, y0 = (k % n).astype(np.float64) * w, (k // n).astype(np.float64) * h    # the cell's top-left corner in texels (x right, y down)
    upper = (np.arange(F) % 2 == 0)
    # corner 0 at the right angle; then the corner along y and the corner along x, which in (u, v = 1 - y / Ht) is counter-clockwise
    ax, ay = np.where(upper, x0 + p, x0 + w - p), np.where(upper, y0 + p, y0 + h - p)
    bx, by = ax, np.where(upper, y0 + h * (1.0 - d - p / w), y0 + h * (d + p / w))
    cx, cy = np.where(upper, x0 + w * (1.0 - d - p / h), x0 + w * (d + p / h)), ay
    xy = np.stack([np.stack([ax, ay], -1), np.stack([bx, by], -1), np.stack([cx, cy], -1)], 1).reshape(-1, 2)
    uvs = np.stack([xy[:, 0] / Wt, 1.0 - xy[:, 1] / Ht], -1).astype(np.float32)
    uv_faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    return uvs, uv_faces, {"n": n, "cell": (h, w), "padding": p, "size": (Ht, Wt), "min_size": min_size}


def write_obj(path: str, verts, faces, uvs=None, uv_faces=None, normals=None, texture=None) -> None:
    """Wavefront OBJ (text): ``v`` per vertex, ``vt`` per UV, ``vn`` per vertex normal, and ``f v``, ``f v/vt``, ``f v//vn`` or
    ``f v/vt/vn`` per face, 1-based (normals are per vertex: ``vn`` index = ``v`` index).  With ``texture [Ht,Wt,3]`` (in [0, 1]) the
    files ``<stem>.mtl`` and ``<stem>.png`` are written next to ``path`` — the texture through ``to8b`` and ``io.write_png``, row 0 at the
    top, which is ``v = 1`` — and the OBJ names them (``mtllib``, ``usemtl``).  Plain host code: works without a GPU.  Floats are written
    with 9 significant digits, so float32 values survive a round trip through :func:`read_obj`."""
    import os
    from . import io as mio
    v = np.ascontiguousarray(_host(verts), dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(_host(faces), dtype=np.int64).reshape(-1, 3)
    if (uvs is None) != (uv_faces is None):
        raise ValueError("uvs and uv_faces go together")
    stem = os.path.splitext(os.path.basename(path))[0]
    folder = os.path.dirname(os.path.abspath(path))
    lines = [f"# {len(v)} vertices, {len(f)} faces"]
    if texture is not None:
        if uvs is None:
            raise ValueError("a texture needs uvs and uv_faces")
        img = _host(texture)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"the texture must be [Ht,Wt,3], got {img.shape}")
        mio.write_png(os.path.join(folder, stem + ".png"), to8b(img))
        with open(os.path.join(folder, stem + ".mtl"), "w") as fh:
            fh.write(f"newmtl {stem}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {stem}.png\n")
        lines += [f"mtllib {stem}.mtl", f"usemtl {stem}"]
    lines += ["v %.9g %.9g %.9g" % tuple(float(c) for c in row) for row in v]
    if uvs is not None:
        t = np.ascontiguousarray(_host(uvs), dtype=np.float32).reshape(-1, 2)
        tf = np.ascontiguousarray(_host(uv_faces), dtype=np.int64).reshape(-1, 3)
        if len(tf) != len(f):
            raise ValueError(f"{len(tf)} UV faces for {len(f)} faces")
        lines += ["vt %.9g %.9g" % tuple(float(c) for c in row) for row in t]
    if normals is not None:
        nrm = np.ascontiguousarray(_host(normals), dtype=np.float32).reshape(-1, 3)
        if len(nrm) != len(v):
            raise ValueError(f"{len(nrm)} normals for {len(v)} vertices")
        lines += ["vn %.9g %.9g %.9g" % tuple(float(c) for c in row) for row in nrm]
    for i, tri in enumerate(f + 1):
        if uvs is not None and normals is not None:
            lines.append("f " + " ".join(f"{a}/{b}/{a}" for a, b in zip(tri, tf[i] + 1)))
        elif uvs is not None:
            lines.append("f " + " ".join(f"{a}/{b}" for a, b in zip(tri, tf[i] + 1)))
        elif normals is not None:
            lines.append("f " + " ".join(f"{a}//{a}" for a in tri))
        else:
            lines.append("f " + " ".join(str(a) for a in tri))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def read_obj(path: str) -> dict:
    """Read a Wavefront OBJ: a dict of NumPy arrays ``verts [V,3] float32``, ``faces [F,3] int32``, ``uvs [T,2] float32`` and ``uv_faces
    [F,3] int32`` (both ``None`` when no face has a ``vt``), ``normals [V,3] float32`` (``None`` unless every corner names a ``vn``; the
    ``vn`` of a vertex's LAST corner in file order is the vertex's) and ``mtllib`` (the file's, or ``None``).  Polygons are
    fan-triangulated from their first corner; negative indices count back from the element read last; a face that mixes corners with and
    without ``vt`` raises ``ValueError``; so does a file in which some faces have ``vt`` and others have none (``uv_faces`` has one row
    per face or does not exist), and an index outside what has been read.  Plain host code: works without a GPU."""
    v, vt, vn, faces, uv_faces, n_faces = [], [], [], [], [], []
    mtllib = None
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            w = line.split("#", 1)[0].split()
            if not w:
                continue
            if w[0] == "v":
                v.append([float(c) for c in w[1:4]])
            elif w[0] == "vt":
                vt.append([float(c) for c in (w[1:3] + ["0"])[:2]])
            elif w[0] == "vn":
                vn.append([float(c) for c in w[1:4]])
            elif w[0] == "mtllib":
                mtllib = " ".join(w[1:])
            elif w[0] == "f":
                corners = []
                for word in w[1:]:
                    parts = (word.split("/") + ["", ""])[:3]
                    idx = []
                    for part, have in zip(parts, (len(v), len(vt), len(vn))):
                        if part == "":
                            idx.append(None)
                            continue
                        k = int(part)
                        k = k - 1 if k > 0 else have + k
                        if k < 0 or k >= have or int(part) == 0:
                            raise ValueError(f"{path}:{ln}: index {part} outside the {have} elements read so far")
                        idx.append(k)
                    if idx[0] is None:
                        raise ValueError(f"{path}:{ln}: a corner without a vertex index")
                    corners.append(idx)
                if len(corners) < 3:
                    raise ValueError(f"{path}:{ln}: a face of {len(corners)} corners")
                with_vt = [c[1] is not None for c in corners]
                if any(with_vt) and not all(with_vt):
                    raise ValueError(f"{path}:{ln}: a face that mixes corners with and without vt")
                for k in range(1, len(corners) - 1):
                    tri = (corners[0], corners[k], corners[k + 1])
                    faces.append([c[0] for c in tri])
                    uv_faces.append([c[1] for c in tri] if all(with_vt) else None)
                    n_faces.append([c[2] for c in tri])
    verts = np.asarray(v, np.float32).reshape(-1, 3)
    out = {"verts": verts, "faces": np.asarray(faces, np.int32).reshape(-1, 3), "uvs": None, "uv_faces": None, "normals": None, "mtllib": mtllib}
    if any(t is not None for t in uv_faces):
        if any(t is None for t in uv_faces):
            raise ValueError(f"{path}: faces with and faces without vt")
        out["uvs"], out["uv_faces"] = np.asarray(vt, np.float32).reshape(-1, 2), np.asarray(uv_faces, np.int32).reshape(-1, 3)
    if n_faces and all(k is not None for tri in n_faces for k in tri):
        normals = np.zeros_like(verts)
        table = np.asarray(vn, np.float32).reshape(-1, 3)
        normals[out["faces"].reshape(-1)] = table[np.asarray(n_faces, np.int64).reshape(-1)]
        out["normals"] = normals
    return out


SMOOTH_MAX_ITERATIONS = 1000
_SMOOTH_COUNTS =("flat_corners", "negative_weights", "zero_weight", "bad_index")       # MOFA_SMOOTH_* of the header
_SMOOTH_WEIGHTS = ("uniform", "cotangent")
_SMOOTH_BOUNDARIES = ("fixed", "free")


def _adjacency(who, faces, V, F):
    """The sorted half-edge entries of a mesh (V, F >= 1; ``mofa_cc_validate`` first) and what follows from them: ``perm [P] int64`` (the
    entries ``e = 2 (3 f + c) + dir`` without self-loops, stably sorted by the key ``(i << 31) | j``), ``seg [E+1] int64`` (the runs of the
    E distinct directed pairs), ``offsets``, ``neighbours``, ``boundary`` and, as tensors not yet read, ``degree_max`` and
    ``edges_nonmanifold``."""
    dev = faces.device
    i64 = dict(dtype=torch.int64, device=dev)
    bad = torch.zeros(1, **i64)
    lib.check(lib.load().mofa_cc_validate(faces.data_ptr(), F, V, bad.data_ptr(), lib.stream()), "mofa_cc_validate")
    n_bad = int(bad.cpu()[0])
    if n_bad:
        raise lib.MofaError(f"{who}: {n_bad} of the {3 * F} face indices lie outside [0, {V})")
    f = faces.long()
    a, b = f[:, [1, 2, 0]], f[:, [2, 0, 1]]                                  # corner c: the edge opposite to it
    i, j = torch.stack([a, b], -1).reshape(-1), torch.stack([b, a], -1).reshape(-1)       # entry e = 2 (3 f + c) + dir
    entry = torch.nonzero(i != j)[:, 0]
    key = (i[entry] << 31) | j[entry]
    order = torch.sort(key, stable=True).indices
    perm = entry[order].contiguous()
    pair, run = torch.unique_consecutive(key[order], return_counts=True)
    seg = torch.zeros(pair.shape[0] + 1, **i64)
    seg[1:] = torch.cumsum(run, 0)
    pi, pj = pair >> 31, pair & INT32_MAX
    degree = torch.bincount(pi, minlength=V)
    offsets = torch.zeros(V + 1, **i64)
    offsets[1:] = torch.cumsum(degree, 0)
    boundary = torch.zeros(V, dtype=torch.bool, device=dev)
    boundary[pi[run == 1]] = True                                           # (the pair (j, i) has the same run: both ends are marked)
    return {"offsets": offsets, "neighbours": pj.to(torch.int32).contiguous(), "boundary": boundary, "perm": perm, "seg": seg,
            "degree_max": degree.max(), "edges_nonmanifold": ((run > 2) & (pi < pj)).sum(), "n_isolated": (degree == 0).sum()}


def vertex_adjacency(faces: torch.Tensor, V: int) -> dict:
    """The vertex adjacency of the triangle mesh ``faces [F,3] int32`` over ``V`` vertices, in the fixed order :func:`smooth` sums in:
    ``offsets [V+1] int64`` and ``neighbours [E] int32`` (the neighbours of vertex i are ``neighbours[offsets[i]:offsets[i+1]]``: distinct,
    ascending, symmetric, no self-loops; a degenerate face ``(a, a, b)`` still makes a and b neighbours), ``degree_max`` (int),
    ``boundary [V] bool`` (a vertex on an undirected edge that exactly one face side uses: the uses of {i, j} are counted over both
    directions, a duplicated face counts twice and ``(a, a, b)`` uses {a, b} twice) and ``edges_nonmanifold`` (the undirected edges with
    more than two uses).  Built from a stable sort of the 6 F half-edge entries by ``(i << 31) | j``.

    The faces are validated first (``mofa_cc_validate``, one host read): an index outside [0, V) raises ``MofaError`` before anything else
    runs; so do CPU tensors.  ``V == 0`` or ``F == 0`` gives an empty adjacency without a launch."""
    who = "vertex_adjacency"
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got CPU faces); there is no CPU fallback")
    if faces.dtype != torch.int32 or not faces.is_contiguous() or faces.dim() != 2 or faces.shape[1] != 3:
        raise lib.MofaError(f"{who}: want contiguous int32 faces [F,3], got {faces.dtype} {tuple(faces.shape)} contiguous={faces.is_contiguous()}")
    if isinstance(V, (bool, np.bool_)) or not isinstance(V, (int, np.integer)) or not 0 <= int(V) <= INT32_MAX:
        raise lib.MofaError(f"{who}: V = {V!r} (want an integer 0 .. 2^31 - 1)")
    V, F, dev = int(V), int(faces.shape[0]), faces.device
    if F > INT32_MAX:
        raise lib.MofaError(f"{who}: {F} faces exceed the int32 indices (2^31 - 1)")
    if V == 0 or F == 0:
        return {"offsets": torch.zeros(V + 1, dtype=torch.int64, device=dev), "neighbours": torch.zeros(0, dtype=torch.int32, device=dev),
                "degree_max": 0, "boundary": torch.zeros(V, dtype=torch.bool, device=dev), "edges_nonmanifold": 0}
    with torch.cuda.device(dev):
        adj = _adjacency(who, faces, V, F)
        degree_max, nonmanifold = (int(v) for v in torch.stack([adj["degree_max"], adj["edges_nonmanifold"]]).cpu())
    return {"offsets": adj["offsets"], "neighbours": adj["neighbours"], "degree_max": degree_max, "boundary": adj["boundary"],
            "edges_nonmanifold": nonmanifold}


def _smooth_args(who, iterations, lam, mu, weights, boundary):
    """smooth's parameters, checked before anything touches the GPU: (iterations, lam, mu or None)."""
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= SMOOTH_MAX_ITERATIONS:
        raise lib.MofaError(f"{who}: iterations = {iterations!r} (want an integer 0 .. {SMOOTH_MAX_ITERATIONS})")
    try:
        lam = float(lam)
        mu = None if mu is None else float(mu)
    except (TypeError, ValueError):
        raise lib.MofaError(f"{who}: lam = {lam!r}, mu = {mu!r} (want numbers; mu may be None)") from None
    if not 0.0 < lam <= 1.0:                                                  # (NaN fails both comparisons)
        raise lib.MofaError(f"{who}: lam = {lam} (want 0 < lam <= 1)")
    if mu is not None:
        if not (mu < -lam and np.isfinite(mu)):
            raise lib.MofaError(f"{who}: mu = {mu} (want None for plain Laplacian smoothing, or a finite mu < -lam = {-lam})")
        top = (1.0 - 2.0 * lam) * (1.0 - 2.0 * mu)
        if top < -1.0:
            raise lib.MofaError(f"{who}: lam = {lam}, mu = {mu} amplify the top frequency: (1 - 2 lam) (1 - 2 mu) = {top} < -1 (the "
                                "normalised operator's spectrum is [0, 2])")
    if weights not in _SMOOTH_WEIGHTS:
        raise lib.MofaError(f"{who}: weights = {weights!r} (want 'uniform' or 'cotangent')")
    if boundary not in _SMOOTH_BOUNDARIES:
        raise lib.MofaError(f"{who}: boundary = {boundary!r} (want 'fixed' or 'free')")
    return int(iterations), lam, mu


def smooth(verts: torch.Tensor, faces: torch.Tensor, iterations: int = 10, lam: float = 0.5, mu: Optional[float] = -0.53,
           weights: str = "uniform", boundary: str = "fixed", pinned: Optional[torch.Tensor] = None, timing: bool = False):
    """Taubin lambda | mu smoothing of a triangle mesh's vertices on the GPU (``mofa_smooth_*``): every iteration is a Laplacian step
    ``x += lam L(x)`` followed by one with ``mu < -lam``, a low-pass filter with the transfer function ``(1 - lam k)(1 - mu k)`` over the
    normalised Laplacian's spectrum k in [0, 2] that does not shrink the surface the way plain Laplacian smoothing does.  ``mu=None`` is
    that plain smoothing, one step per iteration: the shrinking baseline.  The defaults are Taubin's published pair, not a tuned one.

    ``L(x)_i`` is the weighted mean of ``x_j - x_i`` over the neighbours j of i in :func:`vertex_adjacency`'s order.  ``weights="uniform"``
    weighs them equally; ``"cotangent"`` uses ``w_ij = max(0, sum of 0.5 cot(the angle opposite {i, j}))``, computed once on the input
    positions (clamped, so that an obtuse pair cannot push a vertex away; frozen, so that the filter stays linear).  All sums are fp64 in a
    fixed order with every operation rounded separately (include/mofanerf_hip.h states them line for line), each step rounds to fp32 once,
    and there is no float atomic: the same mesh gives the same bytes every time.  ``boundary="fixed"`` pins the boundary vertices of
    :func:`vertex_adjacency`, ``"free"`` lets them move (an open border then shrinks inward); ``pinned [V] bool`` is OR-ed in.  A pinned
    vertex, a vertex without neighbours and, with cotangent weights, one whose weights sum to zero keep their bits.  ``faces`` is never
    touched: numbering and topology stay, and the input tensors are not written.

    Returns ``(verts' [V,3] float32, stats)``; ``stats``: ``passes`` (steps run), ``n_pinned``, ``n_boundary``, ``n_isolated`` (vertices
    without neighbours), ``degree_max``, ``edges_nonmanifold``, ``flat_corners`` (corners whose cotangent was set to 0), ``negative_weights``
    (directed pairs clamped), ``zero_weight`` (the last pass's vertices kept for a zero weight sum), ``displacement [V] float32`` (|out - in|
    from fp64) and ``max_displacement`` and, with ``timing=True``, ``times`` (seconds of the ``adjacency``, ``weights``, ``passes`` and
    ``stats`` phases, each ended by a device synchronisation).

    Raises ``MofaError`` — before anything touches the GPU — for ``iterations`` not an integer in 0 .. 1000, ``lam`` outside (0, 1], ``mu``
    not ``None`` and not below ``-lam``, a pair with ``(1 - 2 lam)(1 - 2 mu) < -1`` (it would amplify the top frequency) and unknown
    ``weights`` / ``boundary``; then for CPU tensors, a face index outside the mesh (after ``mofa_cc_validate``, before any other kernel)
    and a non-finite vertex some face references.  ``iterations=0``, ``V == 0`` or ``F == 0`` return the input's bits without a launch of
    the library (and statistics of zeros).  Smoothing moves vertices off the surface they were extracted from; what it does to a trained
    face has not been measured."""
    who = "smooth"
    iterations, lam, mu = _smooth_args(who, iterations, lam, mu, weights, boundary)
    V, F, dev = _mesh_tensors(who, verts, faces)
    if pinned is not None and (not torch.is_tensor(pinned) or pinned.dtype != torch.bool or pinned.shape != (V,) or pinned.device != dev):
        raise lib.MofaError(f"{who}: want pinned = None or a bool mask [{V}] on {dev}")
    passes = iterations * (1 if mu is None else 2)
    stats = dict.fromkeys(("passes", "n_pinned", "n_boundary", "n_isolated", "degree_max", "edges_nonmanifold", "flat_corners",
                           "negative_weights", "zero_weight"), 0)
    stats.update(displacement=torch.zeros(V, dtype=torch.float32, device=dev), max_displacement=0.0)
    if iterations == 0 or V == 0 or F == 0:
        return verts.clone(), stats
    L = lib.load()
    times, clock = {}, [time.perf_counter()]

    def lap(phase):
        if timing:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            times[phase] = now - clock[0]
            clock[0] = now

    with torch.cuda.device(dev):
        stream = lib.stream()
        lap("start")
        adj = _adjacency(who, faces, V, F)
        referenced = torch.zeros(V, dtype=torch.bool, device=dev)
        referenced[faces.reshape(-1).long()] = True
        pin = adj["boundary"].clone() if boundary == "fixed" else torch.zeros(V, dtype=torch.bool, device=dev)
        if pinned is not None:
            pin |= pinned
        head = torch.stack([(referenced & ~torch.isfinite(verts).all(1)).sum(), pin.sum(), adj["boundary"].sum(), adj["n_isolated"],
                            adj["degree_max"], adj["edges_nonmanifold"]]).cpu()
        n_bad, stats["n_pinned"], stats["n_boundary"], stats["n_isolated"], stats["degree_max"], stats["edges_nonmanifold"] = (int(v) for v in head)
        if n_bad:
            raise lib.MofaError(f"{who}: {n_bad} of the vertices the faces reference have a non-finite coordinate")
        offsets, nbr, perm, seg = adj["offsets"], adj["neighbours"], adj["perm"], adj["seg"]
        E, P = int(nbr.shape[0]), int(perm.shape[0])
        lap("adjacency")
        if E == 0:                                                            # (every face is of the form (a, a, a): nobody has a neighbour)
            if timing:
                times.pop("start")
                stats["times"] = times
            return verts.clone(), stats
        counts = torch.zeros(passes + 1, len(_SMOOTH_COUNTS), dtype=torch.int64, device=dev)      # row 0: the weights; row 1 + p: pass p
        w = None
        if weights == "cotangent":
            cots = torch.empty(F, 3, dtype=torch.float64, device=dev)
            lib.check(L.mofa_smooth_corner_cots(lib.ptr(verts), faces.data_ptr(), F, V, cots.data_ptr(), counts.data_ptr(), stream),
                      "mofa_smooth_corner_cots")
            w = torch.empty(E, dtype=torch.float64, device=dev)
            lib.check(L.mofa_smooth_edge_weights(cots.data_ptr(), F, perm.data_ptr(), P, seg.data_ptr(), E, w.data_ptr(), counts.data_ptr(),
                                                 stream), "mofa_smooth_edge_weights")
        lap("weights")
        pin8 = pin.to(torch.uint8) if (boundary == "fixed" or pinned is not None) else None
        bufs = (torch.empty_like(verts), torch.empty_like(verts))             # the input is read by the first pass only, never written
        src = verts
        for p in range(passes):
            dst = bufs[p % 2]
            lib.check(L.mofa_smooth_step(lib.ptr(src), V, offsets.data_ptr(), nbr.data_ptr(), E, None if w is None else w.data_ptr(),
                                         None if pin8 is None else pin8.data_ptr(), lam if (mu is None or p % 2 == 0) else mu, lib.ptr(dst),
                                         counts.data_ptr() + 8 * len(_SMOOTH_COUNTS) * (p + 1), stream), "mofa_smooth_step")
            src = dst
        lap("passes")
        c = counts.cpu().numpy()                                              # the counters, read once
        n_bad = int(c[:, _SMOOTH_COUNTS.index("bad_index")].sum())
        if n_bad:
            raise lib.MofaError(f"{who}: {n_bad} indices were out of range inside the passes (the mesh changed while it was smoothed?)")
        d = src.double() - verts.double()
        stats["displacement"] = torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).float()
        stats["max_displacement"] = float(stats["displacement"].max())
        lap("stats")
    stats.update(passes=passes, flat_corners=int(c[0, 0]), negative_weights=int(c[0, 1]), zero_weight=int(c[passes, 2]))
    if timing:
        times.pop("start")
        stats["times"] = times
    return src, stats


ICP_TERMS = 36           # MOFA_ICP_TERMS: the 28 + 7 + 1 sums of a step
ICP_CHUNK = 1024         # MOFA_ICP_CHUNK: rows per first-level sum
ICP_MAX_ITERATIONS = 10000
_ICP_METRIC = {"point": 0, "plane": 1}                                                                          # MOFA_ICP_POINT / _PLANE
_ICP_MODEL = {"translation": (3, 4, 5), "rigid": (0, 1, 2, 3, 4, 5), "similarity": (0, 1, 2, 3, 4, 5, 6)}       # the unknowns solved for
_ICP_IDENTITY = (1.0, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0))


# ---- the host side of a registration step: plain IEEE fp64 (+ - * / sqrt), every operation in the order DESIGN 3.22 writes down ----------
def _quat_unit(q):
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return (q[0] / n, q[1] / n, q[2] / n, q[3] / n)


def _quat_mul(a, b):
    return (((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3], ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
            ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1], ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0])


def _quat_rotation(q):
    w, x, y, z = q
    return (1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y))


def _rotation_quat(R):
    """The unit quaternion of a rotation matrix (9 floats, row-major) by Shepperd's choice of the largest pivot."""
    tr = (R[0] + R[4]) + R[8]
    if tr > 0.0:
        S = math.sqrt(tr + 1.0) * 2.0
        q = (0.25 * S, (R[7] - R[5]) / S, (R[2] - R[6]) / S, (R[3] - R[1]) / S)
    elif R[0] > R[4] and R[0] > R[8]:
        S = math.sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0
        q = ((R[7] - R[5]) / S, 0.25 * S, (R[1] + R[3]) / S, (R[2] + R[6]) / S)
    elif R[4] > R[8]:
        S = math.sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0
        q = ((R[2] - R[6]) / S, (R[1] + R[3]) / S, 0.25 * S, (R[5] + R[7]) / S)
    else:
        S = math.sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0
        q = ((R[3] - R[1]) / S, (R[2] + R[6]) / S, (R[5] + R[7]) / S, 0.25 * S)
    return _quat_unit(q)


def _icp_solve(sums, unknowns):
    """The step ``x [7]`` (zeros outside ``unknowns``) of ``(sum A) x = -(sum g)`` restricted to ``unknowns``, by Cholesky; None when a pivot
    is not positive and finite, or the solution is not finite."""
    H = [[0.0] * 7 for _ in range(7)]
    k = 0
    for a in range(7):
        for b in range(a, 7):
            H[a][b] = H[b][a] = sums[k]
            k += 1
    n = len(unknowns)
    Lm = [[0.0] * n for _ in range(n)]
    for j in range(n):
        s = H[unknowns[j]][unknowns[j]]
        for k in range(j):
            s = s - Lm[j][k] * Lm[j][k]
        if not (s > 0.0 and math.isfinite(s)):
            return None
        Lm[j][j] = math.sqrt(s)
        for i in range(j + 1, n):
            s = H[unknowns[i]][unknowns[j]]
            for k in range(j):
                s = s - Lm[i][k] * Lm[j][k]
            Lm[i][j] = s / Lm[j][j]
    z = [0.0] * n
    for i in range(n):
        s = -sums[28 + unknowns[i]]
        for k in range(i):
            s = s - Lm[i][k] * z[k]
        z[i] = s / Lm[i][i]
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = z[i]
        for k in range(i + 1, n):
            s = s - Lm[k][i] * x[k]
        x[i] = s / Lm[i][i]
    if not all(math.isfinite(v) for v in x):
        return None
    full = [0.0] * 7
    for j, i in enumerate(unknowns):
        full[i] = x[j]
    return full


def _icp_compose(state, x, mu):
    """(s, q, t) after the step ``x`` about the pivot ``mu``; None when the step's scale 1 + sigma is not positive."""
    s, q, t = state
    ds = 1.0 + x[6]
    if not ds > 0.0:
        return None
    dq = _quat_unit((1.0, 0.5 * x[0], 0.5 * x[1], 0.5 * x[2]))
    dR = _quat_rotation(dq)
    u = (t[0] - mu[0], t[1] - mu[1], t[2] - mu[2])
    t = tuple((ds * ((dR[3 * r] * u[0] + dR[3 * r + 1] * u[1]) + dR[3 * r + 2] * u[2]) + mu[r]) + x[3 + r] for r in range(3))
    return ds * s, _quat_unit(_quat_mul(dq, q)), t


def _icp_step_size(x, extent):
    return max(max(abs(x[0]), abs(x[1]), abs(x[2])), max(abs(x[3]), abs(x[4]), abs(x[5])) / extent, abs(x[6]))


def _icp_extent(box):
    """(the centre [3], the largest edge or 1) of a float32 box [2,3], in fp64."""
    lo, hi = (np.asarray(b, dtype=np.float32).astype(np.float64) for b in box)
    extent = float((hi - lo).max())
    return tuple(float(v) for v in (lo + hi) * 0.5), extent if extent > 0.0 else 1.0


def _icp_init(who, init):
    """``init`` (None, a result dict of fit_transform / register, or a 4 x 4 similarity matrix) as (s, q, t)."""
    if init is None:
        return _ICP_IDENTITY
    try:
        if isinstance(init, dict):
            s = float(init["scale"])
            R = np.asarray(_host(init["rotation"]), dtype=np.float64).reshape(3, 3)
            t = np.asarray(_host(init["translation"]), dtype=np.float64).reshape(3)
        else:
            M = np.asarray(_host(init), dtype=np.float64).reshape(4, 4)
            s = math.sqrt((M[0, 0] * M[0, 0] + M[0, 1] * M[0, 1]) + M[0, 2] * M[0, 2])
            with np.errstate(all="ignore"):
                R, t = M[:3, :3] / s, M[:3, 3]
    except (KeyError, TypeError, ValueError) as e:
        raise lib.MofaError(f"{who}: init = {init!r} (want None, a dict with scale / rotation / translation, or a 4 x 4 matrix): {e}")
    if not (np.isfinite(s) and s > 0 and np.isfinite(R).all() and np.isfinite(t).all()):
        raise lib.MofaError(f"{who}: init needs a finite transform with scale > 0")
    q = _rotation_quat([float(v) for v in R.reshape(-1)])
    if not all(math.isfinite(v) for v in q):
        raise lib.MofaError(f"{who}: init's rotation block is no rotation")
    return s, q, tuple(float(v) for v in t)


def _icp_args(who, model, metric, iterations, tol):
    if model not in _ICP_MODEL:
        raise lib.MofaError(f"{who}: model = {model!r} (want 'rigid', 'similarity' or 'translation')")
    if metric not in _ICP_METRIC:
        raise lib.MofaError(f"{who}: metric = {metric!r} (want 'point' or 'plane')")
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not 0 <= int(iterations) <= ICP_MAX_ITERATIONS:
        raise lib.MofaError(f"{who}: iterations = {iterations!r} (want an integer 0 .. {ICP_MAX_ITERATIONS})")
    tol = float(tol)
    if not tol >= 0:
        raise lib.MofaError(f"{who}: tol = {tol} (want >= 0)")
    return int(iterations), tol


def _icp_weight(who, weight, N, dev):
    if weight is None:
        return torch.ones(N, dtype=torch.float64, device=dev)
    if not torch.is_tensor(weight) or not weight.is_cuda:
        raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got a CPU weight); there is no CPU fallback")
    if weight.dtype != torch.float64 or weight.shape != (N,) or weight.device != dev:
        raise lib.MofaError(f"{who}: want float64 weight [{N}] on {dev}, got {weight.dtype} {tuple(weight.shape)} on {weight.device}")
    if N and not bool((weight >= 0).all()):
        raise lib.MofaError(f"{who}: the weights must be >= 0 (and not NaN)")
    return weight.contiguous()


def _icp_result(state, moved, history, iterations, status):
    s, q, t = state
    R = np.array(_quat_rotation(q), dtype=np.float64).reshape(3, 3)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    return {"scale": float(s), "rotation": R, "translation": np.array(t, dtype=np.float64), "matrix": M, "moved": moved, "history": history,
            "iterations": iterations, "status": status}


def _icp_apply(points, N, state, out=None):
    s, q, t = state
    out = torch.empty_like(points) if out is None else out
    T = (C.c_double * 13)(s, *_quat_rotation(q), *t)
    lib.check(lib.load().mofa_icp_apply(lib.ptr(points), N, T, lib.ptr(out), lib.stream()), "mofa_icp_apply")
    return out


def _icp_reduce(rows, M, ncols):
    """The one row left of ``rows [M, ncols]`` (float64) after mofa_icp_reduce, level by level."""
    L = lib.load()
    while M > 1:
        n = (M + ICP_CHUNK - 1) // ICP_CHUNK
        out = torch.empty(n, ncols, dtype=torch.float64, device=rows.device)
        lib.check(L.mofa_icp_reduce(rows.data_ptr(), M, ncols, out.data_ptr(), lib.stream()), "mofa_icp_reduce")
        rows, M = out, n
    return rows.reshape(-1)


def _icp_sums(moved, target, normals, face, verts, V, faces, F, weight, N, mu, metric):
    """The 36 sums of a step and the sum of the weights, on the host: 37 floats after one read."""
    L, dev = lib.load(), moved.device
    n = (N + ICP_CHUNK - 1) // ICP_CHUNK
    partial = torch.empty(n, ICP_TERMS, dtype=torch.float64, device=dev)
    plane = metric == "plane"
    lib.check(L.mofa_icp_terms_reduce(lib.ptr(moved), lib.ptr(target), lib.ptr(normals) if plane and normals is not None else None,
                                      face.data_ptr() if plane and face is not None else None, lib.ptr(verts) if verts is not None else None, V,
                                      faces.data_ptr() if faces is not None else None, F, weight.data_ptr(), N, _d3(mu), _ICP_METRIC[metric],
                                      partial.data_ptr(), lib.stream()), "mofa_icp_terms_reduce")
    wsum = torch.empty(n, 1, dtype=torch.float64, device=dev)
    lib.check(L.mofa_icp_reduce(weight.data_ptr(), N, 1, wsum.data_ptr(), lib.stream()), "mofa_icp_reduce")
    return [float(v) for v in torch.cat([_icp_reduce(partial, n, ICP_TERMS), _icp_reduce(wsum, n, 1)]).cpu()]


def _icp_update(state, sums, unknowns, mu, extent, entry):
    """One solve and composition: (the new state or None, the status that ends the loop or None); fills ``entry``'s rms and step."""
    entry["rms"] = math.sqrt(sums[35] / sums[36]) if sums[36] > 0.0 else float("nan")
    entry["step"] = float("nan")
    if entry["used"] == 0:
        return None, "no_correspondences"
    x = _icp_solve(sums, unknowns)
    new = None if x is None else _icp_compose(state, x, mu)
    if new is None:
        return None, "singular"
    entry["step"] = _icp_step_size(x, extent)
    return new, None


def transform_points(points: torch.Tensor, scale, rotation, translation) -> torch.Tensor:
    """``scale · rotation · x + translation`` for every row of ``points [N,3] float32`` on the GPU (``mofa_icp_apply``): the sum of a row of
    ``rotation`` (3 x 3) left to right, times ``scale``, plus ``translation``, in fp64, rounded once to float32.  ``N == 0`` launches nothing.
    Raises ``MofaError`` for a CPU tensor, a wrong dtype or shape, or a transform that is not finite."""
    who = "transform_points"
    lib.ptr(points)
    N = _query_points(who, points, points.device)
    try:
        s = float(scale)
        R = np.asarray(_host(rotation), dtype=np.float64).reshape(3, 3)
        t = np.asarray(_host(translation), dtype=np.float64).reshape(3)
    except (TypeError, ValueError) as e:
        raise lib.MofaError(f"{who}: want a scalar scale, a 3 x 3 rotation and a translation of 3: {e}")
    if not (np.isfinite(s) and np.isfinite(R).all() and np.isfinite(t).all()):
        raise lib.MofaError(f"{who}: the transform is not finite")
    out = torch.empty_like(points)
    if N == 0:
        return out
    with torch.cuda.device(points.device):
        T = (C.c_double * 13)(s, *[float(v) for v in R.reshape(-1)], *[float(v) for v in t])
        lib.check(lib.load().mofa_icp_apply(lib.ptr(points), N, T, lib.ptr(out), lib.stream()), "mofa_icp_apply")
    return out


def fit_transform(src: torch.Tensor, dst: torch.Tensor, weight: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
                  model: str = "rigid", metric: str = "point", iterations: int = 8, init=None, tol: float = 0.0) -> dict:
    """The transform ``x -> s R x + t`` that takes the points ``src [N,3] float32`` onto their partners ``dst [N,3] float32`` (landmarks: row
    i of one belongs to row i of the other), by the estimation step of :func:`register` — the same kernels, the same host solve — run
    ``iterations`` times from ``init``; its result is a good ``init`` for :func:`register`.  ``model``: ``"translation"``, ``"rigid"`` or
    ``"similarity"``; ``metric="plane"`` measures along ``normals [N,3] float32`` (unit normals at ``dst``, taken as they are).  ``weight [N]
    float64`` (>= 0; 0 leaves a pair out).  A pair with a non-finite coordinate is left out and counted.  The pivot is the centre of
    ``dst``'s box.  Returns what :func:`register` returns.  ``N == 0``: the identity (or ``init``), ``status="empty"``, no launch."""
    who = "fit_transform"
    lib.ptr(src), lib.ptr(dst)
    N = _query_points(who, src, src.device)
    dev = src.device
    if _query_points(who, dst, dev) != N:
        raise lib.MofaError(f"{who}: {N} source points, {dst.shape[0]} partners")
    iterations, tol = _icp_args(who, model, metric, iterations, tol)
    if metric == "plane":
        if normals is None:
            raise lib.MofaError(f"{who}: the plane metric needs normals [N,3]")
        if _query_points(who, normals, dev) != N:
            raise lib.MofaError(f"{who}: {N} points, {normals.shape[0]} normals")
    weight = _icp_weight(who, weight, N, dev)
    state = _icp_init(who, init)
    if N == 0:
        return _icp_result(state, torch.empty_like(src), [], 0, "empty")
    history, status, done = [], "iterations", 0
    with torch.cuda.device(dev):
        finite = torch.isfinite(dst).all(1)
        mu, extent = _icp_extent(torch.stack([dst[finite].amin(0), dst[finite].amax(0)]).cpu().numpy()) if bool(finite.any()) else ((0.0,) * 3, 1.0)
        moved = torch.empty_like(src)
        for _ in range(iterations):
            _icp_apply(src, N, state, moved)
            ok = finite & torch.isfinite(moved).all(1)
            w = torch.where(ok, weight, torch.zeros_like(weight))
            used, bad = (int(v) for v in torch.stack([(w > 0).sum(), (~ok).sum()]).cpu())
            entry = {"used": used, "rejected": {"non_finite": bad}}
            history.append(entry)
            sums = _icp_sums(moved, dst, normals, None, None, 0, None, 0, w, N, mu, metric)
            new, stop = _icp_update(state, sums, _ICP_MODEL[model], mu, extent, entry)
            if stop:
                status = stop
                break
            state, done = new, done + 1
            if entry["step"] <= tol:
                status = "converged"
                break
        _icp_apply(src, N, state, moved)
    return _icp_result(state, moved, history, done, status)


def _border_flags(who, faces, V, F):
    """(face_border [F] uint8: bit k = the edge opposite corner k is used once over both directions; vert_border [V] uint8)."""
    adj = _adjacency(who, faces, V, F)
    run = adj["seg"][1:] - adj["seg"][:-1]
    entry = adj["perm"][torch.repeat_interleave(run, run) == 1]
    corner = entry[(entry & 1) == 0] >> 1                       # both directions of a border edge are runs of one: take dir 0
    bits = torch.zeros(F, 3, dtype=torch.uint8, device=faces.device)
    bits.view(-1)[corner] = 1
    return (bits[:, 0] | (bits[:, 1] << 1) | (bits[:, 2] << 2)).contiguous(), adj["boundary"].to(torch.uint8).contiguous()


def register(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, model: str = "rigid", metric: str = "plane", iterations: int = 30,
             init=None, weight: Optional[torch.Tensor] = None, max_distance=None, trim=None, reject_border: bool = True, tol: float = 0.0,
             pivot=None, grid=None, timing: bool = False) -> dict:
    """Registers the points ``points [N,3] float32`` onto the triangle mesh ``(verts [V,3] float32, faces [F,3] int32)`` by iterated closest
    points on the GPU: finds ``x -> s R x + t`` (``model``: ``"translation"``, ``"rigid"``, ``"similarity"``) such that the moved points lie on
    the mesh.  The target is binned once (closest_points' grid; ``grid`` as there: it changes no bit); every iteration then

    1. moves the points (``mofa_icp_apply``),
    2. finds their exact closest points (``mofa_dist_query``, bounded by ``max_distance``),
    3. rejects a correspondence that is not finite, has no face (with ``max_distance``: lies beyond it) or — ``reject_border`` — whose closest
       point lies on a border edge or border vertex of the mesh (``mofa_icp_reject``: where an open mesh ends, the closest point of
       everything past the end is the rim, and those pairs pull the fit inwards),
    4. ``trim`` in (0, 1]: of the n correspondences left with a weight > 0 keeps those whose squared distance is at most the
       ``ceil(trim n)``-th smallest (ties all kept),
    5. sums the normal equations of the linearised step about ``pivot`` (None: the centre of the mesh's box) in a fixed order
       (``mofa_icp_terms_reduce`` / ``mofa_icp_reduce``): ``metric="plane"`` measures along the closest face's normal and converges
       quadratically near the answer, ``"point"`` measures the full offset and converges linearly,
    6. solves them on the host by Cholesky and composes the transform through a unit quaternion; no transcendental is involved, so the
       whole loop is a fixed sequence of IEEE operations: the same input gives the same bytes.

    ``weight [N] float64`` (>= 0): a point of weight 0 is moved but left out of the fit.  Returns a dict: ``scale`` (float), ``rotation
    [3,3]``, ``translation [3]``, ``matrix [4,4]`` (NumPy float64), ``moved [N,3] float32``, ``history`` (per iteration: ``rms`` — weighted, of
    the residuals the step was computed from —, ``used``, ``rejected`` by cause, ``step`` = max(|omega|, |tau| / extent, |sigma|)),
    ``iterations`` (steps taken) and ``status``: ``"converged"`` (step <= ``tol``), ``"iterations"``, ``"singular"`` (a pivot of the Cholesky
    factor is not positive — a plane lets the points slide — or the step's scale is not; the last transform is kept),
    ``"no_correspondences"`` (also a mesh without faces) or ``"empty"`` (``N == 0``: the identity, or ``init``, and no launch).  ``timing=True``
    adds ``times``: seconds of ``bin`` and, summed over the iterations, of ``query``, ``terms`` (steps 3 - 5) and ``host``, each ended by a
    device synchronisation.  A local method: it finds the nearest minimum, so start it from :func:`fit_transform` of a few landmarks when the
    meshes are far apart.

    Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, a face index outside the mesh, a non-finite target vertex, negative
    weights, ``trim`` outside (0, 1], ``max_distance`` not > 0, an unknown model or metric and a grid out of range."""
    who = "register"
    V, F, dev = _mesh_tensors(who, verts, faces)
    N = _query_points(who, points, dev)
    iterations, tol = _icp_args(who, model, metric, iterations, tol)
    maxd = _max_distance(who, max_distance)
    grid = _dist_grid_arg(who, grid)
    if trim is not None:
        trim = float(trim)
        if not 0.0 < trim <= 1.0:
            raise lib.MofaError(f"{who}: trim = {trim} (want in (0, 1], or None)")
    if pivot is not None:
        pivot = tuple(float(v) for v in np.asarray(pivot, dtype=np.float64).reshape(3))
        if not all(math.isfinite(v) for v in pivot):
            raise lib.MofaError(f"{who}: pivot = {pivot} (want finite)")
    weight = _icp_weight(who, weight, N, dev)
    state = _icp_init(who, init)
    if N == 0:
        return _icp_result(state, points.clone(), [], 0, "empty")
    if V == 0 or F == 0:
        with torch.cuda.device(dev):
            return _icp_result(state, _icp_apply(points, N, state), [], 0, "no_correspondences")
    history, status, done, times = [], "iterations", 0, dict.fromkeys(("bin", "query", "terms", "host"), 0.0)

    def lap(name, since):
        if timing:
            torch.cuda.synchronize(dev)
            times[name] += time.perf_counter() - since
        return time.perf_counter()

    with torch.cuda.device(dev):
        clock = lap("bin", 0.0)
        times["bin"] = 0.0
        b = _dist_lists(who, verts, faces, V, F, grid)
        mu, extent = _icp_extent(b["box"])
        mu = pivot if pivot is not None else mu
        if reject_border:
            face_border, vert_border = _border_flags(who, faces, V, F)
            border = torch.empty(N, dtype=torch.uint8, device=dev)
        clock = lap("bin", clock)
        moved = torch.empty_like(points)
        zero = torch.zeros_like(weight)
        for _ in range(iterations):
            _icp_apply(points, N, state, moved)
            res = _dist_query(moved, N, verts, faces, V, F, b, maxd)
            clock = lap("query", clock)
            finite = torch.isfinite(moved).all(1) & (torch.isfinite(res["d2"]) | (res["face"] < 0))
            has = finite & (res["face"] >= 0)
            ok = has
            if reject_border:
                lib.check(lib.load().mofa_icp_reject(res["face"].data_ptr(), lib.ptr(res["bary"]), N, faces.data_ptr(), F, V, face_border.data_ptr(),
                                                     vert_border.data_ptr(), border.data_ptr(), lib.stream()), "mofa_icp_reject")
                on_border = has & (border != 0)
                ok = has & ~on_border
            else:
                on_border = torch.zeros_like(has)
            valid = ok & (weight > 0)
            keep = valid
            if trim is not None:
                d2v = res["d2"][valid]
                if d2v.numel():
                    k = min(max(int(math.ceil(trim * d2v.numel())), 1), d2v.numel())
                    keep = valid & (res["d2"] <= torch.sort(d2v).values[k - 1])          # (a value: no order of equal elements enters)
            w = torch.where(keep, weight, zero)
            n_used, n_bad, n_none, n_border, n_valid = (int(v) for v in torch.stack([keep.sum(), (~finite).sum(), (finite & ~has).sum(),
                                                                                     on_border.sum(), valid.sum()]).cpu())
            entry = {"used": n_used, "rejected": {"non_finite": n_bad, "beyond" if max_distance is not None else "no_face": n_none,
                                                  "border": n_border, "trimmed": n_valid - n_used}}
            history.append(entry)
            sums = _icp_sums(moved, res["closest"], None, res["face"], verts, V, faces, F, w, N, mu, metric)
            clock = lap("terms", clock)
            new, stop = _icp_update(state, sums, _ICP_MODEL[model], mu, extent, entry)
            clock = lap("host", clock)
            if stop:
                status = stop
                break
            state, done = new, done + 1
            if entry["step"] <= tol:
                status = "converged"
                break
        _icp_apply(points, N, state, moved)
    out = _icp_result(state, moved, history, done, status)
    out["grid"] = b["grid"]
    if timing:
        out["times"] = times
    return out


def register_meshes(verts_a: torch.Tensor, faces_a: torch.Tensor, verts_b: torch.Tensor, faces_b: torch.Tensor, spacing: float,
                    max_subdiv: int = 64, **register_kw) -> dict:
    """Registers mesh a onto mesh b (:func:`register`): the source points are a's surface quadrature (:func:`sample_faces` with ``spacing``
    and ``max_subdiv``) with its area weights, followed by a's vertices at weight 0 — moved along, left out of the fit.  Returns
    :func:`register`'s dict (``moved`` holds the samples, then the vertices) plus ``verts [V,3] float32``, a's vertices under the transform,
    and ``n_samples``."""
    who = "register_meshes"
    _mesh_tensors(who, verts_a, faces_a)
    _mesh_tensors(who, verts_b, faces_b)
    if "weight" in register_kw:
        raise lib.MofaError(f"{who}: the weights are the quadrature's; register() takes explicit ones")
    pts, _, weight = sample_faces(verts_a, faces_a, spacing, max_subdiv)
    S = int(pts.shape[0])
    src = torch.cat([pts, verts_a]).contiguous()
    weight = torch.cat([weight, torch.zeros(verts_a.shape[0], dtype=torch.float64, device=verts_a.device)])
    out = register(src, verts_b, faces_b, weight=weight, **register_kw)
    out["verts"], out["n_samples"] = out["moved"][S:].contiguous(), S
    return out


WARP_MAX_CG = 10000      # MOFA_WARP_MAX_CG
WARP_REC_RHO = 8         # MOFA_WARP_REC_RHO: the record's first rho; before it a, frozen, cause, steps, tol^2 (MOFA_WARP_REC_*)
_WARP_STOPS = {0: "iterations", 1: "tolerance", 2: "breakdown"}       # MOFA_WARP_STOP_*


def _warp_args(who, metric, stiffness, point_weight, cg_iterations, cg_tol):
    """The scalar parameters of warp_to / warp, checked before any tensor is looked at: (the stiffness schedule, point_weight, cg_tol)."""
    if metric not in _ICP_METRIC:
        raise lib.MofaError(f"{who}: metric = {metric!r} (want 'point' or 'plane')")
    try:
        levels = [float(a) for a in np.asarray(stiffness, dtype=np.float64).reshape(-1)]
        point_weight, cg_tol = float(point_weight), float(cg_tol)
    except (TypeError, ValueError):
        raise lib.MofaError(f"{who}: stiffness = {stiffness!r}, point_weight = {point_weight!r}, cg_tol = {cg_tol!r} (want numbers)") from None
    if not levels or not all(math.isfinite(a) and a >= 0.0 for a in levels):
        raise lib.MofaError(f"{who}: stiffness = {stiffness!r} (want one or more finite values >= 0)")
    if not (point_weight >= 0.0 and math.isfinite(point_weight)):
        raise lib.MofaError(f"{who}: point_weight = {point_weight} (want finite, >= 0)")
    if isinstance(cg_iterations, (bool, np.bool_)) or not isinstance(cg_iterations, (int, np.integer)) or not 1 <= int(cg_iterations) <= WARP_MAX_CG:
        raise lib.MofaError(f"{who}: cg_iterations = {cg_iterations!r} (want an integer 1 .. {WARP_MAX_CG})")
    if not 0.0 <= cg_tol < 1.0:
        raise lib.MofaError(f"{who}: cg_tol = {cg_tol} (want in [0, 1))")
    return levels, point_weight, cg_tol


def _warp_template(who, verts, faces, init):
    """The template of warp_to / warp on the GPU: (V, F, device, the adjacency or None when nobody has a neighbour, the start d [V,3] float64).
    Refuses a face index outside the mesh and a non-finite vertex that a face references."""
    V, F, dev = _mesh_tensors(who, verts, faces)
    if init is not None:
        if not torch.is_tensor(init) or not init.is_cuda:
            raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got a CPU init); there is no CPU fallback")
        if init.dtype != torch.float64 or init.shape != (V, 3) or init.device != dev:
            raise lib.MofaError(f"{who}: want init = None or a float64 displacement [{V},3] on {dev}, got {init.dtype} {tuple(init.shape)}")
        if V and not bool(torch.isfinite(init).all()):
            raise lib.MofaError(f"{who}: init is not finite")
    d = torch.zeros(V, 3, dtype=torch.float64, device=dev) if init is None else init.clone().contiguous()
    adj = None
    if V and F:
        with torch.cuda.device(dev):
            adj = _adjacency(who, faces, V, F)
            referenced = torch.zeros(V, dtype=torch.bool, device=dev)
            referenced[faces.reshape(-1).long()] = True
            n_bad = int((referenced & ~torch.isfinite(verts).all(1)).sum())
        if n_bad:
            raise lib.MofaError(f"{who}: {n_bad} of the vertices the faces reference have a non-finite coordinate")
    return V, F, dev, adj, d


def _warp_graph(adj, V, dev):
    """(offsets, neighbours, E) of the template's adjacency; without one every list is empty."""
    if adj is None:
        return torch.zeros(V + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), 0
    return adj["offsets"], adj["neighbours"], int(adj["neighbours"].shape[0])


def _warp_apply(verts, d, V, out):
    lib.check(lib.load().mofa_warp_apply(lib.ptr(verts), d.data_ptr(), V, lib.ptr(out), lib.stream()), "mofa_warp_apply")
    return out


class _WarpSolver:
    """The buffers of the per-vertex system and its solve, allocated once per call of warp_to / warp."""

    def __init__(self, V, graph, cg_iterations, cg_tol, dev):
        f64 = dict(dtype=torch.float64, device=dev)
        self.V, (self.offsets, self.nbr, self.E), self.K, self.tol = V, graph, cg_iterations, cg_tol
        self.D, self.b, self.minv, self.energy = torch.empty(V, 6, **f64), torch.empty(V, 3, **f64), torch.empty(V, 3, **f64), torch.empty(V, **f64)
        self.work = torch.empty(int(lib.load().mofa_warp_workspace_doubles(V)), **f64)
        self.rec = torch.empty(WARP_REC_RHO + cg_iterations + 1, **f64)
        self.bad_system = torch.zeros((V + 255) // 256, dtype=torch.int64, device=dev)
        self.bad_solve = torch.zeros((V + ICP_CHUNK - 1) // ICP_CHUNK, dtype=torch.int64, device=dev)

    def system(self, verts, moved, target, normals, face, tverts, TV, tfaces, TF, weight, hweight, hpos, metric, point_weight, alpha):
        plane = metric == "plane"
        lib.check(lib.load().mofa_warp_system(
            lib.ptr(verts), lib.ptr(moved), lib.ptr(target), lib.ptr(normals) if plane and normals is not None else None,
            face.data_ptr() if plane and face is not None else None, lib.ptr(tverts) if tverts is not None else None, TV,
            tfaces.data_ptr() if tfaces is not None else None, TF, weight.data_ptr(), None if hweight is None else hweight.data_ptr(),
            None if hpos is None else lib.ptr(hpos), self.offsets.data_ptr(), self.E, self.V, _ICP_METRIC[metric], point_weight, alpha,
            self.D.data_ptr(), self.b.data_ptr(), self.minv.data_ptr(), self.energy.data_ptr(), self.bad_system.data_ptr(), lib.stream()),
            "mofa_warp_system")

    def solve(self, alpha, x):
        """Enqueues the whole solve from ``x`` (float64 [V,3], overwritten); nothing is read back here."""
        lib.check(lib.load().mofa_warp_solve(self.D.data_ptr(), self.b.data_ptr(), self.minv.data_ptr(), self.offsets.data_ptr(),
                                             self.nbr.data_ptr() if self.E else None, self.E, self.V, alpha, self.K, self.tol, x.data_ptr(),
                                             self.work.data_ptr(), self.rec.data_ptr(), self.bad_solve.data_ptr(), lib.stream()), "mofa_warp_solve")

    def tail(self):
        """What the host reads after a solve, still on the device: the record, then the two bad-index counts."""
        return torch.cat([self.rec, torch.stack([self.bad_system.sum(), self.bad_solve.sum()]).double()])

    def record(self, who, tail):
        """(rho [K + 1], steps, stop) from the host copy of :meth:`tail`."""
        n_bad = int(tail[-2]) + int(tail[-1])
        if n_bad:
            raise lib.MofaError(f"{who}: {n_bad} indices were out of range inside the solve (the mesh changed while it was warped?)")
        return tail[WARP_REC_RHO:WARP_REC_RHO + self.K + 1].copy(), int(tail[3]), _WARP_STOPS[int(tail[2])]


_WARP_MODELS = ("displacement", "arap")


class _WarpArap:
    """The buffers of the as-rigid-as-possible stiffness, allocated once per call of warp / deform: the rotations fitted to the
    current d (``R [V,9]`` float64), those of the last iteration taken (``taken``), the per-vertex fit and the two kernels' counters."""

    def __init__(self, V, graph, dev):
        f64 = dict(dtype=torch.float64, device=dev)
        self.V, (self.offsets, self.nbr, self.E) = V, graph
        self.R, self.fit = torch.empty(V, 9, **f64), torch.empty(V, **f64)
        self.taken = torch.eye(3, **f64).reshape(1, 9).repeat(V, 1)
        self.sums = torch.empty((V + ICP_CHUNK - 1) // ICP_CHUNK, 1, **f64)
        self.bad_fit = torch.zeros((V + 255) // 256, 2, dtype=torch.int64, device=dev)
        self.bad_rhs = torch.zeros((V + 255) // 256, dtype=torch.int64, device=dev)

    def _graph(self):
        return self.offsets.data_ptr(), self.nbr.data_ptr() if self.E else None, self.E, self.V

    def rotations(self, verts, d):
        """Fits ``R`` to the displacement ``d`` (``mofa_warp_rotations``); returns the sum of the fit, one number still on the device."""
        L = lib.load()
        lib.check(L.mofa_warp_rotations(lib.ptr(verts), d.data_ptr(), *self._graph(), self.R.data_ptr(), self.fit.data_ptr(),
                                        self.bad_fit.data_ptr(), lib.stream()), "mofa_warp_rotations")
        lib.check(L.mofa_icp_reduce(self.fit.data_ptr(), self.V, 1, self.sums.data_ptr(), lib.stream()), "mofa_icp_reduce")
        return _icp_reduce(self.sums, int(self.sums.shape[0]), 1)

    def amend(self, verts, alpha, b):
        """b += alpha g(R) (``mofa_warp_arap_rhs``)."""
        lib.check(lib.load().mofa_warp_arap_rhs(lib.ptr(verts), self.R.data_ptr(), *self._graph(), alpha, b.data_ptr(), self.bad_rhs.data_ptr(),
                                                lib.stream()), "mofa_warp_arap_rhs")

    def tail(self, fit_sum):
        """What the host reads of an iteration, still on the device: the sum of the fit, the index faults, the non-finite fits."""
        return torch.cat([fit_sum.reshape(1), torch.stack([self.bad_fit[:, 0].sum() + self.bad_rhs.sum(), self.bad_fit[:, 1].sum()]).double()])

    def energy(self, who, tail):
        """``arap_energy`` from the host copy of :meth:`tail`."""
        if int(tail[1]):
            raise lib.MofaError(f"{who}: {int(tail[1])} indices were out of range inside the rotation fit (the mesh changed while it was warped?)")
        return 0.5 * float(tail[0])

    def take(self):
        self.R, self.taken = self.taken, self.R

    def result(self):
        return self.taken.reshape(self.V, 3, 3)


def warp_to(verts: torch.Tensor, faces: torch.Tensor, targets: torch.Tensor, weight: Optional[torch.Tensor] = None,
            normals: Optional[torch.Tensor] = None, metric: str = "point", stiffness: float = 1.0, point_weight: float = 1e-2, init=None,
            cg_iterations: int = 200, cg_tol: float = 1e-8):
    """Deforms the template ``(verts [V,3] float32, faces [F,3] int32)`` towards explicit per-vertex targets — row i of ``targets [V,3]
    float32`` belongs to vertex i — by ONE solve of the step :func:`warp` iterates (``mofa_warp_system`` / ``mofa_warp_solve``): the
    displacement ``d [V,3] float64`` that minimises

        ``sum_i w_i rho_i(v_i + d_i - c_i)  +  stiffness * sum_{edges {i,j}} |d_i - d_j|^2``

    over the undirected edges of :func:`vertex_adjacency`.  ``metric="point"``: ``rho_i(u) = |u|^2``; ``"plane"``: ``(n_i . u)^2 +
    point_weight |u|^2`` with ``normals [V,3] float32`` (unit normals at the targets, taken as they are; required).  ``weight [V] float64``
    (>= 0): a vertex of weight 0, or with a non-finite target, follows its neighbours through the stiffness term alone — landmark-driven
    deformation is this call with weight 0 everywhere but at the landmarks.  The normal equations are solved by Jacobi-preconditioned
    conjugate gradients from ``init`` (a displacement [V,3] float64; None: zero): exactly ``cg_iterations`` steps are enqueued and the host
    reads nothing in between; a flag in device memory freezes the solve once ``rho <= cg_tol^2 rho_0`` or the curvature ``p . A p`` is
    not positive, and a frozen step leaves every vector's bits alone.  Every sum has a fixed order (include/mofanerf_hip.h): the same input
    gives the same bytes.

    Returns ``(verts' [V,3] float32 = (float)(verts + d), d [V,3] float64, solve)``; ``solve``: ``rho`` (NumPy [cg_iterations + 1]: the
    preconditioned residual ``r . z`` after 0 .. cg_iterations steps), ``steps`` (those that moved d) and ``stop`` (``"tolerance"``,
    ``"breakdown"`` or ``"iterations"``).  A vertex without neighbours and without weight keeps its start.  ``V == 0`` launches nothing.
    ``faces`` and the numbering are never touched.  Raises ``MofaError`` for an unknown metric, a negative or non-finite stiffness or
    ``point_weight``, ``cg_iterations`` outside 1 .. 10000, ``cg_tol`` outside [0, 1) — all before any tensor is looked at —, CPU tensors,
    wrong dtypes or shapes, a face index outside the mesh, a non-finite vertex a face references and negative weights."""
    who = "warp_to"
    levels, point_weight, cg_tol = _warp_args(who, metric, stiffness, point_weight, cg_iterations, cg_tol)
    if len(levels) != 1:
        raise lib.MofaError(f"{who}: stiffness = {stiffness!r} (want one value; warp() takes a schedule)")
    V, F, dev, adj, d = _warp_template(who, verts, faces, init)
    if _query_points(who, targets, dev) != V:
        raise lib.MofaError(f"{who}: {V} vertices, {targets.shape[0]} targets")
    if metric == "plane":
        if normals is None:
            raise lib.MofaError(f"{who}: the plane metric needs normals [V,3]")
        if _query_points(who, normals, dev) != V:
            raise lib.MofaError(f"{who}: {V} vertices, {normals.shape[0]} normals")
    weight = _icp_weight(who, weight, V, dev)
    if V == 0:
        return verts.clone(), d, {"rho": np.zeros(0), "steps": 0, "stop": "iterations"}
    with torch.cuda.device(dev):
        ok = torch.isfinite(targets).all(1)
        if metric == "plane":
            ok &= torch.isfinite(normals).all(1)
        w = torch.where(ok, weight, torch.zeros_like(weight))
        solver = _WarpSolver(V, _warp_graph(adj, V, dev), int(cg_iterations), cg_tol, dev)
        moved = _warp_apply(verts, d, V, torch.empty_like(verts))
        solver.system(verts, moved, targets, normals, None, None, 0, None, 0, w, None, None, metric, point_weight, levels[0])
        solver.solve(levels[0], d)
        rho, steps, stop = solver.record(who, solver.tail().cpu().numpy())
        _warp_apply(verts, d, V, moved)
    return moved, d, {"rho": rho, "steps": steps, "stop": stop}


def _warp_handles(who, handles, V, dev):
    """``handles = (index [K], position [K,3] float32, weight: a scalar or [K] float64)`` as dense (weight [V] float64, position [V,3]
    float32) on the device, or (None, None)."""
    if handles is None:
        return None, None
    try:
        index, pos, hw = handles
    except (TypeError, ValueError):
        raise lib.MofaError(f"{who}: handles = (index [K], position [K,3], weight), got {type(handles).__name__}") from None
    for name, t in (("index", index), ("position", pos)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise lib.MofaError(f"{who}: the HIP path needs tensors on the GPU (got CPU handle {name}); there is no CPU fallback")
    if index.dtype not in (torch.int32, torch.int64) or index.dim() != 1 or index.device != dev:
        raise lib.MofaError(f"{who}: want handle indices [K] int32 or int64 on {dev}, got {index.dtype} {tuple(index.shape)} on {index.device}")
    K = int(index.shape[0])
    if pos.dtype != torch.float32 or pos.shape != (K, 3) or pos.device != dev:
        raise lib.MofaError(f"{who}: want handle positions [{K},3] float32 on {dev}, got {pos.dtype} {tuple(pos.shape)} on {pos.device}")
    if torch.is_tensor(hw):
        if hw.dtype != torch.float64 or hw.shape != (K,) or hw.device != dev:
            raise lib.MofaError(f"{who}: want handle weights a number or [{K}] float64 on {dev}, got {hw.dtype} {tuple(hw.shape)}")
    else:
        hw = torch.full((K,), float(hw), dtype=torch.float64, device=dev)
    index = index.long()
    if K:
        if not bool(((index >= 0) & (index < V)).all()):
            raise lib.MofaError(f"{who}: a handle index lies outside [0, {V})")
        if int(torch.unique(index).shape[0]) != K:
            raise lib.MofaError(f"{who}: a handle index is repeated")
        if not bool(torch.isfinite(pos).all()) or not bool((torch.isfinite(hw) & (hw >= 0)).all()):
            raise lib.MofaError(f"{who}: the handles need finite positions and finite weights >= 0")
    hweight, hpos = torch.zeros(V, dtype=torch.float64, device=dev), torch.zeros(V, 3, dtype=torch.float32, device=dev)
    hweight[index], hpos[index] = hw, pos
    return hweight, hpos


def warp(verts: torch.Tensor, faces: torch.Tensor, target_verts: torch.Tensor, target_faces: torch.Tensor, metric: str = "plane",
         stiffness=(10.0, 1.0, 0.1), iterations: int = 5, point_weight: float = 1e-2, weight: Optional[torch.Tensor] = None, handles=None,
         max_distance=None, reject_border: bool = True, init=None, tol: float = 0.0, cg_iterations: int = 200, cg_tol: float = 1e-8, grid=None,
         timing: bool = False, stiffness_model: str = "displacement") -> dict:
    """Warps the template ``(verts [V,3] float32, faces [F,3] int32)`` onto the target mesh ``(target_verts, target_faces)`` without touching
    its topology — non-rigid registration by stiffness-regularised iterated closest points with one translation per vertex (Amberg-style
    optimal-step N-ICP) —, so that meshes of different triangulations come out in ONE vertex numbering.  The unknown is a
    displacement ``d [V,3] float64``; the warped vertex is ``(float)(verts + d)``.  The target is binned once (closest_points' grid; ``grid``
    as there: it changes no bit).  For every level of the ``stiffness`` schedule, ``iterations`` times:

    1. the template is moved (``mofa_warp_apply``),
    2. its vertices' exact closest points are found (``mofa_dist_query``, bounded by ``max_distance``),
    3. a vertex is rejected from the data term when it is not finite, has no face (with ``max_distance``: lies beyond it) or —
       ``reject_border`` — when its closest point lies on the target's border (``mofa_icp_reject``); a rejected vertex keeps its stiffness
       rows and its handle,
    4. the per-vertex system of ``sum_i w_i rho_i(v_i + d_i - c_i) + alpha sum_{edges} |d_i - d_j|^2 + sum_l beta_l |v_l + d_l - p_l|^2`` is
       built (``mofa_warp_system``; ``metric`` and ``point_weight`` as in :func:`warp_to`, the normal that of the closest face),
    5. and solved by preconditioned conjugate gradients from the previous d (``mofa_warp_solve``: ``cg_iterations`` steps enqueued, frozen
       on the device at ``cg_tol``); the host reads one small record per iteration.

    Stiff levels move the template as a near-rigid sheet, loose ones let it take the target's detail.  The stiffness acts on the
    DISPLACEMENTS: it penalises a rotation of the template as much as a bend, so align first (:func:`register_meshes`).  ``weight [V]
    float64`` (>= 0) weighs the data term; ``handles = (index [K], position [K,3] float32, weight)`` pins landmark vertices to positions
    (a repeated index is refused).  A level ends early when ``max_i |delta d_i| <= tol * extent`` (the largest edge of the target's box).

    Returns a dict: ``verts [V,3] float32``, ``displacement [V,3] float64``, ``history`` (per iteration: ``stiffness``, ``rms`` — of the
    residuals the step was computed from, sqrt(sum w rho / sum w) —, ``used``, ``rejected`` by cause, ``cg_steps``, ``rho`` (the solve's last),
    ``stop`` and ``step`` = max |delta d_i|), ``iterations`` (solves taken), ``status`` — ``"iterations"``, ``"converged"`` (the last level
    ended on ``tol``), ``"no_correspondences"`` (no vertex kept; also a target without faces), ``"singular"`` (a solve's first step found
    ``p . A p > 0`` false with ``rho_0 > 0``; the last d is kept) or ``"empty"`` (``V == 0``: no launch) —, ``grid`` and, with
    ``timing=True``, ``times``: seconds of ``bin`` and, summed over the iterations, ``query`` (steps 1 - 2), ``system`` (3 - 4) and ``solve``,
    each ended by a device synchronisation.  Every sum has a fixed order and no transcendental is involved: the same input gives the same
    bytes.  A local method with no normal-compatibility test and no colour term.

    ``stiffness_model="arap"`` replaces the stiffness term by the as-rigid-as-possible one,
    ``alpha / 2 sum_i sum_{j in N(i)} |(y_i - y_j) - R_i (v_i - v_j)|^2`` with a rotation ``R_i`` per vertex: between steps 4 and 5 the rotations
    are fitted to the current d (``mofa_warp_rotations``: Horn's quaternion by a fixed number of Jacobi sweeps, always a proper rotation,
    the identity bit for bit at d = 0) and the right-hand side is amended (``mofa_warp_arap_rhs``); the matrix and the solve stay the same.
    A rotation of the template is then free and its edge lengths are kept.  Every history entry gains ``arap_energy`` (the term without
    alpha, at the d the iteration started from), the result ``rotations [V,3,3] float64`` (those of the last iteration taken; the identity
    before one) and ``times`` the key ``arap``.  Uniform edge weights only (no cotangent weights), a surface term (no volumetric rigidity),
    still a local method.  The default ``"displacement"`` runs exactly the launches described above and returns exactly those keys.

    Raises ``MofaError`` for an unknown ``stiffness_model``, the scalar arguments :func:`warp_to` refuses, an empty schedule, ``iterations`` outside 0 .. 10000, ``tol`` < 0
    (before any tensor is looked at), CPU tensors, wrong dtypes or shapes, face or handle indices outside the mesh, a non-finite template
    vertex that a face references, a non-finite target vertex or handle, negative weights, ``max_distance`` not > 0 and a grid out of
    range."""
    who = "warp"
    if stiffness_model not in _WARP_MODELS:
        raise lib.MofaError(f"{who}: stiffness_model = {stiffness_model!r} (want 'displacement' or 'arap')")
    levels, point_weight, cg_tol = _warp_args(who, metric, stiffness, point_weight, cg_iterations, cg_tol)
    iterations, tol = _icp_args(who, "rigid", metric, iterations, tol)
    maxd = _max_distance(who, max_distance)
    grid = _dist_grid_arg(who, grid)
    V, F, dev, adj, d = _warp_template(who, verts, faces, init)
    TV, TF, tdev = _mesh_tensors(who, target_verts, target_faces)
    if tdev != dev:
        raise lib.MofaError(f"{who}: the template on {dev}, the target on {tdev}")
    weight = _icp_weight(who, weight, V, dev)
    hweight, hpos = _warp_handles(who, handles, V, dev)

    arap = None

    def result(moved, history, done, status, g):
        out = {"verts": moved, "displacement": d, "history": history, "iterations": done, "status": status, "grid": g}
        if stiffness_model == "arap":
            out["rotations"] = arap.result() if arap is not None else torch.zeros(0, 3, 3, dtype=torch.float64, device=dev)
        return out

    if V == 0:
        return result(verts.clone(), [], 0, "empty", grid if grid is not None else (1, 1, 1))
    history, status, done, times = [], "iterations", 0, dict.fromkeys(("bin", "query", "system", "solve"), 0.0)
    if stiffness_model == "arap":
        times["arap"] = 0.0

    def lap(name, since):
        if timing:
            torch.cuda.synchronize(dev)
            times[name] += time.perf_counter() - since
        return time.perf_counter()

    with torch.cuda.device(dev):
        moved = torch.empty_like(verts)
        if stiffness_model == "arap":
            arap = _WarpArap(V, _warp_graph(adj, V, dev), dev)
        if TV == 0 or TF == 0:
            return result(_warp_apply(verts, d, V, moved), [], 0, "no_correspondences", grid if grid is not None else (1, 1, 1))
        clock = lap("bin", 0.0)
        times["bin"] = 0.0
        b = _dist_lists(who, target_verts, target_faces, TV, TF, grid)
        _, extent = _icp_extent(b["box"])
        if reject_border:
            face_border, vert_border = _border_flags(who, target_faces, TV, TF)
            border = torch.empty(V, dtype=torch.uint8, device=dev)
        solver = _WarpSolver(V, _warp_graph(adj, V, dev), int(cg_iterations), cg_tol, dev)
        zero = torch.zeros_like(weight)
        x = torch.empty_like(d)
        clock = lap("bin", clock)
        stopped = None
        for alpha in levels:
            status = "iterations"
            for _ in range(iterations):
                _warp_apply(verts, d, V, moved)
                res = _dist_query(moved, V, target_verts, target_faces, TV, TF, b, maxd)
                clock = lap("query", clock)
                finite = torch.isfinite(moved).all(1) & (torch.isfinite(res["d2"]) | (res["face"] < 0))
                has = finite & (res["face"] >= 0)
                if reject_border:
                    lib.check(lib.load().mofa_icp_reject(res["face"].data_ptr(), lib.ptr(res["bary"]), V, target_faces.data_ptr(), TF, TV,
                                                         face_border.data_ptr(), vert_border.data_ptr(), border.data_ptr(), lib.stream()),
                              "mofa_icp_reject")
                    on_border = has & (border != 0)
                else:
                    on_border = torch.zeros_like(has)
                keep = has & ~on_border & (weight > 0)
                w = torch.where(keep, weight, zero)
                solver.system(verts, moved, res["closest"], None, res["face"], target_verts, TV, target_faces, TF, w, hweight, hpos, metric,
                              point_weight, alpha)
                n = (V + ICP_CHUNK - 1) // ICP_CHUNK
                sums = torch.empty(2, n, 1, dtype=torch.float64, device=dev)
                for row, src in enumerate((solver.energy, w)):
                    lib.check(lib.load().mofa_icp_reduce(src.data_ptr(), V, 1, sums[row].data_ptr(), lib.stream()), "mofa_icp_reduce")
                head = torch.cat([_icp_reduce(sums[0], n, 1), _icp_reduce(sums[1], n, 1),
                                  torch.stack([keep.sum(), (~finite).sum(), (finite & ~has).sum(), on_border.sum()]).double()])
                clock = lap("system", clock)
                if arap is not None:
                    fit_sum = arap.rotations(verts, d)
                    arap.amend(verts, alpha, solver.b)
                    clock = lap("arap", clock)
                x.copy_(d)
                solver.solve(alpha, x)
                t = x - d
                step = torch.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]).max()
                if arap is None:
                    host = torch.cat([head, step.reshape(1), solver.tail()]).cpu().numpy()       # the one read of this iteration
                else:
                    host = torch.cat([head, step.reshape(1), solver.tail(), arap.tail(fit_sum)]).cpu().numpy()
                    host, fitted = host[:-3], host[-3:]
                clock = lap("solve", clock)
                sum_e, sum_w, (n_used, n_bad, n_none, n_border) = float(host[0]), float(host[1]), (int(v) for v in host[2:6])
                entry = {"stiffness": alpha, "rms": math.sqrt(sum_e / sum_w) if sum_w > 0.0 else float("nan"), "used": n_used,
                         "rejected": {"non_finite": n_bad, "beyond" if max_distance is not None else "no_face": n_none, "border": n_border},
                         "cg_steps": 0, "rho": float("nan"), "stop": None, "step": float("nan")}
                history.append(entry)
                if arap is not None:
                    entry["arap_energy"] = arap.energy(who, fitted)
                if n_used == 0:                                  # (the solve that was enqueued is not taken up)
                    stopped = "no_correspondences"
                    break
                rho, steps, stop = solver.record(who, host[7:])
                entry["cg_steps"], entry["rho"], entry["stop"] = steps, float(rho[-1]), stop
                if stop == "breakdown" and steps == 0 and rho[0] > 0.0:
                    stopped = "singular"
                    break
                entry["step"] = float(host[6])
                d, x = x, d
                done += 1
                if arap is not None:
                    arap.take()
                if entry["step"] <= tol * extent:
                    status = "converged"
                    break
            if stopped:
                status = stopped
                break
        _warp_apply(verts, d, V, moved)
    out = result(moved, history, done, status, b["grid"])
    if timing:
        out["times"] = times
    return out


def deform(verts: torch.Tensor, faces: torch.Tensor, handles, stiffness: float = 1.0, iterations: int = 40, init=None, tol: float = 0.0,
           cg_iterations: int = 200, cg_tol: float = 1e-8) -> dict:
    """Edits the mesh ``(verts [V,3] float32, faces [F,3] int32)`` by its handles — as-rigid-as-possible deformation (Sorkine and Alexa's
    local/global iteration): ``handles = (index [K], position [K,3] float32, weight)`` as in :func:`warp` pull landmark
    vertices to positions and the surface follows as rigidly as it can.  The unknown is a displacement ``d [V,3] float64`` that minimises

        ``stiffness / 2 sum_i sum_{j in N(i)} |(y_i - y_j) - R_i (v_i - v_j)|^2  +  sum_l beta_l |y_l - p_l|^2``,   ``y = v + d``,

    over d and one rotation ``R_i`` per vertex, on :func:`vertex_adjacency`'s lists with uniform edge weights.  ``iterations`` times: the
    rotations are fitted to the current d (``mofa_warp_rotations``: Horn's quaternion of the neighbourhood's covariance by a fixed number
    of Jacobi sweeps — always a proper rotation, also on a flat neighbourhood, and the identity bit for bit at d = 0); the system is built
    with the handles as the only data term (``mofa_warp_system``, every data weight 0), the rotation term is added to its right-hand side
    (``mofa_warp_arap_rhs``) and it is solved from the current d by the conjugate gradients of :func:`warp` (``mofa_warp_solve``); the host
    reads one small record per iteration.  ``init`` (a displacement [V,3] float64) starts the iteration elsewhere than at rest; it stops
    early when ``max_i |delta d_i| <= tol * extent`` (the largest edge of the vertices' box).

    Returns a dict: ``verts [V,3] float32 = (float)(verts + d)``, ``displacement [V,3] float64``, ``rotations [V,3,3] float64`` (those the
    last solve taken was built from; the identity before one), ``history`` (per iteration: ``arap_energy`` — the stiffness term without
    ``stiffness`` at the d the iteration started from, with its freshly fitted rotations —, ``cg_steps``, ``rho``, ``stop``, ``step``),
    ``iterations`` (solves taken) and ``status``: ``"iterations"``, ``"converged"``, ``"singular"`` (as in :func:`warp`) or ``"empty"``
    (``V == 0``: no launch).  Every sum has a fixed order: the same input gives the same bytes.

    What is fixed and what is not claimed: uniform edge weights only, no cotangent weights, so an irregular triangulation is stiffer where
    it is denser; a surface term, no volumetric or tetrahedral rigidity; a local method — it finds the rest-like pose near its start, not
    the global minimum; and local/global converges linearly, slowly when the handles are few: on the tests' 9 x 9 patch, 32 border handles
    reach 1e-5 of a rigid motion by 60 degrees in 40 iterations, five handles are still 6e-2 away after 40 and 1.6e-3 after 160 (a NumPy
    prototype; README).  A vertex without neighbours and without a handle keeps its start.  ``faces`` and the numbering are never touched.

    Raises ``MofaError`` for the scalar arguments :func:`warp_to` refuses (one stiffness), ``iterations`` outside 0 .. 10000, ``tol`` < 0
    (before any tensor is looked at), missing handles or handles without a positive weight, CPU tensors, wrong dtypes or shapes, face or
    handle indices outside the mesh and a non-finite vertex that a face references."""
    who = "deform"
    levels, _, cg_tol = _warp_args(who, "point", stiffness, 0.0, cg_iterations, cg_tol)
    if len(levels) != 1:
        raise lib.MofaError(f"{who}: stiffness = {stiffness!r} (want one value)")
    iterations, tol = _icp_args(who, "rigid", "point", iterations, tol)
    if handles is None:
        raise lib.MofaError(f"{who}: handles = (index [K], position [K,3], weight) are required: they are the only data term")
    alpha = levels[0]
    V, F, dev, adj, d = _warp_template(who, verts, faces, init)
    hweight, hpos = _warp_handles(who, handles, V, dev)
    if V == 0:
        return {"verts": verts.clone(), "displacement": d, "rotations": torch.zeros(0, 3, 3, dtype=torch.float64, device=dev), "history": [],
                "iterations": 0, "status": "empty"}
    with torch.cuda.device(dev):
        if not bool((hweight > 0).any()):
            raise lib.MofaError(f"{who}: no handle has a positive weight")
        _, extent = _icp_extent(torch.stack([verts.min(0).values, verts.max(0).values]).cpu().numpy())
        graph = _warp_graph(adj, V, dev)
        solver, arap = _WarpSolver(V, graph, int(cg_iterations), cg_tol, dev), _WarpArap(V, graph, dev)
        zero = torch.zeros(V, dtype=torch.float64, device=dev)
        x, moved = torch.empty_like(d), torch.empty_like(verts)
        history, status, done = [], "iterations", 0
        for _ in range(iterations):
            fit_sum = arap.rotations(verts, d)
            solver.system(verts, verts, verts, None, None, None, 0, None, 0, zero, hweight, hpos, "point", 0.0, alpha)
            arap.amend(verts, alpha, solver.b)
            x.copy_(d)
            solver.solve(alpha, x)
            t = x - d
            step = torch.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]).max()
            host = torch.cat([step.reshape(1), solver.tail(), arap.tail(fit_sum)]).cpu().numpy()       # the one read of this iteration
            entry = {"arap_energy": arap.energy(who, host[-3:]), "cg_steps": 0, "rho": float("nan"), "stop": None, "step": float("nan")}
            history.append(entry)
            rho, steps, stop = solver.record(who, host[1:-3])
            entry["cg_steps"], entry["rho"], entry["stop"] = steps, float(rho[-1]), stop
            if stop == "breakdown" and steps == 0 and rho[0] > 0.0:
                status = "singular"
                break
            entry["step"] = float(host[0])
            d, x = x, d
            done += 1
            arap.take()
            if entry["step"] <= tol * extent:
                status = "converged"
                break
        _warp_apply(verts, d, V, moved)
    return {"verts": moved, "displacement": d, "rotations": arap.result(), "history": history, "iterations": done, "status": status}


SHAPE_MAX_ROWS = 256          # MOFA_SHAPE_MAX_ROWS: meshes of a model, and modes + 1 of a fit
SHAPE_PIVOT_FLOOR = 2.0 ** -40   # a Cholesky pivot at or below this share of its diagonal entry has lost 40 bits to cancellation: singular
SHAPE_JACOBI_SWEEPS = 64      # the cap of the host's cyclic Jacobi (8 meshes take 5 sweeps, 256 random ones 11)


# ---- the host side of a shape model: plain IEEE fp64 (+ - * / sqrt), every operation in the order DESIGN 3.25 writes down -----------------
def _shape_jacobi(G):
    """(eigenvalues [n] descending, eigenvectors [n,n] in columns, sweeps) of the symmetric ``G`` by cyclic Jacobi.  A sweep visits the pairs
    (p, q), p < q, row by row: (0,1) (0,2) .. (0,n-1) (1,2) ..  With x = A_pq: a pair with x == 0 is skipped; one with
    ``|A_pp| + 100 |x| == |A_pp|`` and ``|A_qq| + 100 |x| == |A_qq|``, or with ``norm + |x| == norm`` (norm = the largest ``|G_ii|``: G's own
    entries carry a larger error, and without this rule the null space of a rank-deficient G is turned for many sweeps), gets A_pq = A_qp = 0
    and is skipped; otherwise
    ``theta = (A_qq - A_pp) / (2 x)``, ``t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta theta + 1))``, ``c = 1 / sqrt(t t + 1)``, ``s = t c``;
    columns p, q of A become ``c a_p - s a_q`` and ``s a_p + c a_q`` (both from the old columns), rows p, q the same vectors, ``A_pp = A_pp -
    t x``, ``A_qq = A_qq + t x``, ``A_pq = A_qp = 0``; columns p, q of W (the identity at first) turn the same way.  The loop stops after a
    sweep that rotated nothing, or after SHAPE_JACOBI_SWEEPS.  The diagonal is sorted descending, equal values by their index; every
    eigenvector's component of largest magnitude (the first among equal ones) is made positive."""
    A = np.array(G, dtype=np.float64)
    n = len(A)
    W = np.eye(n)
    norm = float(np.abs(np.diag(A)).max()) if n else 0.0
    sweeps = 0
    with np.errstate(all="ignore"):
        for _ in range(SHAPE_JACOBI_SWEEPS):
            rotated = 0
            for p in range(n - 1):
                for q in range(p + 1, n):
                    x = float(A[p, q])
                    if x == 0.0:
                        continue
                    g = 100.0 * abs(x)
                    if (abs(A[p, p]) + g == abs(A[p, p]) and abs(A[q, q]) + g == abs(A[q, q])) or norm + abs(x) == norm:
                        A[p, q] = A[q, p] = 0.0
                        continue
                    theta = (float(A[q, q]) - float(A[p, p])) / (2.0 * x)
                    t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                    c = 1.0 / math.sqrt(t * t + 1.0)
                    s = t * c
                    cp, cq = A[:, p].copy(), A[:, q].copy()
                    npp, nqq = cp[p] - t * x, cq[q] + t * x
                    new_p, new_q = c * cp - s * cq, s * cp + c * cq
                    A[:, p], A[:, q] = new_p, new_q
                    A[p, :], A[q, :] = new_p, new_q
                    A[p, p], A[q, q] = npp, nqq
                    A[p, q] = A[q, p] = 0.0
                    wp, wq = W[:, p].copy(), W[:, q].copy()
                    W[:, p], W[:, q] = c * wp - s * wq, s * wp + c * wq
                    rotated += 1
            sweeps += 1
            if rotated == 0:
                break
    lam = np.diag(A).copy()
    order = sorted(range(n), key=lambda i: (-lam[i], i))
    lam, W = lam[order], W[:, order]
    for k in range(n):
        if W[int(np.argmax(np.abs(W[:, k]))), k] < 0:
            W[:, k] = -W[:, k]
    return lam, W, sweeps


def _shape_solve(A, rhs, lam):
    """x of ``(A + lam I) x = rhs`` by :func:`_icp_solve`'s Cholesky (L's columns left to right, every sum over k ascending; a column's
    elements are updated together, elementwise); None when a pivot is not above SHAPE_PIVOT_FLOOR times its diagonal entry (two equal
    modes leave a pivot of rounding noise, of either sign) and finite, or the solution is not finite."""
    H = np.array(A, dtype=np.float64)
    n = len(rhs)
    for i in range(n):
        H[i, i] = H[i, i] + lam
    Lm = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            col = H[j:, j].copy()
            for k in range(j):
                col = col - Lm[j:, k] * Lm[j, k]
            s = float(col[0])
            if not (s > SHAPE_PIVOT_FLOOR * float(H[j, j]) and math.isfinite(s)):
                return None
            d = math.sqrt(s)
            Lm[j, j] = d
            Lm[j + 1:, j] = col[1:] / d
        r = np.array(rhs, dtype=np.float64)
        z = np.zeros(n)
        for i in range(n):
            z[i] = r[i] / Lm[i, i]
            r[i + 1:] = r[i + 1:] - Lm[i + 1:, i] * z[i]
        Lt, x = Lm.tolist(), [0.0] * n
        for i in range(n - 1, -1, -1):
            s = float(z[i])
            for k in range(i + 1, n):
                s = s - Lt[k][i] * x[k]
            x[i] = s / Lt[i][i]
    x = np.array(x, dtype=np.float64)
    return x if np.isfinite(x).all() else None


def _shape_matrix(sums, R):
    """The symmetric [R,R] matrix of the R (R + 1) / 2 sums of mofa_shape_gram (the upper triangle row by row)."""
    G = np.zeros((R, R))
    iu = np.triu_indices(R)
    G[iu] = sums
    G.T[iu] = sums
    return G


def _shape_step(sums, K, c, lam):
    """(the step of ``(A + lam I) dc = -(g + lam c)`` or None, the energy) from the sums of the modes and the residual row."""
    G = _shape_matrix(sums, K + 1)
    g = G[:K, K].copy()
    rhs = -g if lam == 0.0 else -(g + lam * np.asarray(c, dtype=np.float64))
    return _shape_solve(G[:K, :K], rhs, lam), float(G[K, K])


def _shape_inverse(state):
    """``[1 / s, R^T, -(1 / s) R^T t]`` (13 doubles) of the pose (s, q, t)."""
    s, q, t = state
    R = _quat_rotation(q)
    si = 1.0 / s
    return (C.c_double * 13)(si, R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8],
                             *[-(si * ((R[r] * t[0] + R[3 + r] * t[1]) + R[6 + r] * t[2])) for r in range(3)])


# ---- the device side ----------------------------------------------------------------------------------------------------------------------
def _shape_gram(P, R, N, weight=None, group=1):
    """The R (R + 1) / 2 sums of mofa_shape_gram over ``P [R, N]`` (float64, GPU), reduced level by level; on the host."""
    L, dev = lib.load(), P.device
    npairs, M = R * (R + 1) // 2, (N + ICP_CHUNK - 1) // ICP_CHUNK
    rows = torch.empty(M, npairs, dtype=torch.float64, device=dev)
    lib.check(L.mofa_shape_gram(P.data_ptr(), R, N, None if weight is None else weight.data_ptr(), group, rows.data_ptr(), lib.stream()),
              "mofa_shape_gram")
    while M > 1:
        n = (M + ICP_CHUNK - 1) // ICP_CHUNK
        out = torch.empty(n, npairs, dtype=torch.float64, device=dev)
        lib.check(L.mofa_shape_reduce(rows.data_ptr(), M, npairs, out.data_ptr(), lib.stream()), "mofa_shape_reduce")
        rows, M = out, n
    return rows.reshape(-1).cpu().numpy()


def _shape_combine(base, coef, rows, n):
    """``out [B, n]`` (float64, GPU) of mofa_shape_combine: ``coef [B, R]`` (host), ``rows [R, n]``, ``base [n]`` or None."""
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    B, R = coef.shape
    out = torch.empty(B, n, dtype=torch.float64, device=rows.device)
    c = torch.from_numpy(coef).to(rows.device)
    lib.check(lib.load().mofa_shape_combine(None if base is None else base.data_ptr(), c.data_ptr(), rows.data_ptr(), B, R, n, out.data_ptr(),
                                            lib.stream()), "mofa_shape_combine")
    return out


def _shape_model_arg(who, model, components=None):
    """(mean [V,3], modes [K',V,3], V, K', device) of a model dict, checked; K' = min(components, K)."""
    try:
        mean, modes = model["mean"], model["modes"]
    except (KeyError, TypeError):
        raise lib.MofaError(f"{who}: want a model dict of shape_model / read_shape_model (mean, modes)")
    for name, t in (("mean", mean), ("modes", modes)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise lib.MofaError(f"{who}: the HIP path needs the model on the GPU (got a CPU {name}); there is no CPU fallback")
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise lib.MofaError(f"{who}: want a contiguous float64 {name}, got {t.dtype} contiguous={t.is_contiguous()}")
    if mean.dim() != 2 or mean.shape[1] != 3 or modes.dim() != 3 or modes.shape[1:] != mean.shape or modes.device != mean.device:
        raise lib.MofaError(f"{who}: want mean [V,3] and modes [K,V,3] on one device, got {tuple(mean.shape)} and {tuple(modes.shape)}")
    K, V = int(modes.shape[0]), int(mean.shape[0])
    if K >= SHAPE_MAX_ROWS or V > INT32_MAX // 3:
        raise lib.MofaError(f"{who}: {K} modes (want < {SHAPE_MAX_ROWS}) / {V} vertices (want 3 V < 2^31)")
    if components is not None:
        if isinstance(components, (bool, np.bool_)) or not isinstance(components, (int, np.integer)) or int(components) < 0:
            raise lib.MofaError(f"{who}: components = {components!r} (want an integer >= 0, or None)")
        K = min(K, int(components))
    return mean, modes[:K], V, K, mean.device


def _shape_regularize(who, regularize) -> float:
    lam = float(regularize)
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise lib.MofaError(f"{who}: regularize = {regularize} (want finite and >= 0)")
    return lam


def _shape_coeffs(who, coeffs, K):
    """Coefficients from the caller as a host array [B, K'] with K' <= K."""
    try:
        c = np.asarray(_host(coeffs), dtype=np.float64)
        c = c.reshape(1, -1) if c.ndim == 1 else c
        if c.ndim != 2 or c.shape[1] > K or not np.isfinite(c).all():
            raise ValueError(f"shape {c.shape}")
    except (TypeError, ValueError) as e:
        raise lib.MofaError(f"{who}: want finite coefficients [B, K'] with K' <= {K}: {e}")
    return np.ascontiguousarray(c)


def _shape_synth(mean, modes, V, c):
    """``mean + sum_k c[b][k] modes[k]`` as [B, V, 3] float64 (mofa_shape_combine); no mode: the mean."""
    c = np.asarray(c, dtype=np.float64).reshape(len(c), -1)
    if c.shape[1] == 0 or V == 0:
        return mean.unsqueeze(0).repeat(len(c), 1, 1)
    return _shape_combine(mean, c, modes[:c.shape[1]], 3 * V).reshape(len(c), V, 3)


def shape_model(meshes: torch.Tensor, components=None, rank_tol: float = 1e-10, align: Optional[str] = None, align_iterations: int = 2,
                timing: bool = False) -> dict:
    """A linear shape model — a mean and modes of variation — of ``meshes [M,V,3] float32`` on the GPU, ``2 <= M <= 256`` meshes with one
    vertex numbering (outputs of :func:`warp`): principal components by the M x M Gram matrix, the covariance itself is never formed.

    1. ``mofa_shape_centre``: ``mean[j]`` = the sum over the meshes in their order divided by M, ``X[m] = meshes[m] - mean`` (float64),
    2. ``mofa_shape_gram``: ``G = X X^T`` in a fixed order (chunks of 1,024 columns, ``mofa_icp_reduce``'s sum; ``mofa_shape_reduce`` for
       the later levels),
    3. the host decomposes G by cyclic Jacobi written with ``+ - * / sqrt`` only (:func:`_shape_jacobi` states the order of the pairs, the
       rotation, the skip rule, the stopping rule, the order of the eigenvalues and the sign rule),
    4. K = ``components``, or the number of eigenvalues above ``rank_tol`` times the largest; at most M - 1, and only eigenvalues > 0,
    5. ``sigma_k = sqrt(lambda_k / (M - 1))``,
    6. ``modes[k] = (sigma_k / sqrt(lambda_k)) * sum_m U[m][k] X[m]`` (``mofa_shape_combine``, m ascending): a mode is in length units,
       a coefficient in standard deviations.

    ``align="rigid"`` / ``"similarity"`` first runs ``align_iterations`` rounds, each fitting every mesh onto the current mean (rounded to
    float32) by :func:`fit_transform` (all vertices, the point metric, from the round before) and taking the mean of the moved meshes;
    ``transforms [M,4,4]`` (NumPy) then holds what moved each mesh.  Returns a dict: ``mean [V,3]``, ``modes [K,V,3]`` (float64, GPU),
    ``sigma [K]``, ``eigenvalues [M]``, ``coeffs [M,K]`` (the training meshes' own coefficients, ``U[m][k] * (sqrt(lambda_k) / sigma_k)``),
    ``explained [K]`` (``lambda_k`` over the sum of all in their order) — NumPy float64 —, ``n_meshes`` and ``status``: ``"ok"``, or
    ``"sweeps"`` when the Jacobi ran into its cap.  The same input gives the same bytes.  ``timing=True`` adds ``times``: seconds of ``align``,
    ``gram`` (centre, Gram kernel, reduce levels and the read-back), ``jacobi`` (the host decomposition) and ``modes``, each ended by a device
    synchronisation.

    Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, M < 2, M > 256, V = 0, non-finite vertices and an unknown ``align``."""
    who = "shape_model"
    lib.ptr(meshes)
    if meshes.dim() != 3 or meshes.shape[2] != 3:
        raise lib.MofaError(f"{who}: want meshes [M,V,3], got {tuple(meshes.shape)}")
    M, V, dev = int(meshes.shape[0]), int(meshes.shape[1]), meshes.device
    if not 2 <= M <= SHAPE_MAX_ROWS:
        raise lib.MofaError(f"{who}: {M} meshes (want 2 .. {SHAPE_MAX_ROWS})")
    if not 1 <= V <= INT32_MAX // 3:
        raise lib.MofaError(f"{who}: {V} vertices (want 1 .. (2^31 - 1) / 3)")
    if align not in (None, "rigid", "similarity"):
        raise lib.MofaError(f"{who}: align = {align!r} (want None, 'rigid' or 'similarity')")
    if components is not None and (isinstance(components, (bool, np.bool_)) or not isinstance(components, (int, np.integer)) or int(components) < 0):
        raise lib.MofaError(f"{who}: components = {components!r} (want an integer >= 0, or None)")
    if isinstance(align_iterations, (bool, np.bool_)) or not isinstance(align_iterations, (int, np.integer)) or not 0 <= int(align_iterations) <= 100:
        raise lib.MofaError(f"{who}: align_iterations = {align_iterations!r} (want an integer 0 .. 100)")
    rank_tol = float(rank_tol)
    if not 0.0 <= rank_tol < 1.0:
        raise lib.MofaError(f"{who}: rank_tol = {rank_tol} (want in [0, 1))")
    n, L = 3 * V, lib.load()
    times = dict.fromkeys(("align", "gram", "jacobi", "modes"), 0.0)

    def lap(name, since):
        if timing:
            torch.cuda.synchronize(dev)
            times[name] += time.perf_counter() - since
        return time.perf_counter()

    with torch.cuda.device(dev):
        if not bool(torch.isfinite(meshes).all()):
            raise lib.MofaError(f"{who}: the meshes hold non-finite vertices")
        clock = time.perf_counter()
        mean = torch.empty(V, 3, dtype=torch.float64, device=dev)
        X = torch.empty(M, n, dtype=torch.float64, device=dev)

        def centre(ms):
            lib.check(L.mofa_shape_centre(lib.ptr(ms), M, n, mean.data_ptr(), X.data_ptr(), lib.stream()), "mofa_shape_centre")

        transforms = None
        if align is not None:
            src, fits = meshes, [None] * M
            for _ in range(int(align_iterations)):
                centre(meshes)
                mean32 = mean.to(torch.float32)
                fits = [fit_transform(src[m], mean32, model=align, metric="point", init=fits[m]) for m in range(M)]
                meshes = torch.stack([f["moved"] for f in fits]).contiguous()
            transforms = np.stack([f["matrix"] if f is not None else np.eye(4) for f in fits])
        clock = lap("align", clock)
        centre(meshes)
        G = _shape_matrix(_shape_gram(X, M, n), M)
        clock = lap("gram", clock)
        lam, U, sweeps = _shape_jacobi(G)
        clock = lap("jacobi", clock)
        K = int(components) if components is not None else int((lam > rank_tol * float(lam.max())).sum())
        K = min(K, M - 1)
        pos = 0
        while pos < K and lam[pos] > 0:
            pos += 1
        K = pos
        sigma = np.array([math.sqrt(lam[k] / float(M - 1)) for k in range(K)])
        root = np.array([math.sqrt(lam[k]) for k in range(K)])
        if K:
            modes = torch.from_numpy(sigma / root).to(dev)[:, None] * _shape_combine(None, U[:, :K].T.copy(), X, n)
        else:
            modes = torch.zeros(0, n, dtype=torch.float64, device=dev)
        clock = lap("modes", clock)
    total = 0.0
    for v in lam:
        total = total + float(v)
    out = {"mean": mean, "modes": modes.reshape(K, V, 3).contiguous(), "sigma": sigma, "eigenvalues": lam, "coeffs": U[:, :K] * (root / sigma)[None, :],
           "explained": lam[:K] / total if K else np.zeros(0), "n_meshes": M, "status": "ok" if sweeps < SHAPE_JACOBI_SWEEPS else "sweeps"}
    if transforms is not None:
        out["transforms"] = transforms
    if timing:
        out["times"] = times
    return out


def shape_synthesize(model: dict, coeffs, dtype=torch.float64) -> torch.Tensor:
    """The meshes ``mean + sum_k coeffs[b][k] modes[k]`` of a model of :func:`shape_model`: ``coeffs [B, K']`` (a host array or a tensor;
    ``K' <= K``: the leading modes) gives ``[B,V,3]`` on the model's device (``mofa_shape_combine``: the sum over k ascending from 0.0,
    then added to the mean, in float64).  ``dtype=torch.float32`` rounds that result once at the end.  Raises ``MofaError`` for a model
    that is not on the GPU, coefficients that are not finite or too many, and another dtype."""
    who = "shape_synthesize"
    mean, modes, V, K, dev = _shape_model_arg(who, model)
    if dtype not in (torch.float64, torch.float32):
        raise lib.MofaError(f"{who}: dtype = {dtype} (want torch.float64 or torch.float32)")
    c = _shape_coeffs(who, coeffs, K)
    if len(c) == 0:
        return torch.empty(0, V, 3, dtype=dtype, device=dev)
    if len(c) > 65535:
        raise lib.MofaError(f"{who}: {len(c)} meshes in one call (want <= 65,535)")
    with torch.cuda.device(dev):
        return _shape_synth(mean, modes, V, c).to(dtype)


def shape_project(model: dict, verts: torch.Tensor, weight: Optional[torch.Tensor] = None, regularize: float = 0.0, components=None) -> dict:
    """The coefficients of a mesh with the model's vertex numbering (``verts [V,3] float32``: an output of :func:`warp`, or landmarks with
    ``weight [V] float64`` 0 elsewhere): the minimum of ``sum_i w_i |mean_i + sum_k c_k m_ki - v_i|^2 + regularize |c|^2``.  The residual
    ``mean - v`` joins the modes as one more row; one pass of ``mofa_shape_gram`` (group 3: a weight per vertex) yields A, g and the
    energy, and the host solves ``(A + regularize I) c = -g`` by Cholesky.  A vertex that is not finite gets weight 0.  ``components``:
    the leading modes only.  Returns ``coeffs [K]`` (NumPy float64), ``verts [V,3]`` (float64, GPU: the reconstruction), ``rms`` (weighted,
    of the reconstruction against ``verts``) and ``status``: ``"ok"``, ``"singular"`` (a pivot of the Cholesky factor is not positive: the
    weighted vertices do not fix the modes; coefficients 0) or ``"empty"`` (no vertex with a weight > 0)."""
    who = "shape_project"
    mean, modes, V, K, dev = _shape_model_arg(who, model, components)
    if _query_points(who, verts, dev) != V:
        raise lib.MofaError(f"{who}: the model has {V} vertices, verts {verts.shape[0]}")
    lam = _shape_regularize(who, regularize)
    weight = _icp_weight(who, weight, V, dev)
    c = np.zeros(K)
    with torch.cuda.device(dev):
        w = torch.where(torch.isfinite(verts).all(1), weight, torch.zeros_like(weight)) if V else weight
        if V == 0 or int((w > 0).sum()) == 0:
            return {"coeffs": c, "verts": _shape_synth(mean, modes, V, c[None])[0], "rms": float("nan"), "status": "empty"}
        n = 3 * V
        P = torch.empty(K + 1, n, dtype=torch.float64, device=dev)
        P[:K] = modes.reshape(K, n)
        P[K] = (mean - verts.double()).reshape(n)
        wsum = float(_icp_reduce(w.reshape(V, 1), V, 1).cpu()[0])
        x, _ = _shape_step(_shape_gram(P, K + 1, n, w, 3), K, c, lam)
        status = "ok"
        if x is None:
            x, status = c, "singular"
        recon = _shape_synth(mean, modes, V, x[None])[0]
        e = _shape_gram((recon - verts.double()).reshape(1, n).contiguous(), 1, n, w, 3)[0]
        with np.errstate(all="ignore"):
            rms = float(np.sqrt(e / np.float64(wsum)))
    return {"coeffs": x, "verts": recon, "rms": rms, "status": status}


def shape_fit(model: dict, target_verts: torch.Tensor, target_faces: torch.Tensor, metric: str = "plane", pose: Optional[str] = None,
              iterations: int = 20, regularize: float = 0.0, init=None, init_coeffs=None, weight: Optional[torch.Tensor] = None,
              max_distance=None, reject_border: bool = True, tol: float = 0.0, components=None, grid=None, timing: bool = False) -> dict:
    """Fits a model of :func:`shape_model` to the mesh ``(target_verts [T,3] float32, target_faces [F,3] int32)`` with a triangulation of
    its own, by iterated closest points: the unknowns are the coefficients ``c`` and, with ``pose`` (one of :func:`register`'s models), a
    pose ``x -> s R x + t`` — K + 7 numbers, between :func:`register` (7) and :func:`warp` (3 V).  The fit cannot leave the span of the
    examples, which is what keeps it steady on partial or noisy targets; its ``verts`` are :func:`warp`'s natural ``init``.  The target is
    binned once (``grid`` as in :func:`closest_points`: it changes no bit).  An iteration is

    * with ``pose``, the pose phase: synthesise the model (``mofa_shape_combine``), round it to float32 and move it
      (``mofa_icp_apply``), find the closest points, reject exactly as :func:`register` does (not finite, no face / beyond
      ``max_distance``, on the target's border with ``reject_border``) and take one step of :func:`register` on (s, R, t) — its sums, its
      solve, its pivot (the centre of the target's box) and extent;
    * the shape phase: synthesise, move, query and reject again, then one Gauss–Newton step ``(A + regularize I) dc = -(g + regularize c)``
      from one pass of ``mofa_shape_gram`` over K + 1 rows.  ``metric="plane"``: ``mofa_shape_plane_rows`` gives ``s (R^T n) . m_ki`` per mode
      and the residual ``n . (moved - closest)`` along the closest face's normal n (group 1).  ``"point"``: the closest points are taken
      back into the model's frame by ``mofa_icp_apply`` with the inverse pose (composed on the host: ``1 / s``, ``R^T``, ``-(1 / s) R^T t``),
      the rows are the modes and the residual ``y - c'`` (group 3).  A column whose residual is not finite gets weight 0.

    ``plane`` is the default because a model vertex may slide along the target's surface at no cost: where the target is the model's
    own surface the first step lands on it (the test scene: 5e-9 after one iteration), while ``point`` pulls every vertex to a closest
    point that is the wrong partner until the shapes agree, and contracts by a constant factor (there 0.6 per iteration).  ``weight [V]
    float64`` (>= 0), ``init`` (a pose as :func:`register` takes it), ``init_coeffs [K]``, ``components`` (the leading modes only).  The
    fit has converged when the pose step and ``max |dc|`` are both ``<= tol``.

    Returns a dict: ``coeffs [K]``, ``scale``, ``rotation [3,3]``, ``translation [3]``, ``matrix [4,4]`` (NumPy float64), ``verts [V,3]
    float32`` (in the target's frame), ``model_verts [V,3]`` float64 (in the model's), ``history`` (per iteration ``{"pose": entry or None,
    "shape": entry}``, an entry holding ``used``, ``rejected`` by cause, ``rms`` and ``step``), ``iterations``, ``grid`` and ``status``:
    ``"converged"``, ``"iterations"``, ``"singular"`` (a Cholesky pivot of either step is not positive; the last state is kept),
    ``"no_correspondences"`` (also a target without faces) or ``"empty"`` (a model without vertices).  ``timing=True`` adds ``times``:
    seconds of ``bin`` and, summed over the iterations, ``query`` (synthesis, move, closest points), ``rows`` (rejection, pose sums, rows),
    ``gram`` and ``host``, each ended by a device synchronisation.  No robust kernel and no coarse-to-fine: a local method.

    Raises ``MofaError`` for CPU tensors, wrong dtypes or shapes, a face index outside the target, a non-finite target vertex, negative
    weights, ``max_distance`` not > 0, ``regularize`` < 0, an unknown metric or pose model and a grid out of range."""
    who = "shape_fit"
    mean, modes, V, K, dev = _shape_model_arg(who, model, components)
    TV, F, tdev = _mesh_tensors(who, target_verts, target_faces)
    if tdev != dev:
        raise lib.MofaError(f"{who}: the model on {dev}, the target on {tdev}")
    iterations, tol = _icp_args(who, pose if pose is not None else "rigid", metric, iterations, tol)
    lam = _shape_regularize(who, regularize)
    maxd = _max_distance(who, max_distance)
    grid = _dist_grid_arg(who, grid)
    weight = _icp_weight(who, weight, V, dev)
    state = _icp_init(who, init)
    c = np.zeros(K) if init_coeffs is None else _shape_coeffs(who, init_coeffs, SHAPE_MAX_ROWS)[0][:K].copy()
    if len(c) != K:
        raise lib.MofaError(f"{who}: init_coeffs holds {len(c)} coefficients, the fit has {K} modes")
    times = dict.fromkeys(("bin", "query", "rows", "gram", "host"), 0.0)
    L = lib.load()

    def lap(name, since):
        if timing:
            torch.cuda.synchronize(dev)
            times[name] += time.perf_counter() - since
        return time.perf_counter()

    def finish(history, done, status, grid_used):
        with torch.cuda.device(dev):
            y = _shape_synth(mean, modes, V, c[None])[0]
            moved = _icp_apply(y.to(torch.float32), V, state) if V else torch.empty(0, 3, dtype=torch.float32, device=dev)
        out = _icp_result(state, moved, history, done, status)
        out["verts"] = out.pop("moved")
        out["coeffs"], out["model_verts"], out["grid"] = c, y, grid_used
        if timing:
            out["times"] = times
        return out

    if V == 0:
        return finish([], 0, "empty", grid)
    if TV == 0 or F == 0:
        return finish([], 0, "no_correspondences", grid)
    history, status, done = [], "iterations", 0
    n = 3 * V
    with torch.cuda.device(dev):
        clock = time.perf_counter()
        b = _dist_lists(who, target_verts, target_faces, TV, F, grid)
        mu, extent = _icp_extent(b["box"])
        if reject_border:
            face_border, vert_border = _border_flags(who, target_faces, TV, F)
            border = torch.empty(V, dtype=torch.uint8, device=dev)
        zero = torch.zeros_like(weight)
        moved = torch.empty(V, 3, dtype=torch.float32, device=dev)
        P = torch.empty(K + 1, n if metric == "point" else V, dtype=torch.float64, device=dev)
        if metric == "point":
            P[:K] = modes.reshape(K, n)
        clock = lap("bin", clock)

        def correspond():
            y = _shape_synth(mean, modes, V, c[None])[0]
            _icp_apply(y.to(torch.float32), V, state, moved)
            res = _dist_query(moved, V, target_verts, target_faces, TV, F, b, maxd)
            nonlocal clock
            clock = lap("query", clock)
            finite = torch.isfinite(moved).all(1) & (torch.isfinite(res["d2"]) | (res["face"] < 0))
            has = finite & (res["face"] >= 0)
            if reject_border:
                lib.check(L.mofa_icp_reject(res["face"].data_ptr(), lib.ptr(res["bary"]), V, target_faces.data_ptr(), F, TV, face_border.data_ptr(),
                                            vert_border.data_ptr(), border.data_ptr(), lib.stream()), "mofa_icp_reject")
                on_border = has & (border != 0)
            else:
                on_border = torch.zeros_like(has)
            keep = has & ~on_border & (weight > 0)
            n_used, n_bad, n_none, n_border = (int(v) for v in torch.stack([keep.sum(), (~finite).sum(), (finite & ~has).sum(), on_border.sum()]).cpu())
            entry = {"used": n_used, "rejected": {"non_finite": n_bad, "beyond" if max_distance is not None else "no_face": n_none,
                                                  "border": n_border}}
            return y, res, keep, entry

        for _ in range(iterations):
            record = {"pose": None, "shape": None}
            history.append(record)
            pose_step = 0.0
            if pose is not None:
                y, res, keep, entry = correspond()
                record["pose"] = entry
                w = torch.where(keep, weight, zero)
                sums = _icp_sums(moved, res["closest"], None, res["face"], target_verts, TV, target_faces, F, w, V, mu, metric)
                clock = lap("rows", clock)
                new, stop = _icp_update(state, sums, _ICP_MODEL[pose], mu, extent, entry)
                clock = lap("host", clock)
                if stop:
                    status = stop
                    break
                state, pose_step = new, entry["step"]
            y, res, keep, entry = correspond()
            record["shape"] = entry
            entry["rms"], entry["step"] = float("nan"), float("nan")
            if metric == "plane":
                T = (C.c_double * 13)(state[0], *_quat_rotation(state[1]), *state[2])
                lib.check(L.mofa_shape_plane_rows(lib.ptr(moved), lib.ptr(res["closest"]), res["face"].data_ptr(), lib.ptr(target_verts), TV,
                                                  target_faces.data_ptr(), F, T, modes.data_ptr() if K else None, K, V, P.data_ptr(), lib.stream()),
                          "mofa_shape_plane_rows")
                keep = keep & torch.isfinite(P[K])
                group, width = 1, V
            else:
                back = torch.empty_like(moved)
                lib.check(L.mofa_icp_apply(lib.ptr(res["closest"]), V, _shape_inverse(state), lib.ptr(back), lib.stream()), "mofa_icp_apply")
                P[K] = (y - back.double()).reshape(n)
                keep = keep & torch.isfinite(P[K].reshape(V, 3)).all(1)
                group, width = 3, n
            w = torch.where(keep, weight, zero)
            entry["used"] = int(keep.sum())
            wsum = float(_icp_reduce(w.reshape(V, 1), V, 1).cpu()[0])
            clock = lap("rows", clock)
            sums = _shape_gram(P, K + 1, width, w, group)
            clock = lap("gram", clock)
            with np.errstate(all="ignore"):
                entry["rms"] = float(np.sqrt(sums[-1] / np.float64(wsum))) if wsum > 0 else float("nan")
            if entry["used"] == 0:
                status = "no_correspondences"
                break
            dc, _ = _shape_step(sums, K, c, lam)
            clock = lap("host", clock)
            if dc is None:
                status = "singular"
                break
            c = c + dc
            entry["step"] = float(np.abs(dc).max()) if K else 0.0
            done += 1
            if pose_step <= tol and entry["step"] <= tol:
                status = "converged"
                break
    return finish(history, done, status, b["grid"])


def write_shape_model(path: str, model: dict, faces=None) -> None:
    """Writes a model of :func:`shape_model` (and, with ``faces [F,3]``, the triangles its vertices share) as one ``.npz`` of plain arrays:
    ``mean``, ``modes``, ``sigma``, ``eigenvalues``, ``coeffs``, ``explained`` (float64), ``n_meshes``, ``transforms`` if the model has them,
    ``faces`` (int32).  Nothing is pickled."""
    arrays = {k: np.asarray(_host(model[k]), dtype=np.float64) for k in ("mean", "modes", "sigma", "eigenvalues", "coeffs", "explained")}
    arrays["n_meshes"] = np.asarray(int(model["n_meshes"]), dtype=np.int64)
    if "transforms" in model:
        arrays["transforms"] = np.asarray(model["transforms"], dtype=np.float64)
    if faces is not None:
        arrays["faces"] = np.asarray(_host(faces), dtype=np.int32).reshape(-1, 3)
    with open(path, "wb") as fh:
        np.savez(fh, **arrays)


def read_shape_model(path: str, device="cuda") -> dict:
    """The model :func:`write_shape_model` wrote (``allow_pickle=False``): ``mean`` and ``modes`` as float64 tensors on ``device``, the rest
    NumPy; ``faces`` (an int32 tensor on ``device``) when the file holds them.  ``status`` is ``"ok"``.  Raises ``MofaError`` for a file that
    is not such a model."""
    who = "read_shape_model"
    try:
        with np.load(path, allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        out = {k: np.asarray(arrays[k], dtype=np.float64) for k in ("sigma", "eigenvalues", "coeffs", "explained")}
        mean, modes = np.asarray(arrays["mean"], dtype=np.float64), np.asarray(arrays["modes"], dtype=np.float64)
        out["n_meshes"] = int(arrays["n_meshes"])
    except (KeyError, ValueError, OSError) as e:
        raise lib.MofaError(f"{who}: {path} is no shape model: {e}")
    if mean.ndim != 2 or mean.shape[1] != 3 or modes.ndim != 3 or modes.shape[1:] != mean.shape or len(out["sigma"]) != len(modes):
        raise lib.MofaError(f"{who}: {path}: mean {mean.shape}, modes {modes.shape}, sigma {out['sigma'].shape} do not belong together")
    out["mean"], out["modes"] = torch.from_numpy(mean).to(device).contiguous(), torch.from_numpy(modes).to(device).contiguous()
    if "transforms" in arrays:
        out["transforms"] = np.asarray(arrays["transforms"], dtype=np.float64)
    if "faces" in arrays:
        out["faces"] = torch.from_numpy(np.asarray(arrays["faces"], dtype=np.int32)).to(device).contiguous()
    out["status"] = "ok"
    return out


# faces whose clipped box of samples holds at least this many pixels are walked one wavefront per face (mofa_raster_faces); the choice
# changes no bit of the frame.  profiles/mesh_raster.md holds the sweep it comes from.
WAVE_MIN_PIXELS = 64


def _pose_tensor(c2w, dev) -> torch.Tensor:
    pose = torch.as_tensor(np.asarray(c2w.detach().cpu() if torch.is_tensor(c2w) else c2w), dtype=torch.float32)[:3, :4]
    return pose.contiguous().to(dev)


def rasterize(verts: torch.Tensor, faces: torch.Tensor, H: int, W: int, K, c2w, attrs: Optional[torch.Tensor] = None, znear: float = 1e-3,
              bary: bool = False, normals: bool = False, wave_min_pixels: Optional[int] = None) -> dict:
    """Rasterise a triangle mesh (``verts [V,3] float32``, ``faces [F,3] int32``, on the GPU) from the pinhole camera ``K`` / ``c2w`` of
    ``get_rays`` (``mofa_raster_project`` / ``_faces`` / ``_resolve``): pixel (i, j) is sampled at the integer point, and ``depth`` is the
    ray parameter of that pixel's ray — the depth ``Renderer.render_geometry`` gives without NDC.  Returns a dict of GPU tensors:
    ``depth [H,W]`` (0 where nothing is hit), ``face [H,W] int32`` (-1), ``mask [H,W] bool`` (``face >= 0``), ``counts [4] int64`` (faces
    drawn, culled — a vertex nearer than ``znear``, outside the 2^20-pixel guard band or non-finite, or an index out of range; there is
    no near-plane clipping —, degenerate after the snap to 1/256 pixel, and drawn faces that took the wavefront path; read it only if
    wanted: nothing here synchronises) and, on request, ``bary [H,W,3]`` (perspective-correct), ``attr [H,W,C]`` (``attrs [V,C]``, C in
    1 .. 16, interpolated) and ``normal [H,W,3]`` (the face's unit normal, turned to the camera).  Both windings are drawn; the nearest
    face wins and the lower index among equal depths, so the same input gives the same bits every time."""
    H, W = int(H), int(W)
    lib.ptr(verts)
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise lib.MofaError(f"rasterize: want verts [V,3], got {tuple(verts.shape)}")
    if not faces.is_cuda:
        raise lib.MofaError("the HIP path needs tensors on the GPU (got CPU faces); there is no CPU fallback")
    if faces.dtype != torch.int32 or not faces.is_contiguous() or faces.dim() != 2 or faces.shape[1] != 3:
        raise lib.MofaError(f"rasterize: want contiguous int32 faces [F,3], got {faces.dtype} {tuple(faces.shape)}")
    dev = verts.device
    if faces.device != dev:
        raise lib.MofaError(f"rasterize: verts on {dev}, faces on {faces.device}")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    C_attr = 0
    if attrs is not None:
        lib.ptr(attrs)
        if attrs.dim() != 2 or attrs.shape[0] != V or attrs.device != dev:
            raise lib.MofaError(f"rasterize: want attrs [{V},C] on {dev}, got {tuple(attrs.shape)} on {attrs.device}")
        C_attr = int(attrs.shape[1])
        if not 1 <= C_attr <= 16:
            raise lib.MofaError(f"rasterize: C = {C_attr} attributes per vertex (want 1 .. 16)")
    znear = float(znear)
    if not (np.isfinite(znear) and znear > 0):
        raise lib.MofaError(f"rasterize: znear = {znear} (want finite and > 0)")
    wmp = WAVE_MIN_PIXELS if wave_min_pixels is None else int(wave_min_pixels)
    if not 0 <= wmp <= INT32_MAX:
        raise lib.MofaError(f"rasterize: wave_min_pixels = {wave_min_pixels} (want 0 .. 2^31 - 1)")
    L = lib.load()
    nbytes = L.mofa_raster_workspace_bytes(V, F, H, W) if (abs(H) <= INT32_MAX and abs(W) <= INT32_MAX) else 0
    if nbytes == 0:
        raise lib.MofaError(f"rasterize: H = {H}, W = {W} with {V} vertices and {F} faces is refused (H, W >= 1, H W < 2^31)")
    fx, fy, cx, cy = float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])
    with torch.cuda.device(dev):
        pose = _pose_tensor(c2w, dev)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = {"depth": torch.empty(H, W, dtype=torch.float32, device=dev), "face": torch.empty(H, W, dtype=torch.int32, device=dev),
               "counts": torch.empty(4, dtype=torch.int64, device=dev)}
        if bary:
            out["bary"] = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
        if attrs is not None:
            out["attr"] = torch.empty(H, W, C_attr, dtype=torch.float32, device=dev)
        if normals:
            out["normal"] = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
        stream = lib.stream()
        lib.check(L.mofa_raster_project(verts.data_ptr(), V, F, H, W, fx, fy, cx, cy, lib.ptr(pose), znear, ws.data_ptr(), stream),
                  "mofa_raster_project")
        lib.check(L.mofa_raster_faces(faces.data_ptr(), F, V, H, W, wmp, ws.data_ptr(), out["counts"].data_ptr(), stream), "mofa_raster_faces")
        lib.check(L.mofa_raster_resolve(verts.data_ptr(), V, faces.data_ptr(), F, lib.ptr(attrs), max(C_attr, 1), H, W, fx, fy, cx, cy, lib.ptr(pose),
                                        ws.data_ptr(), lib.ptr(out["depth"]), out["face"].data_ptr(), lib.ptr(out.get("bary")),
                                        lib.ptr(out.get("attr")), lib.ptr(out.get("normal")), stream), "mofa_raster_resolve")
    out["mask"] = out["face"] >= 0
    return out


def depth_agreement(depth_mesh: torch.Tensor, mask_mesh: torch.Tensor, depth_vol: torch.Tensor, acc: torch.Tensor, acc_min: float) -> dict:
    """How well a rasterised mesh lies where the volume renders its surface, from one camera: ``depth_mesh`` / ``mask_mesh`` of
    :func:`rasterize`, ``depth_vol`` / ``acc`` of ``Renderer.render_geometry`` (non-NDC; the median depth is the one to compare a surface
    with).  The volume's mask is ``acc >= acc_min``.  Returns ``iou`` (of the two masks; 1.0 when both are empty), ``n_mesh``, ``n_vol``,
    ``n_both`` (pixel counts of each mask and of their overlap) and ``median_abs`` / ``p95_abs`` of ``|depth_mesh - depth_vol|`` on the
    overlap (NaN when it is empty).  Plain torch; reads the results back."""
    m = mask_mesh.to(torch.bool)
    v = acc >= float(acc_min)
    both = m & v
    n_mesh, n_vol, n_both = int(m.sum()), int(v.sum()), int(both.sum())
    union = n_mesh + n_vol - n_both
    out = {"iou": n_both / union if union else 1.0, "n_mesh": n_mesh, "n_vol": n_vol, "n_both": n_both,
           "median_abs": float("nan"), "p95_abs": float("nan")}
    if n_both:
        d = (depth_mesh[both].to(torch.float64) - depth_vol[both].to(torch.float64)).abs().sort().values

        def quantile(q):                                  # linear between the two nearest ranks (numpy's default), on any number of pixels
            pos = q * (n_both - 1)
            lo = int(pos)
            hi = min(lo + 1, n_both - 1)
            return float(d[lo] + (d[hi] - d[lo]) * (pos - lo))

        out["median_abs"], out["p95_abs"] = quantile(0.5), quantile(0.95)
    return out


def to8b(x) -> np.ndarray:
    """The reference's quantisation (tools/run_nerf_helpers.py:12): ``(255 * clip(x, 0, 1))`` truncated to uint8."""
    return (255 * np.clip(np.asarray(x, dtype=np.float32), 0, 1)).astype(np.uint8)


def _host(t) -> np.ndarray:
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def write_ply(path: str, verts, faces, colors=None, normals=None) -> None:
    """Binary little-endian PLY: ``float x, y, z`` (+ ``float nx, ny, nz`` from ``normals``, + ``uchar red, green, blue`` from ``colors``
    in [0,1] through ``to8b``) per vertex, ``list uchar int vertex_indices`` per face."""
    v = np.ascontiguousarray(_host(verts), dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(_host(faces), dtype=np.int32).reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    vrec = np.empty(len(v), dtype=fields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        nrm = np.ascontiguousarray(_host(normals), dtype=np.float32).reshape(-1, 3)
        if len(nrm) != len(v):
            raise ValueError(f"{len(nrm)} normals for {len(v)} vertices")
        vrec["nx"], vrec["ny"], vrec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        c = to8b(_host(colors)).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"{len(c)} colours for {len(v)} vertices")
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    frec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    frec["n"], frec["i"] = 3, f
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\n{props}"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path: str):
    """Read what :func:`write_ply` writes: ``(verts [V,3] float32, faces [F,3] int32, colors [V,3] uint8 or None)``, and a fourth
    element ``normals [V,3] float32`` when the file holds ``nx, ny, nz``."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    if lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    n_v = n_f = 0
    vprops = []
    element = None
    for ln in lines[2:]:
        w = ln.split()
        if w[0] == "element":
            element = w[1]
            if element == "vertex":
                n_v = int(w[2])
            elif element == "face":
                n_f = int(w[2])
        elif w[0] == "property" and element == "vertex":
            vprops.append(w[2])
    types = {"x": "<f4", "y": "<f4", "z": "<f4", "nx": "<f4", "ny": "<f4", "nz": "<f4", "red": "u1", "green": "u1", "blue": "u1"}
    vdt = np.dtype([(p, types[p]) for p in vprops])
    vrec = np.frombuffer(data, dtype=vdt, count=n_v, offset=end)
    frec = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=n_f, offset=end + n_v * vdt.itemsize)
    if n_f and not (frec["n"] == 3).all():
        raise ValueError(f"{path}: faces that are not triangles")
    verts = np.stack([vrec["x"], vrec["y"], vrec["z"]], -1).astype(np.float32).reshape(-1, 3)
    colors = np.stack([vrec["red"], vrec["green"], vrec["blue"]], -1).reshape(-1, 3) if "red" in vprops else None
    faces = np.ascontiguousarray(frec["i"]).astype(np.int32).reshape(-1, 3)
    if "nx" not in vprops:
        return verts, faces, colors
    return verts, faces, colors, np.stack([vrec["nx"], vrec["ny"], vrec["nz"]], -1).astype(np.float32).reshape(-1, 3)


__all__: Sequence[str] = ("grid_spec", "grid_points", "iso_surface", "band_surface", "refine_vertices", "density_normals", "vertex_normals", "components", "select_components", "keep_components", "simplify", "closest_points", "sample_faces", "surface_distance", "dist_grid", "default_dist_grid", "winding_number", "signed_distance",
                           "inside_grid", "wind_grid", "default_wind_grid", "vertex_adjacency", "smooth", "rasterize", "depth_agreement", "to8b", "write_ply",
                           "read_ply", "uv_locate", "texel_centres", "texel_map", "texel_surface", "texture_state", "texture_image", "dilate_texture",
                           "sample_texture", "face_atlas", "default_uv_grid", "write_obj", "read_obj")

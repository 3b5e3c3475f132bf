"""NumPy restatement of the narrow-band extraction (include/mofanerf_hip.h, mofa_band_*): the active-brick fixed point of seeding plus
growth, and the band mesh in the GPU's exact output order, built brick by brick from tests/mt_reference.py's marching tetrahedra on each
brick's (B+1)^3 sub-grid and stitched by global edge_id.  Test code, not product."""
import itertools

import numpy as np

import mt_reference as mt


def bricks_per_axis(res, B):
    assert all((n - 1) % B == 0 and n > B for n in res), (res, B)
    return tuple((n - 1) // B for n in res)


def seeded_bricks(grid, level, B):
    """[bx,by,bz] bool: the brick's 8 corner samples are not all on one side of the level."""
    inside = np.asarray(grid, dtype=np.float32) >= np.float32(level)
    c = inside[::B, ::B, ::B]
    corners = [c[dx:c.shape[0] - 1 + dx, dy:c.shape[1] - 1 + dy, dz:c.shape[2] - 1 + dz] for dx, dy, dz in itertools.product((0, 1), repeat=3)]
    s = np.sum(corners, axis=0)
    return (s > 0) & (s < 8)


def mixed_cells(grid, level):
    """[nx-1,ny-1,nz-1] bool: the cell's 8 corners are not all on one side (the cell holds a triangle)."""
    inside = np.asarray(grid, dtype=np.float32) >= np.float32(level)
    nx, ny, nz = inside.shape
    s = sum(inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) for dx, dy, dz in itertools.product((0, 1), repeat=3))
    return (s > 0) & (s < 8)


def active_fixed_point(grid, level, B):
    """(active [bx,by,bz] bool, seeded [bx,by,bz] bool, rounds): seeding, then growth from the bricks added last — an outer-layer cell
    with a triangle activates every neighbour brick it touches across a face, an edge or a corner — until nothing is added."""
    nb = bricks_per_axis(grid.shape, B)
    seeded = seeded_bricks(grid, level, B)
    m = mixed_cells(grid, level).reshape(nb[0], B, nb[1], B, nb[2], B)
    # touches[o]: the brick has a mixed cell in the layer facing offset o (o_a = -1: local 0, +1: local B-1, 0: any)
    touches = {}
    for o in itertools.product((-1, 0, 1), repeat=3):
        if o == (0, 0, 0):
            continue
        sel = m
        for a, oa in enumerate(o):
            idx = [slice(None)] * 6
            idx[2 * a + 1] = slice(0, 1) if oa < 0 else (slice(B - 1, B) if oa > 0 else slice(None))
            sel = sel[tuple(idx)]
        touches[o] = sel.any(axis=(1, 3, 5))
    active, new, rounds = seeded.copy(), seeded.copy(), 0
    while new.any():
        grow = np.zeros_like(active)
        for o, t in touches.items():
            src = new & t
            dst = [slice(max(oa, 0), n + min(oa, 0)) for oa, n in zip(o, nb)]
            srcs = [slice(max(-oa, 0), n - max(oa, 0)) for oa, n in zip(o, nb)]
            grow[tuple(dst)] |= src[tuple(srcs)]
        new = grow & ~active
        active |= new
        rounds += bool(new.any())
    return active, seeded, rounds


def band_mesh(grid, level, lo, step, B, active):
    """(verts [V,3] float32, faces [F,3] int32, edge_ids [V] int64) of the active bricks, in the GPU's order: vertices by brick
    (ascending index), then edge_id; faces by brick, cell, tet, triangle.  Each brick's triangles come from marching tetrahedra on its own
    (B+1)^3 sub-grid; its local vertices are renamed by global edge_id, and a vertex is stored by the brick that owns its lower end."""
    g = np.asarray(grid, dtype=np.float32)
    nx, ny, nz = g.shape
    nb = bricks_per_axis(g.shape, B)
    dense_verts, _ = mt.marching_tets(g, level, lo, step)
    dense_ids = dense_edge_ids(g, level)
    e = B + 1
    owned_ids, faces_global = [], []
    for b in np.flatnonzero(active.reshape(-1)):
        bi, bj, bk = np.unravel_index(b, nb)
        o = np.array([bi, bj, bk]) * B
        sub = g[o[0]:o[0] + e, o[1]:o[1] + e, o[2]:o[2] + e]
        _, f = mt.marching_tets(sub, level, lo, step)
        lid = dense_edge_ids(sub, level)                                      # local edge ids, in local vertex order
        lidx, d = lid // 7, lid % 7
        li, lj, lk = lidx // (e * e), (lidx // e) % e, lidx % e
        gid = 7 * (((o[0] + li) * ny + o[1] + lj) * nz + o[2] + lk) + d
        faces_global.append(gid[f] if len(f) else np.zeros((0, 3), np.int64))
        hi = [B if bb == n - 1 else B - 1 for bb, n in zip((bi, bj, bk), nb)]
        own = (li <= hi[0]) & (lj <= hi[1]) & (lk <= hi[2])
        owned_ids.append(gid[own])
    ids = np.concatenate(owned_ids) if owned_ids else np.zeros(0, np.int64)
    fg = np.concatenate(faces_global) if faces_global else np.zeros((0, 3), np.int64)
    pos = np.searchsorted(dense_ids, ids)                                    # the dense vertex of every band vertex (positions)
    assert np.array_equal(dense_ids[pos], ids)
    order = np.argsort(ids, kind="stable")
    at = np.minimum(np.searchsorted(ids[order], fg), max(len(ids) - 1, 0))
    assert len(fg) == 0 or np.array_equal(ids[order][at], fg), "a face uses an edge no active brick owns"
    faces = order[at] if len(fg) else np.zeros((0, 3), np.int64)
    return dense_verts[pos].reshape(-1, 3), faces.astype(np.int32).reshape(-1, 3), ids.astype(np.int64)


def dense_edge_ids(grid, level):
    """edge_id of every vertex of mt.marching_tets(grid, level, ...), in its vertex order (increasing)."""
    g = np.asarray(grid, dtype=np.float32)
    inside = g >= np.float32(level)
    nx, ny, nz = g.shape
    flags = np.zeros((nx, ny, nz, 7), dtype=bool)
    for d, (dx, dy, dz) in enumerate(mt.DIRS):
        flags[:nx - dx, :ny - dy, :nz - dz, d] = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
    return np.flatnonzero(flags.reshape(-1)).astype(np.int64)


def renumber(verts, faces, edge_ids):
    """The mesh with its vertices in increasing edge_id (the dense numbering) and its faces as a canonical multiset: each triangle
    rotated (orientation kept) to start at its smallest index, the rows sorted."""
    ids = np.asarray(edge_ids, dtype=np.int64)
    order = np.argsort(ids, kind="stable")
    new_of_old = np.empty(len(ids), dtype=np.int64)
    new_of_old[order] = np.arange(len(ids))
    return np.asarray(verts)[order], canonical_faces(new_of_old[np.asarray(faces, dtype=np.int64)] if len(faces) else faces), ids[order]


def canonical_faces(faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return f
    r = np.argmin(f, axis=1)
    rows = np.arange(len(f))[:, None]
    f = f[rows, (r[:, None] + np.arange(3)[None, :]) % 3]
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]

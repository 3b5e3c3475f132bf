"""NumPy restatement of the mesh simplification (include/mofanerf_hip.h, mofa_simp_*; mofanerf_amd.mesh.simplify): cell keys in fp32,
face quadrics in fp64, the two-level sums in the kernel's fixed order and tree, the 3 x 3 solve in the header's operation order, the
three-way fallback, the face rules (degenerate faces, fins) and the compaction — to the bit.  Test code, not product.  ``mismatches`` is
THE comparison: the GPU tests assert that it returns nothing, the CPU tests show that it sees every injected fault (``fault=``).
The checkers (``edge_balance``, ``cell_violations``, ``optimality_violations``) are written independently of the restatement's own path."""
import numpy as np

import cc_reference as cc
import mt_reference as mt

CHUNK = 1024                 # mesh.CC_CHUNK
CELLS = 2 ** 21
COUNTERS = ("placed_quadric", "placed_mean", "placed_first", "mean_requested")
NUMBERS = ("n_clusters", "verts_in", "faces_in", "verts_out", "faces_out", "faces_degenerate", "faces_cancelled", "edges_multiple") + COUNTERS
FAULTS = ("key_round", "origin_ignored", "once_per_face", "d_sign", "mean_all", "no_containment", "w_a00", "fins_kept", "fins_adjacent",
          "dups_dropped", "input_order", "orientation_lost")


class Refused(ValueError):
    """What mesh.simplify answers with MofaError."""


# ---- keys -------------------------------------------------------------------------------------------------------------------------------
def cell3(cell):
    c = np.asarray(cell, dtype=np.float32).reshape(-1)
    return np.repeat(c, 3) if c.size == 1 else c.reshape(3)


def default_origin(verts):
    return np.asarray(verts, dtype=np.float32).reshape(-1, 3).min(0)


def keys(points, origin, cell, fault=None):
    """(keys [n] int64, number of points without one): q = floorf((x - origin) / cell) in fp32, every operation rounded separately;
    -1 for a non-finite coordinate or a q outside [0, 2^21)."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    o = np.zeros(3, dtype=np.float32) if fault == "origin_ignored" else np.asarray(origin, dtype=np.float32).reshape(3)
    c = cell3(cell)
    with np.errstate(all="ignore"):
        t = ((p - o) / c).astype(np.float32)
        t = np.rint(t) if fault == "key_round" else np.floor(t)
        ok = ((t >= 0) & (t < CELLS)).all(1)
    q = np.where(ok[:, None], t, 0).astype(np.int64)
    k = np.where(ok, (q[:, 0] << 42) | (q[:, 1] << 21) | q[:, 2], -1)
    return k, int((~ok).sum())


# ---- quadrics ---------------------------------------------------------------------------------------------------------------------------
def face_quadrics(verts, faces, fault=None):
    """[F,10] float64: A00 A01 A02 A11 A12 A22 b0 b1 b2 c of n = (v1 - v0) x (v2 - v0), d = -n . v0, in the kernel's operation order."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    p, q, r = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = q - p, r - p
    nx, ny, nz = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    d = -((nx * p[:, 0] + ny * p[:, 1]) + nz * p[:, 2])
    if fault == "d_sign":
        d = -d
    return np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d, d * d], 1)


# ---- the fixed-order, fixed-tree sums -----------------------------------------------------------------------------------------------------
def seg_sum(rows, start, end):
    """out[s] = the kernel's sum of rows[start[s]:end[s]]: thread t adds rows t, t + 256, ... from +0.0, then the tree over 256 partial
    sums.  (Padding with +0.0 is exact: a partial sum that started at +0.0 is never -0.0.)"""
    rows = np.asarray(rows, dtype=np.float64)
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    n = end - start
    out = np.zeros((len(start), rows.shape[1]))
    iters = np.maximum((n + 255) // 256, 1)
    padded = np.concatenate([rows, np.zeros((1, rows.shape[1]))])
    for k in np.unique(iters):
        seg = np.flatnonzero(iters == k)
        for lo in range(0, len(seg), 256):                          # (blocks: bounded memory)
            s = seg[lo:lo + 256]
            idx = start[s, None] + np.arange(k * 256)[None, :]
            idx = np.where(idx < end[s, None], idx, len(rows))
            vals = padded[idx].reshape(len(s), k, 256, rows.shape[1])
            acc = np.zeros((len(s), 256, rows.shape[1]))
            for j in range(k):
                acc = acc + vals[:, j]
            w = 128
            while w >= 1:
                acc = acc[:, :w] + acc[:, w:2 * w]
                w //= 2
            out[s] = acc[:, 0]
    return out


def two_level_sum(rows, counts):
    """Per label, the sum of its run of ``rows`` (sorted by label, ``counts`` per label): chunks of CHUNK rows first, then each label's
    chunks — mesh.simplify's two launches of mofa_simp_seg_sum."""
    counts = np.asarray(counts, dtype=np.int64)
    run = np.concatenate([[0], np.cumsum(counts)])
    per_label = (counts + CHUNK - 1) // CHUNK
    first = np.concatenate([[0], np.cumsum(per_label)])
    label_of = np.repeat(np.arange(len(counts)), per_label)
    start = run[label_of] + CHUNK * (np.arange(first[-1]) - first[label_of])
    partial = seg_sum(rows, start, np.minimum(start + CHUNK, run[label_of + 1]))
    return seg_sum(partial, first[:-1], first[1:])


# ---- placement --------------------------------------------------------------------------------------------------------------------------
def place(Q, S, cluster_keys, first_verts, origin, cell, regularize, placement, fault=None):
    """(rep [C,3] float32, route [C]: 1 quadric, 2 mean, 3 first vertex): the header's operation order, the three-way fallback."""
    C = len(Q)
    with np.errstate(all="ignore"):
        m = S[:, :3] / S[:, 3:4]
        route = np.zeros(C, dtype=np.int64)
        rep = np.zeros((C, 3), dtype=np.float32)
        if placement == "quadric":
            w = regularize * (Q[:, 0] if fault == "w_a00" else ((Q[:, 0] + Q[:, 3]) + Q[:, 5]))
            a00, a11, a22, a01, a02, a12 = Q[:, 0] + w, Q[:, 3] + w, Q[:, 5] + w, Q[:, 1], Q[:, 2], Q[:, 4]
            r0, r1, r2 = w * m[:, 0] - Q[:, 6], w * m[:, 1] - Q[:, 7], w * m[:, 2] - Q[:, 8]
            c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
            c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
            det = (a00 * c00 + a01 * c01) + a02 * c02
            x = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                          ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1).astype(np.float32)
            ok = (w > 0) & np.isfinite(w) & (det > 0) & np.isfinite(det)
            inside = keys(x, origin, cell)[0] == cluster_keys
            if fault == "no_containment":
                inside = np.isfinite(x).all(1)
            ok &= inside
            rep[ok], route[ok] = x[ok], 1
        mean = m.astype(np.float32)
        ok = (route == 0) & (keys(mean, origin, cell)[0] == cluster_keys)
        if fault == "no_containment":
            ok = route == 0
        rep[ok], route[ok] = mean[ok], 2
    rest = route == 0
    rep[rest], route[rest] = first_verts[rest], 3
    return rep, route


# ---- the face rules ---------------------------------------------------------------------------------------------------------------------
def canonical(tri, fault=None):
    """Rows rotated so that the (first) smallest index comes first, the cyclic order kept."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    if fault == "orientation_lost":
        return np.sort(tri, 1)
    k = np.argmin(tri, 1)
    return np.take_along_axis(tri, (k[:, None] + np.arange(3)[None, :]) % 3, 1)


def cancel_fins(rot, fault=None):
    """Keep mask over canonical non-degenerate faces: among the faces with one vertex set, with p and q faces of the two orientations,
    the first |p - q| of the majority orientation in face order."""
    n = len(rot)
    if n == 0 or fault == "fins_kept":
        return np.ones(n, dtype=bool)
    odd = (rot[:, 1] > rot[:, 2]).astype(np.int64)
    _, g = np.unique(np.sort(rot, 1), axis=0, return_inverse=True)
    g = g.reshape(-1)
    if fault == "fins_adjacent":
        keep = np.ones(n, dtype=bool)
        i = 0
        while i + 1 < n:
            if g[i] == g[i + 1] and odd[i] != odd[i + 1]:
                keep[i] = keep[i + 1] = False
                i += 2
            else:
                i += 1
        return keep
    k = 2 * g + odd
    order = np.argsort(k, kind="stable")
    count = np.bincount(k, minlength=2 * (int(g.max()) + 1))
    begin = np.cumsum(count) - count
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n) - begin[k[order]]
    keep = rank < count[k] - count[k ^ 1]
    if fault == "dups_dropped":
        keep &= rank < 1
    return keep


def edges_multiple(faces):
    """Directed edges that more than one face uses."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return 0
    e = mt.directed_edges(f)
    _, n = np.unique(e[:, 0] * (1 << 31) + e[:, 1], return_counts=True)
    return int((n > 1).sum())


# ---- the whole pass ---------------------------------------------------------------------------------------------------------------------
def simplify(verts, faces, cell, origin=None, regularize=1e-3, placement="quadric", fault=None):
    """(verts', faces', stats) as mesh.simplify gives them, NumPy arrays; ``stats`` also holds the intermediate ``keys_out`` (the key of
    every output vertex), ``origin``, ``cell`` and, before the compaction, ``cluster`` [V], ``rep`` [C,3], ``route`` [C], ``used`` [C]."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V, F = len(verts), len(faces)
    c3 = cell3(cell)
    if not (np.isfinite(c3).all() and (c3 > 0).all()):
        raise Refused(f"cell = {cell}")
    if not (np.isfinite(regularize) and regularize > 0):
        raise Refused(f"regularize = {regularize}")
    if placement not in ("quadric", "mean"):
        raise Refused(f"placement = {placement}")
    if V == 0 or F == 0:
        stats = dict.fromkeys(NUMBERS, 0)
        stats.update(verts_in=V, faces_in=F, cluster_of=np.full(V, -1, dtype=np.int32))
        return np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32), stats
    bad = int(((faces < 0) | (faces >= V)).sum())
    if bad:
        raise Refused(f"{bad} of the {3 * F} face indices lie outside [0, {V})")
    o3 = default_origin(verts) if origin is None else np.asarray(origin, dtype=np.float32).reshape(3)
    if not np.isfinite(o3).all():
        raise Refused(f"origin = {o3}")
    key, bad = keys(verts, o3, c3, fault)
    if bad:
        raise Refused(f"{bad} of the {V} vertices have no cell")
    f64 = faces.astype(np.int64)
    referenced = np.zeros(V, dtype=bool)
    referenced[f64.reshape(-1)] = True
    cluster_keys, inverse = np.unique(key[referenced], return_inverse=True)
    C = len(cluster_keys)
    cluster = np.full(V, -1, dtype=np.int64)
    cluster[referenced] = inverse.reshape(-1)
    # per cluster: (x, y, z, 1) over its referenced vertices, stably sorted by cluster (the unreferenced -1 come first)
    member = cluster
    if fault == "mean_all":
        at = np.minimum(np.searchsorted(cluster_keys, key), C - 1)
        member = np.where(cluster_keys[at] == key, at, -1)
    order = np.argsort(member, kind="stable")
    order = order[int((member < 0).sum()):]
    n_verts = np.bincount(member[member >= 0], minlength=C)
    S = two_level_sum(np.concatenate([verts[order].astype(np.float64), np.ones((len(order), 1))], 1), n_verts)
    first = order[np.cumsum(n_verts) - n_verts]
    if placement == "quadric":
        corner = cluster[f64].reshape(-1)
        perm = np.argsort(corner, kind="stable")
        if fault == "once_per_face":
            new = cluster[f64]
            dup = np.stack([np.zeros(F, dtype=bool), new[:, 1] == new[:, 0], (new[:, 2] == new[:, 0]) | (new[:, 2] == new[:, 1])], 1).reshape(-1)
            perm = perm[~dup[perm]]
        Q = two_level_sum(face_quadrics(verts, faces, fault)[perm // 3], np.bincount(corner[perm], minlength=C))
    else:
        Q = np.zeros((C, 10))
    rep, route = place(Q, S, cluster_keys, verts[first], o3, c3, float(regularize), placement, fault)
    # faces
    new = cluster[f64]
    degenerate = (new[:, 0] == new[:, 1]) | (new[:, 1] == new[:, 2]) | (new[:, 2] == new[:, 0])
    rot = canonical(new[~degenerate], fault)
    keep = cancel_fins(rot, fault)
    kept = rot[keep]
    used = np.zeros(C, dtype=bool)
    used[kept.reshape(-1)] = True
    vmap = np.where(used, np.cumsum(used) - 1, -1)
    out_v, out_f = rep[used], vmap[kept].astype(np.int32).reshape(-1, 3)
    cluster_of = np.where(cluster >= 0, vmap[np.maximum(cluster, 0)], -1).astype(np.int32)
    keys_out = cluster_keys[used]
    if fault == "input_order":                                       # output vertices by their first input vertex instead of by key
        by_first = np.argsort(first[used], kind="stable")
        back = np.empty_like(by_first)
        back[by_first] = np.arange(len(by_first))
        out_v, keys_out = out_v[by_first], keys_out[by_first]
        out_f = back[out_f].astype(np.int32).reshape(-1, 3)
        cluster_of = np.where(cluster_of >= 0, back[np.maximum(cluster_of, 0)], -1).astype(np.int32)
    stats = dict(n_clusters=C, verts_in=V, faces_in=F, verts_out=len(out_v), faces_out=len(out_f), faces_degenerate=int(degenerate.sum()),
                 faces_cancelled=int((~keep).sum()), placed_quadric=int((route == 1).sum()), placed_mean=int((route == 2).sum()),
                 placed_first=int((route == 3).sum()), mean_requested=C if placement == "mean" else 0, edges_multiple=edges_multiple(out_f),
                 cluster_of=cluster_of, keys_out=keys_out, origin=o3, cell=c3, cluster=cluster, rep=rep, route=route, used=used)
    return np.ascontiguousarray(out_v), np.ascontiguousarray(out_f), stats


# ---- the comparison the GPU tests use -----------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind == "f" else a


def mismatches(got, want):
    """Names of what differs between two (verts', faces', stats) results: the vertices' bits, the faces, ``cluster_of`` and every number."""
    (gv, gf, gs), (wv, wf, ws) = got, want
    bad = []
    for name, g, w, dt in (("verts", gv, wv, np.float32), ("faces", gf, wf, np.int32), ("cluster_of", gs["cluster_of"], ws["cluster_of"], np.int32)):
        g = np.asarray(g)
        if g.dtype != dt or g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)):
            bad.append(name)
    return bad + [k for k in NUMBERS if int(gs[k]) != int(ws[k])]


# ---- independent checkers -----------------------------------------------------------------------------------------------------------------
def edge_balance(faces):
    """Net use count(a -> b) - count(b -> a) of every undirected edge {a < b} some face uses: all zero for a closed, consistently
    oriented mesh."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = mt.directed_edges(f)
    e = e[e[:, 0] != e[:, 1]]
    if len(e) == 0:
        return np.zeros(0, dtype=np.int64)
    sign = np.where(e[:, 0] < e[:, 1], 1, -1)
    _, inv = np.unique(e.min(1) * (1 << 32) + e.max(1), return_inverse=True)
    return np.bincount(inv.reshape(-1), weights=sign).astype(np.int64)


def cell_violations(points, want_keys, origin, cell):
    """How many points do not lie in the cell their key names (the key arithmetic, redone per point with Python scalars of float32)."""
    o, c = np.asarray(origin, dtype=np.float32), cell3(cell)
    bad = 0
    for p, k in zip(np.asarray(points, dtype=np.float32).reshape(-1, 3), np.asarray(want_keys).tolist()):
        q = [int(np.floor(np.float32(np.float32(p[a] - o[a]) / c[a]))) if np.isfinite(p[a]) else -1 for a in range(3)]
        bad += not (all(0 <= v < CELLS for v in q) and (q[0] << 42 | q[1] << 21 | q[2]) == k)
    return bad


def optimality_violations(verts, faces, stats, regularize):
    """For every quadric-placed cluster, recomputed in np.longdouble from the faces: G(x) = E(x) + w |x - m|^2 <= E(m) = G(m), where
    E(x) = the sum over the cluster's corners of (n . (x - v0))^2, w = regularize * trace(A), m = the mean of its vertices.  x is the exact
    minimiser of G rounded twice (the fp64 solve, then fp32); G is quadratic, so G(x) - G(x*) = 1/2 grad G(x) . (x - x*), and with
    |x_a - x*_a| <= half an ulp of the fp32 x_a the slack is sum_a |grad G(x)_a| ulp(x_a) / 2 — derived, not tuned (it is twice the
    bound; the fp64 solve's error enters only squared).  Returns (violations, clusters checked, the largest (G(x) - E(m)) / slack)."""
    L = np.longdouble
    v = np.asarray(verts, dtype=np.float32).astype(L)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    cluster, rep, route = stats["cluster"], stats["rep"], stats["route"]
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    v0 = v[f[:, 0]]
    corner_cluster = cluster[f]
    bad, checked, worst = 0, 0, -np.inf
    for c in np.flatnonzero(route == 1):
        rows = np.concatenate([np.flatnonzero(corner_cluster[:, k] == c) for k in range(3)])       # a face counts once per corner in c
        nn, pp = n[rows], v0[rows]
        members = np.flatnonzero(cluster == c)
        m = v[members].sum(0) / L(len(members))
        w = L(regularize) * (nn * nn).sum()
        x = rep[c].astype(L)
        E = lambda y: (((y - pp) * nn).sum(1) ** 2).sum()
        grad = 2 * (nn * ((x - pp) * nn).sum(1)[:, None]).sum(0) + 2 * w * (x - m)
        slack = (np.abs(grad) * (np.spacing(np.abs(rep[c])).astype(L) / 2)).sum()
        excess = E(x) + w * ((x - m) ** 2).sum() - E(m)
        checked += 1
        bad += bool(excess > slack)
        if slack > 0:
            worst = max(worst, float(excess / slack))
    return bad, checked, worst


# ---- test meshes ------------------------------------------------------------------------------------------------------------------------
def lattice_cell(step, m):
    """The cell of m grid steps per axis, as Renderer.extract_mesh(simplify=m) computes it: float32(m) * step in float32."""
    return (np.float32(m) * np.asarray(step, dtype=np.float32)).astype(np.float32)


def shell_mesh(res=(41, 41, 41)):
    grid, lo, step = cc.shell_field(res)
    return mt.marching_tets(grid, 0.0, lo, step) + (lo, step)


def tetrahedron():
    """One vertex per unit cell, outward orientation."""
    verts = np.array([(0.5, 0.5, 0.5), (1.5, 0.25, 0.5), (0.5, 1.5, 0.75), (0.25, 0.5, 1.5)], dtype=np.float32)
    return verts, np.array([(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)], dtype=np.int32)


def tetrahedron_with_stray():
    """The tetrahedron plus a vertex no face references, in vertex 0's cell: it belongs to no cluster and to no mean."""
    verts, faces = tetrahedron()
    return np.concatenate([verts, np.array([(0.125, 0.875, 0.25)], dtype=np.float32)]), faces


def fin_mesh(n_between=40, seed=2):
    """A tetrahedron (one vertex per unit cell) whose face (1, 2, 3) also appears reversed, far apart in face order: ``n_between`` more
    copies of the tetrahedron's other faces lie between the two, and the pair must still cancel."""
    verts, faces = tetrahedron()
    filler = np.tile(faces[:3], (n_between, 1))
    return verts, np.concatenate([faces, filler, [(3, 2, 1)]]).astype(np.int32)


def three_and_one():
    """Three copies of one face (two of them rotated) and one opposite: two of the three survive."""
    verts, _ = tetrahedron()
    return verts, np.array([(0, 1, 2), (1, 2, 0), (2, 1, 0), (2, 0, 1)], dtype=np.int32)


def boundary_mesh():
    """Vertices exactly at the origin, on cell boundaries and just below them, cells of 0.25 from the origin (-1, -1, -1)."""
    b = np.float32(-0.5)
    verts = np.array([(-1, -1, -1), (b, -1, -1), (np.nextafter(b, np.float32(-1)), -1, -1), (-1, b, -0.75), (-1, -1, 0.25), (0, 0, 0),
                      (-0.5, -0.5, -0.5), (0.7, 0.1, -0.3)], dtype=np.float32)
    faces = np.array([(0, 1, 3), (1, 2, 4), (2, 5, 6), (0, 4, 7), (3, 6, 7), (1, 5, 7), (0, 2, 1)], dtype=np.int32)
    return verts, faces, np.full(3, -1, dtype=np.float32), np.float32(0.25)


def two_cell_strip(V, seed):
    """cc_reference.strip with its vertices squeezed into two cells of size 1 from the origin 0: x in [0, 2), y and z in [0, 1).  One
    cluster's corners span many chunks of CHUNK.  Every face of the strip is degenerate then, so two more vertices in cells of their own
    and two faces that join them to the two big clusters keep both representatives in the output."""
    _, faces = cc.strip(V, seed)
    rng = np.random.default_rng(seed + 1)
    verts = rng.random((V + 2, 3)).astype(np.float32) * np.float32(0.999)
    verts[:V, 0] += (rng.random(V) < 0.5).astype(np.float32)
    verts[V:, 0] += np.array([2, 3], dtype=np.float32)
    left, right = int(np.flatnonzero(verts[:V, 0] < 1)[0]), int(np.flatnonzero(verts[:V, 0] >= 1)[0])
    faces = np.concatenate([faces, [(left, right, V), (left, V, V + 1)]]).astype(np.int32)
    return verts, faces, np.zeros(3, dtype=np.float32), np.float32(1.0)


def fan_of_corners(n_corners, seed):
    """A fan around vertex-cluster 0 with exactly ``n_corners`` corners in cell 0: faces (hub_i, rim_j, rim_j+1) whose hub vertices all lie
    in cell 0 and whose rim vertices have a cell of their own each (cells of size 1, origin 0)."""
    rng = np.random.default_rng(seed)
    n_rim = 9
    hub = (rng.random((n_corners, 3)).astype(np.float32) * np.float32(0.9) + np.float32(0.05))
    rim = np.stack([np.arange(1, n_rim + 1), np.zeros(n_rim), np.zeros(n_rim)], 1).astype(np.float32) + rng.random((n_rim, 3)).astype(np.float32) * np.float32(0.5)
    j = np.arange(n_corners) % (n_rim - 1)
    faces = np.stack([np.arange(n_corners), n_corners + j, n_corners + j + 1], 1).astype(np.int32)
    return np.concatenate([hub, rim]), faces, np.zeros(3, dtype=np.float32), np.float32(1.0)

"""NumPy restatement of the mesh winding number (include/mofanerf_hip.h, mofa_wind_*; mesh.winding_number / signed_distance /
surface_distance(signed=True)): the vertex classes, the canonical edge flags and the height test in float64 on the float32 coordinates
widened, every difference and product rounded separately; brute force over all faces, the 2-D binning and the column walk with its
counters, the open-edge count and the signed statistics.  Test code, not product: the GPU output must equal it integer for integer.

``faults`` (a collection of names) injects the mistakes the tests must be able to see, one per name in FAULTS."""
import numpy as np

FAULTS = ("both_closed", "per_face_edge", "no_height_test", "unsigned", "swap_uv", "no_range_clamp")
COUNTERS = ("non_finite_queries", "flat_faces")                 # the counters no grid changes
WALK_COUNTERS = COUNTERS + ("face_tests", "max_column")         # and those of one grid's walk


def widen(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def axes(axis, faults=()):
    """(u, v, a): (u, v, a) is right-handed."""
    a = int(axis)
    if a not in (0, 1, 2):
        raise ValueError(f"axis = {axis}")
    u, v = (a + 1) % 3, (a + 2) % 3
    return (v, u, a) if "swap_uv" in faults else (u, v, a)


def _edge(p, A, B, rA, rB, u, v, faults):
    """The contribution (-1, 0, +1) of the edge A -> B of a face; p [N,1,3], A / B [1,F,3], rA / rB [N,F] the classes of its endpoints."""
    straddle = rA != rB
    L, R = np.where(rA[..., None], B, A), np.where(rA[..., None], A, B)          # the non-right and the right endpoint: the same for both faces
    pu, pv = p[..., u], p[..., v]
    if "per_face_edge" in faults:                                                # the face's own direction, the same strict test both ways
        E = (B[..., u] - A[..., u]) * (pv - A[..., v]) - (B[..., v] - A[..., v]) * (pu - A[..., u])
        above = np.where(rA, ~(E < 0), E < 0)
    else:
        E = (R[..., u] - L[..., u]) * (pv - L[..., v]) - (R[..., v] - L[..., v]) * (pu - L[..., u])
        above = E < 0
    if "no_range_clamp" not in faults:
        above = np.where(pv >= np.maximum(L[..., v], R[..., v]), False, np.where(pv < np.minimum(L[..., v], R[..., v]), True, above))
    return np.where(straddle & above, np.where(rA, 1, -1), 0).astype(np.int8)


def pair_w(points, verts, faces, axis=2, faults=(), chunk=1 << 21):
    """[N, F] int8: what face f adds to the winding number of query i (steps 1-3: -1, 0 or +1; a non-finite query gets 0)."""
    u, v, a = axes(axis, faults)
    p = widen(points).reshape(-1, 3)
    X = widen(verts).reshape(-1, 3)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]            # [F, 3 corners, 3]
    N, F = len(p), len(X)
    out = np.zeros((N, F), dtype=np.int8)
    if N == 0 or F == 0:
        return out
    finite = np.isfinite(p).all(1)
    x = [X[None, :, k] for k in range(3)]
    step = max(1, chunk // F)
    with np.errstate(all="ignore"):
        for i0 in range(0, N, step):
            q = p[i0:i0 + step, None, :]
            if "both_closed" in faults:                                                          # per edge: >= at its start, > at its end
                cls = [(x[k][..., u] >= q[..., u], x[(k + 1) % 3][..., u] > q[..., u]) for k in range(3)]
            else:
                r = [x[k][..., u] > q[..., u] for k in range(3)]
                cls = [(r[k], r[(k + 1) % 3]) for k in range(3)]
            w = np.zeros((len(q), F), dtype=np.int8)
            for k in range(3):
                w += _edge(q, x[k], x[(k + 1) % 3], cls[k][0], cls[k][1], u, v, faults)
            lo = np.minimum(np.minimum(x[0][..., a], x[1][..., a]), x[2][..., a])
            hi = np.maximum(np.maximum(x[0][..., a], x[1][..., a]), x[2][..., a])
            ab, ac, d = x[1] - x[0], x[2] - x[0], q - x[0]
            n = (ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                 ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0])
            s = (n[0] * d[..., 0] + n[1] * d[..., 1]) + n[2] * d[..., 2]
            hit = np.where(w > 0, s < 0, s > 0)
            if "no_range_clamp" not in faults:
                hit = np.where(q[..., a] < lo, True, np.where(q[..., a] >= hi, False, hit))
            if "no_height_test" in faults:
                hit = np.ones_like(hit)
            w = np.where(hit, w, 0).astype(np.int8)
            w[~finite[i0:i0 + step]] = 0
            out[i0:i0 + step] = w
    return out


def flat_faces(verts, faces, axis=2, faults=()):
    """[F] bool: faces without extent in u or in v (they enter no cell and can never be crossed)."""
    u, v, _ = axes(axis, faults)
    X = widen(verts).reshape(-1, 3)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    return (X[..., u].min(1) == X[..., u].max(1)) | (X[..., v].min(1) == X[..., v].max(1)) if len(X) else np.zeros(0, dtype=bool)


def _result(points, W, faults):
    finite = np.isfinite(widen(points).reshape(-1, 3)).all(1)
    W = W.astype(np.int32)
    winding = np.abs(W).sum(1) if "unsigned" in faults else W.sum(1)
    return {"winding": winding.astype(np.int32), "crossings": np.abs(W).sum(1).astype(np.int32), "inside": winding != 0}, finite


def brute_force(points, verts, faces, axis=2, faults=(), pairs=None):
    """What mesh.winding_number returns (``winding``, ``crossings``, ``inside``, ``counts`` without the walk's counters): every face for
    every query."""
    W = pairs if pairs is not None else pair_w(points, verts, faces, axis, faults)
    out, finite = _result(points, W, faults)
    out["counts"] = {"non_finite_queries": int((~finite).sum()), "flat_faces": int(flat_faces(verts, faces, axis, faults).sum())}
    return out


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
def grid_of(verts, n, axis=2, faults=()):
    """(origin [2], cell [2], n [2]) of the grid of ``n`` cells (an int or a pair) over the (u, v) box of ``verts``, as mesh.wind_grid
    computes them."""
    u, v, _ = axes(axis, faults)
    x = widen(verts).reshape(-1, 3)[:, [u, v]]
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), (2,)).copy()
    origin = x.min(0)
    extent = x.max(0) - origin
    with np.errstate(all="ignore"):
        cell = np.where(extent > 0, extent / n.astype(np.float64), 1.0)
    return origin, cell, n


def cell_index(x, origin, cell, n):
    with np.errstate(all="ignore"):
        t = np.floor((x - origin) / cell)
    return np.where(t >= 0, np.where(t < n, t, n - 1), 0).astype(np.int64)


def bin_faces(verts, faces, grid, axis=2, faults=()):
    """(cell_start [cells + 1], pair_face [P], flat count): every face with extent in u and in v in every cell of idx(min u) .. idx(max u)
    x idx(min v) .. idx(max v), the pairs sorted stably by cell id iu n[1] + iv."""
    u, v, _ = axes(axis, faults)
    origin, cell, n = grid
    X = widen(verts).reshape(-1, 3)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)][..., [u, v]]          # [F, 3, 2]
    flat = flat_faces(verts, faces, axis, faults)
    cells, ids = [], []
    if len(X):
        lo, hi = cell_index(X.min(1), origin, cell, n), cell_index(X.max(1), origin, cell, n)
        for i in np.flatnonzero(~flat):
            gu, gv = np.meshgrid(np.arange(lo[i, 0], hi[i, 0] + 1), np.arange(lo[i, 1], hi[i, 1] + 1), indexing="ij")
            cid = (gu * n[1] + gv).reshape(-1)
            cells.append(cid)
            ids.append(np.full(len(cid), i, dtype=np.int64))
    cells = np.concatenate(cells) if cells else np.zeros(0, dtype=np.int64)
    ids = np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)
    by = np.argsort(cells, kind="stable")
    start = np.zeros(int(n.prod()) + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(cells, minlength=int(n.prod())))
    return start, ids[by], int(flat.sum())


def column_walk(points, verts, faces, n, axis=2, faults=(), pairs=None):
    """What mesh.winding_number returns at grid ``n``, by the kernel's walk: the clamped column of (p.u, p.v) and the faces listed there, in
    list order.  ``counts`` also holds ``face_tests`` (the listed faces walked) and ``max_column`` (the longest list a query walked).  The
    pair arithmetic comes from pair_w (a function of the pair alone)."""
    u, v, _ = axes(axis, faults)
    p = widen(points).reshape(-1, 3)
    grid = grid_of(verts, n, axis, faults)
    origin, cell, n = grid
    W = pairs if pairs is not None else pair_w(points, verts, faces, axis, faults)
    start, pair_face, n_flat = bin_faces(verts, faces, grid, axis, faults)
    finite = np.isfinite(p).all(1)
    listed = np.zeros(W.shape, dtype=bool)
    tests = longest = 0
    for i in np.flatnonzero(finite):
        c = cell_index(p[i, [u, v]], origin, cell, n)
        col = int(c[0] * n[1] + c[1])
        ids = pair_face[start[col]:start[col + 1]]
        listed[i, ids] = True
        tests += len(ids)
        longest = max(longest, len(ids))
    out, _ = _result(points, np.where(listed, W, 0), faults)
    out["counts"] = {"non_finite_queries": int((~finite).sum()), "flat_faces": n_flat, "face_tests": tests, "max_column": longest}
    return out


def mismatches(got, want, counters=COUNTERS):
    """The names of what differs between two results: ``winding``, ``crossings``, ``inside`` (dtype, shape, every integer) and ``counters``."""
    bad = []
    for k in ("winding", "crossings", "inside"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype != w.dtype or g.shape != w.shape or not np.array_equal(g, w):
            bad.append(k)
    return bad + [k for k in counters if int(got["counts"][k]) != int(want["counts"][k])]


# ---- closedness and the signed statistics -----------------------------------------------------------------------------------------------
def open_edges(faces):
    """The directed edges (a, b) with count(a -> b) != count(b -> a), each such pair of directions counted once per direction present."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not len(f):
        return 0
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    count = {}
    for a, b in e.tolist():
        count[a, b] = count.get((a, b), 0) + 1
    return sum(1 for (a, b), c in count.items() if count.get((b, a), 0) != c)


def signed_stats(d, weight, found, inside):
    """signed_mean / inside_fraction over the samples with a weight, max_inside / max_outside over all of them, of the distances ``d``
    (float64) that were found."""
    nan = float("nan")
    out = {"signed_mean": nan, "inside_fraction": nan, "max_inside": nan, "max_outside": nan}
    d, weight, inside = d[found], weight[found], inside[found]
    if inside.any():
        out["max_inside"] = float(d[inside].max())
    if (~inside).any():
        out["max_outside"] = float(d[~inside].max())
    keep = weight > 0
    d, weight, inside = d[keep], weight[keep], inside[keep]
    total = weight.sum()
    if len(d) and total > 0:
        out["signed_mean"] = float((weight * np.where(inside, -d, d)).sum() / total)
        out["inside_fraction"] = float((weight * inside).sum() / total)
    return out


# ---- test meshes and query sets ---------------------------------------------------------------------------------------------------------
def cube(lo=0.0, hi=1.0, inward=False):
    """(verts [8,3] float32, faces [12,3] int32) of the cube [lo, hi]^3, normals outward (``inward``: reversed)."""
    c = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)          # index 4 x + 2 y + z
    verts = (lo + (hi - lo) * c).astype(np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]          # -x +x -y +y -z +z, outward
    faces = np.array([t for a, b, c_, d in quads for t in ((a, b, c_), (a, c_, d))], dtype=np.int32)
    return verts, (faces[:, ::-1].copy() if inward else faces)


def merged(*meshes):
    """One mesh of several: (verts, faces) concatenated with the indices shifted."""
    verts, faces, base = [], [], 0
    for v, f in meshes:
        verts.append(np.asarray(v, dtype=np.float32))
        faces.append(np.asarray(f, dtype=np.int32) + base)
        base += len(v)
    return np.concatenate(verts), np.concatenate(faces).astype(np.int32)


CUBE_LATTICE = (-0.5, 0.0, 0.25, 0.5, 1.0, 1.5)


def cube_queries():
    """(points [216,3] float32, on_surface [216] bool, inside [216] bool) for the unit cube: the lattice CUBE_LATTICE^3, whose rays pass
    through the cube's vertices, along its edges and through the diagonals of its faces."""
    g = np.array(CUBE_LATTICE, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    within = ((p >= 0) & (p <= 1)).all(1)
    interior = ((p > 0) & (p < 1)).all(1)
    return p, within & ~interior, interior


def sliver():
    """(verts, faces, queries, winding) for axis 2: one huge face at z = 5 whose tip R = (1 + e, 1 + e), e = 2^-23, lies just right of and
    above the query (1, 1, 0); seen from the tip the upper edge L -> R falls with slope -1 and the lower edge rises with slope 2, so at
    u = 1 the face covers v in [1 - e, 1 + 2 e]: the query's ray crosses it (winding +1 in this vertex order).  The query lies below the
    v-extent of the upper edge, which the range clamp decides ("above").  Without the clamp both differences to L = (-2^40, 2^40) absorb e,
    E rounds to exactly 0 and the tie reads "not above": the face is missed."""
    e, big = 2.0 ** -23, 2.0 ** 40
    verts = np.array([(-big, big, 5.0), (-big, -2 * big, 5.0), (1 + e, 1 + e, 5.0)], dtype=np.float32)
    return verts, np.array([(0, 1, 2)], dtype=np.int32), np.array([(1.0, 1.0, 0.0), (1.0, 1.0, 6.0)], dtype=np.float32), np.array([1, 0], dtype=np.int32)

_fields = {}


def field_case(name, n_queries=900, seed=0):
    """(verts, faces, queries, truth) of one of dist_reference.CASES or ``"shell"`` (cc_reference.shell_field on 21^3): the marching-
    tetrahedra mesh at level 0 and a fixed subsample of the extraction's own lattice points with ``grid != 0`` that are not bit-equal to a
    mesh vertex — the rays of these queries pass through mesh vertices and along mesh edges — with ``truth = grid > 0``."""
    key = (name, n_queries, seed)
    if key not in _fields:
        import cc_reference as cc
        import dist_reference as dr
        import mt_reference as mt
        if name == "shell":
            grid, lo, step = cc.shell_field((21, 21, 21))
            verts, faces = mt.marching_tets(grid, 0.0, lo, step)
        else:
            res = dict(dr.CASES)[name]
            verts, faces, lo, step = cc.field_mesh(name, res)
            grid = mt.field(name, res, lo, step)
        pts, keep = lattice_queries(grid, lo, step, verts)
        truth = (np.asarray(grid).reshape(-1) > 0)[keep]
        rng = np.random.default_rng(seed + len(name))
        n_in = min(n_queries // 2, int(truth.sum()))                               # half of them inside, where the lattice has that many
        pick = np.sort(np.concatenate([rng.choice(np.flatnonzero(truth), n_in, replace=False),
                                       rng.choice(np.flatnonzero(~truth), min(n_queries - n_in, int((~truth).sum())), replace=False)]))
        _fields[key] = (verts, faces, pts[pick], truth[pick])
    return _fields[key]


def lattice_queries(grid, lo, step, verts):
    """(points, flat indices) of the lattice points of ``grid`` with ``grid != 0`` that are not bit-equal to a vertex of ``verts``."""
    import mt_reference as mt
    g = np.asarray(grid, dtype=np.float32)
    pts = mt.grid_points(g.shape, lo, step)
    as_rows = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float32) + np.float32(0)).view(np.dtype((np.void, 12))).reshape(-1)   # (-0 -> +0)
    keep = np.flatnonzero((g.reshape(-1) != 0) & ~np.isin(as_rows(pts), as_rows(verts)))
    return pts[keep], keep

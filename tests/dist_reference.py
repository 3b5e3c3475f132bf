"""NumPy restatement of the mesh surface distance (include/mofanerf_hip.h, mofa_dist_*; mofanerf_amd.mesh.closest_points / sample_faces /
surface_distance): the point-triangle arithmetic operation by operation, brute force over all faces, the grid with its binning, ring walk,
termination bound and ``max_distance``, the quadrature, and the statistics.  Test code, not product.  ``mismatches`` is THE comparison:
the GPU tests assert it returns nothing, tests/test_dist_reference_cpu.py shows that it sees every injected fault (``faults``: a set of
the names in FAULTS).  Two checkers that share nothing with the restatement (``np.longdouble`` optimality on a barycentric lattice, the
barycentric identities) judge the restatement itself."""
import numpy as np

FAULTS = ("edge_as_vertex", "swap_ab_ac", "no_projection", "tie_high", "stop_le", "stop_early", "reached_side", "centroid_binning", "no_clamp",
          "maxd_d2", "keep_degenerate", "f32_d2", "weights_no_k2", "order_transposed")
SHRINK = 1.0 - 2.0 ** -40
COUNTERS = ("degenerate_faces", "non_finite_queries")          # the counters no grid changes
WALK_COUNTERS = COUNTERS + ("candidate_tests", "max_ring")     # and those of one grid's walk


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def widen(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def zero_normal(a, b, c):
    """(the fp64 normal ab x ac [...,3], whether it is exactly zero)"""
    ab, ac = b - a, c - a
    n = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                  ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], -1)
    return n, (n == 0).all(-1)


def closest_on_triangle(p, a, b, c, faults=()):
    """The header's point-triangle arithmetic on broadcastable float64 arrays [...,3]: (d2, q, bary, ok); ``ok`` is False where the interior
    was reached with an unusable s (the face is skipped for that point)."""
    with np.errstate(all="ignore"):
        p, a, b, c = np.broadcast_arrays(p, a, b, c)
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        s = (va + vb) + vc
        rA = (d1 <= 0) & (d2 <= 0)
        left = ~rA
        rB = left & (d3 >= 0) & (d4 <= d3)
        left &= ~rB
        rAB = left & (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        left &= ~rAB
        rC = left & (d6 >= 0) & (d5 <= d6)
        left &= ~rC
        rAC = left & (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        left &= ~rAC
        rBC = left & (va <= 0) & (e >= 0) & (g >= 0)
        rIn = left & ~rBC
        ok = ~rIn | (np.isfinite(s) & (s > 0))
        if "swap_ab_ac" in faults:
            rAB, rAC = rAC, rAB
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        q = np.where(rA[..., None], a, np.where(rB[..., None], b, c))
        bary = np.where(rA[..., None], np.stack([one, zero, zero], -1), np.where(rB[..., None], np.stack([zero, one, zero], -1),
                                                                                 np.stack([zero, zero, one], -1)))
        v = d1 / (d1 - d3)
        qe, be = a + v[..., None] * ab, np.stack([1.0 - v, v, zero], -1)
        if "edge_as_vertex" in faults:
            qe, be = a, np.stack([one, zero, zero], -1)
        q, bary = np.where(rAB[..., None], qe, q), np.where(rAB[..., None], be, bary)
        w = d2 / (d2 - d6)
        qe, be = a + w[..., None] * ac, np.stack([1.0 - w, zero, w], -1)
        if "edge_as_vertex" in faults:
            qe, be = a, np.stack([one, zero, zero], -1)
        q, bary = np.where(rAC[..., None], qe, q), np.where(rAC[..., None], be, bary)
        w = e / (e + g)
        qe, be = b + w[..., None] * (c - b), np.stack([zero, 1.0 - w, w], -1)
        if "edge_as_vertex" in faults:
            qe, be = b, np.stack([zero, one, zero], -1)
        q, bary = np.where(rBC[..., None], qe, q), np.where(rBC[..., None], be, bary)
        v, w = vb / s, vc / s
        qe = (a + v[..., None] * ab) + w[..., None] * ac
        if "no_projection" in faults:
            qe = p
        q, bary = np.where(rIn[..., None], qe, q), np.where(rIn[..., None], np.stack([(1.0 - v) - w, v, w], -1), bary)
        lo, hi = np.where(a < b, a, b), np.where(a > b, a, b)
        lo, hi = np.where(c < lo, c, lo), np.where(c > hi, c, hi)
        q = np.where(q < lo, lo, q)
        q = np.where(q > hi, hi, q)
        d = p - q
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], q, bary, ok


def pair_d2(points, verts, faces, faults=(), chunk=1 << 20):
    """[N,F] float64: the squared distance of every point to every face as the kernel computes it; +inf where the face is skipped for the
    point (a NaN never wins either: it becomes +inf here) and for a degenerate face (unless the fault keeps it)."""
    p, v = widen(points).reshape(-1, 3), widen(verts).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    out = np.empty((len(p), len(f)))
    dead = np.zeros(len(f), dtype=bool) if "keep_degenerate" in faults else zero_normal(a, b, c)[1]
    rows = max(1, chunk // max(1, len(f)))
    for i in range(0, len(p), rows):
        d2, _, _, ok = closest_on_triangle(p[i:i + rows, None], a[None], b[None], c[None], faults)
        out[i:i + rows] = np.where(ok & ~np.isnan(d2) & ~dead[None], d2, np.inf)
    return out, int(zero_normal(a, b, c)[1].sum())


def _finish(points, verts, faces, best, best_d2, max_distance, faults):
    """The output record from every query's winning face (-1: none) and its d2."""
    p, v = widen(points).reshape(-1, 3), widen(verts).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    N = len(p)
    finite = np.isfinite(p).all(1)
    with np.errstate(all="ignore"):
        d = np.sqrt(best_d2)
        hit = finite & (best >= 0) & ((best_d2 if "maxd_d2" in faults else d) <= max_distance)
        closest, bary = np.full((N, 3), np.nan), np.full((N, 3), np.nan)
        if hit.any():
            t = f[best[hit]]
            d2w, q, br, _ = closest_on_triangle(p[hit], v[t[:, 0]], v[t[:, 1]], v[t[:, 2]], faults)
            assert np.array_equal(d2w, best_d2[hit])
            closest[hit], bary[hit] = q, br
        if "f32_d2" in faults:
            d = np.sqrt(best_d2.astype(np.float32)).astype(np.float64)
        return {"distance": np.where(finite, np.where(hit, d, np.inf), np.nan).astype(np.float32),
                "d2": np.where(finite, np.where(hit, best_d2, np.inf), np.nan), "face": np.where(hit, best, -1).astype(np.int32),
                "closest": closest.astype(np.float32), "bary": bary.astype(np.float32)}


def _pick(row, ids, faults):
    """(face, d2) among the candidate faces ``ids`` (any order, repeats allowed) of one query's row of pair_d2: the smaller d2, then the lower
    index; +inf never wins."""
    if len(ids) == 0:
        return -1, np.inf
    d = row[ids]
    m = d.min()
    if not m < np.inf:
        return -1, np.inf
    tied = ids[d == m]
    return int(tied.max() if "tie_high" in faults else tied.min()), float(m)


def brute_force(points, verts, faces, max_distance=np.inf, faults=(), pairs=None):
    """What mesh.closest_points returns (NumPy arrays, ``counts`` with the grid-independent counters) from all N x F pairs."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    D, n_deg = pairs if pairs is not None else pair_d2(points, verts, faces, faults)
    finite = np.isfinite(points).all(1)
    N, F = D.shape
    best, best_d2 = np.full(N, -1, dtype=np.int64), np.full(N, np.inf)
    if F:
        m = D.min(1)
        arg = (F - 1 - np.argmin(D[:, ::-1], 1)) if "tie_high" in faults else np.argmin(D, 1)
        ok = finite & (m < np.inf)
        best[ok], best_d2[ok] = arg[ok], m[ok]
    out = _finish(points, verts, faces, best, best_d2, max_distance, faults)
    out["counts"] = {"degenerate_faces": 0 if "keep_degenerate" in faults else n_deg, "non_finite_queries": int((~finite).sum())}
    return out


# ---- the grid ---------------------------------------------------------------------------------------------------------------------------
def grid_of(verts, n):
    """(origin, cell, slack, n) of the grid of ``n`` cells (an int or three) over the box of ``verts``, as mesh.dist_grid computes them."""
    v = widen(verts).reshape(-1, 3)
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), (3,)).copy()
    origin = v.min(0)
    extent = v.max(0) - origin
    nn = n.astype(np.float64)
    with np.errstate(all="ignore"):
        cell = np.where(extent > 0, extent / nn, 1.0)
    return origin, cell, 2.0 ** -40 * (np.abs(origin) + nn * cell), n


def cell_index(x, origin, cell, n, clamp=True):
    with np.errstate(all="ignore"):
        t = np.floor((x - origin) / cell)
    if not clamp:
        return t.astype(np.int64)
    return np.where(t >= 0, np.where(t < n, t, n - 1), 0).astype(np.int64)


def bin_faces(verts, faces, grid, faults=()):
    """(cell_start [cells + 1], pair_face [P], degenerate count): every non-degenerate face in every cell of its vertices' index box, the
    pairs sorted stably by cell id (ix ny + iy) nz + iz."""
    origin, cell, _, n = grid
    v = widen(verts).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    dead = zero_normal(a, b, c)[1]
    ia, ib, ic = (cell_index(x, origin, cell, n) for x in (a, b, c))
    lo, hi = np.minimum(np.minimum(ia, ib), ic), np.maximum(np.maximum(ia, ib), ic)
    if "centroid_binning" in faults:
        lo = hi = cell_index((a + b + c) / 3.0, origin, cell, n)
    cells, ids = [], []
    for i in range(len(f)):
        if dead[i] and "keep_degenerate" not in faults:
            continue
        gx, gy, gz = np.meshgrid(*(np.arange(lo[i, k], hi[i, k] + 1) for k in range(3)), indexing="ij")
        cid = ((gx * n[1] + gy) * n[2] + gz).reshape(-1)
        cells.append(cid)
        ids.append(np.full(len(cid), i, dtype=np.int64))
    cells = np.concatenate(cells) if cells else np.zeros(0, dtype=np.int64)
    ids = np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)
    by = np.argsort(cells, kind="stable")
    start = np.zeros(int(n.prod()) + 1, dtype=np.int64)
    start[1:] = np.cumsum(np.bincount(cells, minlength=int(n.prod())))
    return start, ids[by], int(dead.sum())


def grid_walk(points, verts, faces, n, max_distance=np.inf, faults=(), pairs=None, slack_on=True):
    """What mesh.closest_points returns at grid ``n``, by the kernel's walk: the clamped start cell, Chebyshev rings clipped to the grid,
    the bound from the sides that have not reached the grid's edge, the strict stop, ``max_distance``.  ``counts`` also holds
    ``candidate_tests`` and ``max_ring``.  The pair arithmetic comes from pair_d2 (a function of the pair alone).  ``slack_on=False``
    takes the bound without its slack and shrink factor: the walk the strict stop was written for (the CPU tests use it to show what the
    strictness protects; the kernel always has the slack)."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    p = points.astype(np.float64)
    grid = grid_of(verts, n)
    origin, cell, slack, n = grid
    SHRINK = globals()["SHRINK"] if slack_on else 1.0
    slack = slack if slack_on else np.zeros(3)
    D, n_deg = pairs if pairs is not None else pair_d2(points, verts, faces, faults)
    start, pair_face, _ = bin_faces(verts, faces, grid, faults)
    N = len(p)
    finite = np.isfinite(p).all(1)
    best, best_d2 = np.full(N, -1, dtype=np.int64), np.full(N, np.inf)
    tests = max_ring = 0
    for i in np.flatnonzero(finite):
        c = cell_index(p[i], origin, cell, n, clamp="no_clamp" not in faults)
        if ((c < 0) | (c >= n)).any():                       # (the fault only) a kernel that finds its cell outside the grid and gives up
            continue
        r = 0
        while True:
            lo, hi = np.maximum(c - r, 0), np.minimum(c + r, n - 1)
            gx, gy, gz = np.meshgrid(*(np.arange(lo[k], hi[k] + 1) for k in range(3)), indexing="ij")
            shell = np.maximum(np.maximum(np.abs(gx - c[0]), np.abs(gy - c[1])), np.abs(gz - c[2])) == r
            cid = ((gx * n[1] + gy) * n[2] + gz)[shell]
            ids = np.concatenate([pair_face[start[k]:start[k + 1]] for k in cid]) if len(cid) else np.zeros(0, dtype=np.int64)
            tests += len(ids)
            f, d2 = _pick(D[i], ids, faults)
            if d2 < best_d2[i] or (d2 == best_d2[i] and f >= 0 and ((f > best[i]) if "tie_high" in faults else (f < best[i]))):
                best[i], best_d2[i] = f, d2
            max_ring = max(max_ring, r)
            rr = r + 1 if "stop_early" in faults else r
            open_, lb = False, np.inf
            for k in range(3):
                blo, bhi = c[k] - rr, c[k] + rr
                if "reached_side" in faults:                     # the grid's own edge counted as a side faces may lie beyond
                    blo, bhi = max(blo, 0), min(bhi, n[k] - 1)
                if c[k] - r > 0 or "reached_side" in faults:
                    lb = min(lb, ((p[i, k] - (origin[k] + float(blo) * cell[k])) - slack[k]) * SHRINK)
                    open_ = open_ or c[k] - r > 0
                if c[k] + r < n[k] - 1 or "reached_side" in faults:
                    lb = min(lb, (((origin[k] + float(bhi + 1) * cell[k]) - p[i, k]) - slack[k]) * SHRINK)
                    open_ = open_ or c[k] + r < n[k] - 1
            if not open_:
                break
            if lb > 0 and ((best_d2[i] <= lb * lb if "stop_le" in faults else best_d2[i] < lb * lb) or lb > max_distance):
                break
            r += 1
    out = _finish(points, verts, faces, best, best_d2, max_distance, faults)
    out["counts"] = {"degenerate_faces": 0 if "keep_degenerate" in faults else n_deg, "non_finite_queries": int((~finite).sum()),
                     "candidate_tests": tests, "max_ring": max_ring}
    return out


# ---- the comparison the GPU tests use ---------------------------------------------------------------------------------------------------
def _same(g, w):
    g, w = np.asarray(g), np.asarray(w)
    if g.dtype != w.dtype or g.shape != w.shape:
        return False
    if g.dtype.kind != "f":
        return np.array_equal(g, w)
    bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    return bool(((np.ascontiguousarray(g).view(bits) == np.ascontiguousarray(w).view(bits)) | (np.isnan(g) & np.isnan(w))).all())


def mismatches(got, want, counters=COUNTERS):
    """The keys of ``got`` (closest_points' dict with its tensors on the host, or one of the restatements') that are not ``want``'s in
    dtype, shape or any bit (a NaN equals a NaN), and the counters that differ."""
    types = {"distance": np.float32, "d2": np.float64, "face": np.int32, "closest": np.float32, "bary": np.float32}
    bad = [k for k, dt in types.items() if np.asarray(got[k]).dtype != dt or not _same(got[k], want[k])]
    return bad + [k for k in counters if int(got["counts"][k]) != int(want["counts"][k])]


# ---- the quadrature ---------------------------------------------------------------------------------------------------------------------
_sub = {}


def subdivision(k, transposed=False):
    """[k^2, 2] the numerators (nv, nw) over 3 k of the centroids of the regular subdivision, in the header's order."""
    if (k, transposed) not in _sub:
        rows = []
        for i in range(k):
            for j in range(k - i):
                rows.append((3 * i + 1, 3 * j + 1))
                if j < k - 1 - i:
                    rows.append((3 * i + 2, 3 * j + 2))
        t = np.array(rows, dtype=np.int64).reshape(-1, 2)
        _sub[k, transposed] = t[:, ::-1].copy() if transposed else t
    return _sub[k, transposed]


def sample_faces(verts, faces, spacing, max_subdiv=64, faults=()):
    """(points [S,3] float32, face_of [S] int32, weight [S] float64, area [F], k [F]) as mesh.sample_faces computes them."""
    v = widen(verts).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n, dead = zero_normal(a, b, c)
    area = np.where(dead, 0.0, 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]))
    ab, ac, bc = b - a, c - a, c - b
    l2 = _dot(ab, ab)
    l2ac, l2bc = _dot(ac, ac), _dot(bc, bc)
    l2 = np.where(l2ac > l2, l2ac, l2)
    l2 = np.where(l2bc > l2, l2bc, l2)
    t = np.ceil(np.sqrt(l2) / float(spacing))
    k = np.where(dead, 0, np.where(t >= 1, np.where(t < max_subdiv, t, max_subdiv), 1)).astype(np.int32)
    pts, face_of, weight = [], [], []
    for i in np.flatnonzero(k > 0):
        ki = int(k[i])
        nvw = subdivision(ki, "order_transposed" in faults)
        nv, nw = nvw[:, 0].astype(np.float64), nvw[:, 1].astype(np.float64)
        nu = (3 * ki - nvw[:, 0] - nvw[:, 1]).astype(np.float64)
        pts.append((((nu[:, None] * a[i] + nv[:, None] * b[i]) + nw[:, None] * c[i]) / float(3 * ki)).astype(np.float32))
        face_of.append(np.full(ki * ki, i, dtype=np.int32))
        weight.append(np.full(ki * ki, area[i] if "weights_no_k2" in faults else area[i] / float(ki * ki)))
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dtype=dt)
    return cat(pts, (0, 3), np.float32), cat(face_of, (0,), np.int32), cat(weight, (0,), np.float64), area, k


def sample_mismatches(got, want):
    """Indices of (points, face_of, weight) that differ from the restatement's in dtype, shape or any bit."""
    return [i for i in range(3) if not _same(got[i], want[i])]


# ---- the metric -------------------------------------------------------------------------------------------------------------------------
def stats(d, weight, found):
    nan = float("nan")
    out = {"mean": nan, "rms": nan, "max": nan, "p50": nan, "p95": nan}
    d, weight = d[found], weight[found]
    if len(d):
        out["max"] = float(d.max())
    keep = weight > 0
    d, weight = d[keep], weight[keep]
    total = weight.sum()
    if len(d) and total > 0:
        out["mean"] = float((weight * d).sum() / total)
        out["rms"] = float(np.sqrt((weight * (d * d)).sum() / total))
        by = np.argsort(d, kind="stable")
        cum = np.cumsum(weight[by])
        for name, q in (("p50", 0.5), ("p95", 0.95)):
            out[name] = float(d[by][min(int(np.searchsorted(cum, q * total)), len(d) - 1)])
    return out


def surface_distance(verts_a, faces_a, verts_b, faces_b, spacing, max_distance=np.inf, vertices=True, faults=()):
    out = {}
    for name, (va, fa, vb, fb) in (("a_to_b", (verts_a, faces_a, verts_b, faces_b)), ("b_to_a", (verts_b, faces_b, verts_a, faces_a))):
        pts, _, weight, _, _ = sample_faces(va, fa, spacing, faults=faults)
        if vertices and len(fa):
            ref = np.zeros(len(va), dtype=bool)
            ref[np.asarray(fa, dtype=np.int64).reshape(-1)] = True
            extra = np.asarray(va, dtype=np.float32)[ref]
            pts, weight = np.concatenate([pts, extra]), np.concatenate([weight, np.zeros(len(extra))])
        res = brute_force(pts, vb, fb, max_distance, faults)
        found = res["face"] >= 0
        with np.errstate(all="ignore"):
            st = stats(np.sqrt(res["d2"]), weight, found)
        st["n_samples"], st["n_beyond"] = len(pts), int((~found).sum()) - res["counts"]["non_finite_queries"]
        out[name] = st
    out["hausdorff"] = max(out["a_to_b"]["max"], out["b_to_a"]["max"])
    out["chamfer"] = out["a_to_b"]["mean"] + out["b_to_a"]["mean"]
    return out


# ---- checkers that share nothing with the restatement -----------------------------------------------------------------------------------
def lattice(m):
    """Barycentric lattice points [(m + 1)(m + 2) / 2, 3] of denominator m, as long doubles."""
    i, j = np.meshgrid(np.arange(m + 1), np.arange(m + 1), indexing="ij")
    keep = i + j <= m
    i, j = i[keep].astype(np.longdouble), j[keep].astype(np.longdouble)
    return np.stack([(m - i - j) / m, i / m, j / m], -1)


def optimality_violations(points, verts, faces, res, queries, m=8):
    """How many of ``queries`` (indices) have some barycentric lattice point, on the winning or on any other non-degenerate triangle, that
    is closer than the reported d2 by more than rounding (2^-44 of the squared scale of the coordinates), or whose reported closest point is
    farther from the query than sqrt(d2) says, in long double."""
    L = np.longdouble
    p, v = np.asarray(points, dtype=np.float32).astype(L), np.asarray(verts, dtype=np.float32).astype(L)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lam = lattice(m)
    tri = np.einsum("lk,fkx->flx", lam, v[f])                        # [F, lattice, 3]
    scale2 = (1 + max(np.abs(p[np.isfinite(p).all(1)]).max(), np.abs(v).max())) ** 2
    tol = L(2.0 ** -44) * scale2
    bad = 0
    for i in queries:
        if res["face"][i] < 0:
            continue
        d2 = ((tri - p[i]) ** 2).sum(-1)
        own = ((np.asarray(res["closest"][i]).astype(L) - p[i]) ** 2).sum()
        # the reported point is the fp32 rounding of the fp64 one: 2^-23 relative on each coordinate
        slack = 4 * np.sqrt(L(res["d2"][i])) * L(2.0 ** -23) * np.sqrt(scale2) + L(2.0 ** -44) * scale2
        bad += bool(d2.min() < L(res["d2"][i]) - tol) or bool(abs(own - L(res["d2"][i])) > slack)
    return bad


def barycentric_violations(verts, faces, res):
    """How many hits break bary >= 0, sum bary = 1 or closest = sum bary v, each within the rounding of fp32 outputs."""
    v = widen(verts)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    hit = res["face"] >= 0
    br, q = res["bary"][hit].astype(np.float64), res["closest"][hit].astype(np.float64)
    t = v[f[res["face"][hit]]]
    scale = 1 + np.abs(v).max()
    bad = (br < -2.0 ** -40).any(1) | (np.abs(br.sum(1) - 1) > 3 * 2.0 ** -24)
    bad |= (np.abs(np.einsum("nk,nkx->nx", br, t) - q) > 4 * 2.0 ** -23 * scale).any(1)
    return int(bad.sum())


# ---- test meshes ------------------------------------------------------------------------------------------------------------------------
def square(n, z=0.0, shift=(0.0, 0.0)):
    """The unit square [0,1]^2 at height z cut into n x n cells of two triangles; (verts float32, faces int32)."""
    g = np.arange(n + 1, dtype=np.float64) / n
    x, y = np.meshgrid(g + shift[0], g + shift[1], indexing="ij")
    verts = np.stack([x, y, np.full_like(x, z)], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v00 = (i * (n + 1) + j).reshape(-1)
    v10, v01, v11 = v00 + (n + 1), v00 + 1, v00 + (n + 2)
    faces = np.concatenate([np.stack([v00, v10, v11], 1), np.stack([v00, v11, v01], 1)]).astype(np.int32)
    return verts, faces


def with_degenerates(verts, faces):
    """The mesh with two degenerate faces in FRONT (so that one that is kept wins its ties): (i, i, j) on the vertices of face 0, and three
    new, exactly collinear vertices floating at y = 1.25.  Returns (verts, faces, the index of vertex i)."""
    verts, faces = np.asarray(verts, dtype=np.float32), np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V = len(verts)
    line = np.array([(0.0, 1.25, 0.0), (0.25, 1.25, 0.0), (0.5, 1.25, 0.0)], dtype=np.float32)
    i, j = int(faces[0, 0]), int(faces[0, 1])
    return np.concatenate([verts, line]), np.concatenate([np.array([(i, i, j), (V, V + 1, V + 2)], dtype=np.int32), faces]), i


def strict_case():
    """(verts, faces, query, n): the box (0, 4)^3 in 4 cells of exactly 1 per axis; face 0 lies in the plane x = 3 (cell 3), face 1 in the
    plane x = 2 (cell 2), and the query (2.5, 2.5, 2.5) of cell 2 is exactly 0.5 from both.  Ring 0 sees face 1 only and the bound without
    slack is exactly 0.5: a stop at <= keeps face 1, the strict stop walks on and finds the lower index."""
    tri = lambda x: [(x, 2.25, 2.25), (x, 2.9, 2.25), (x, 2.25, 2.9)]
    verts = np.array(tri(3.0) + tri(2.0) + [(0, 0, 0), (0.1, 0, 0), (0, 0.1, 0), (4, 4, 4), (3.9, 4, 4), (4, 3.9, 4)], dtype=np.float32)
    return verts, np.arange(12, dtype=np.int32).reshape(4, 3), np.array([(2.5, 2.5, 2.5)], dtype=np.float32), 4


def sample_mesh():
    """Faces with k = 1, 2, max_subdiv exactly, one clipped by max_subdiv, and a degenerate one (spacing 0.25, max_subdiv 8)."""
    verts = np.array([(0, 0, 0), (0.25, 0, 0), (0, 0.2, 0),        # longest edge 0.32: k = 2;  with the next: 0.25 -> k = 1
                      (0, 0, 1), (0.25, 0, 1), (0, 0.125, 1),
                      (0, 0, 2), (2.0, 0, 2), (0, 1.5, 2),         # 2.5 / 0.25 = 10 -> clipped to 8
                      (0, 0, 3), (1.875, 0, 3), (0, 0.5, 3),       # 1.94 / 0.25 -> 8 exactly
                      (5, 5, 5), (6, 6, 6), (7, 7, 7)], dtype=np.float32)
    return verts, np.arange(15, dtype=np.int32).reshape(5, 3)


CASES = (("sphere", (24, 32, 20)), ("two_spheres", (33, 16, 18)), ("torus", (28, 22, 13)))      # cc.FIELDS at reduced lattices
PLANE_GRID = 7                                                                                 # the grid whose cell planes carry queries
_cases = {}


def case(name):
    """(verts, faces, queries, index of the vertex the degenerate face 0 sits on) of one of CASES: mt_reference's field at level 0 on
    (-1, 1)^3 with two degenerate faces in front, and queries_for it (the vertex of the degenerate face among them)."""
    if name not in _cases:
        import cc_reference as cc
        verts, faces, _, _ = cc.field_mesh(name, dict(CASES)[name])
        verts, faces, i = with_degenerates(verts, faces)
        q = queries_for(verts, faces, PLANE_GRID, seed=len(name))
        _cases[name] = (verts, faces, np.concatenate([verts[i:i + 1], np.array([(0.3, 1.2, 0.05)], dtype=np.float32), q]), i)
    return _cases[name]


def queries_for(verts, faces, n_grid, seed=0, n_random=400, n_each=150):
    """The query set of the tests: random points in (-1.3, 1.3)^3, the mesh's own vertices, face centroids, points on the cell planes of the
    grid ``n_grid`` and points at 10 times the box size; float32 [N,3]."""
    rng = np.random.default_rng(seed)
    v = np.asarray(verts, dtype=np.float32)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    origin, cell, _, n = grid_of(v, n_grid)
    hi = origin + n * cell
    parts = [rng.uniform(-1.3, 1.3, (n_random, 3)), v[rng.choice(len(v), min(n_each, len(v)), replace=False)],
             widen(v)[f[rng.choice(len(f), min(n_each, len(f)), replace=False)]].mean(1)]
    planes = rng.uniform(origin - 0.2, hi + 0.2, (n_each, 3))
    for i in range(n_each):                                          # one, two or three coordinates exactly on a cell plane
        for k in rng.choice(3, 1 + i % 3, replace=False):
            planes[i, k] = origin[k] + float(rng.integers(0, n[k] + 1)) * cell[k]
    parts.append(planes)
    d = rng.standard_normal((n_each // 3, 3))
    parts.append((origin + hi) / 2 + 10 * (hi - origin).max() * d / np.linalg.norm(d, axis=1, keepdims=True))
    return np.concatenate(parts).astype(np.float32)

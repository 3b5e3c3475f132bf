"""NumPy restatement of the mesh ray casting (include/mofanerf_hip.h, mofa_ray_query; mofanerf_amd.mesh.ray_cast / ray_bounds): the
watertight ray-triangle arithmetic of Woop, Benthin and Wald operation by operation in float64 on the float32 inputs widened, the box
rule, brute-force selection over all faces, the slab walk over dist_reference's grid and binning with its termination bound and
counters, and the per-ray bounds.  Test code, not product.  ``mismatches`` is THE comparison: the GPU tests assert it returns nothing,
tests/test_ray_reference_cpu.py shows that it sees every injected fault (``faults``: a set of the names in FAULTS)."""
import numpy as np

import dist_reference as dr
import wind_reference as wr

FAULTS = ("no_swap", "zeros_outside", "no_clamp", "tie_high", "tmax_exclusive", "no_slack", "stop_first_hit", "centroid_binning",
          "last_as_first", "cull_swapped", "no_box_rule")
COUNTERS = ("bad_rays", "degenerate_faces")                              # the counters no grid changes
WALK_COUNTERS = COUNTERS + ("face_tests", "max_slabs", "off_box")        # and those of one grid's walk
WHICH = ("first", "last")
CULL = (None, "back", "front")
TOL = 2.0 ** -42          # the box rule's tolerance, times the pair's scale
SLACK = 2.0 ** -40        # the walk's slack, times the ray's scale


def widen(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def ray_axes(d, faults=()):
    """(kz, kx, ky) [N] of directions d [N,3] (float64): kz the axis of the largest |d| (a tie: the lowest), kx / ky the next two, swapped
    where d[kz] < 0."""
    ad = np.abs(d)
    kz = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    neg = np.take_along_axis(d, kz[:, None], 1)[:, 0] < 0
    if "no_swap" not in faults:
        kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    return kz, kx, ky


def bad_rays(o, d):
    return ~(np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1))


def _ax(x, k):
    """x [..., 3] at the per-ray axis k [N] (x's leading dimension is N, possibly followed by F)."""
    if x.ndim == 2:
        return np.take_along_axis(x, k[:, None], 1)[:, 0]
    return np.take_along_axis(x, k[:, None, None], 2)[..., 0]


def pair_arith(o, d, a, b, c, faults=()):
    """The header's per-pair arithmetic.  o, d [N,3]; a, b, c [N,3] (one face per ray) or [N,F,3].  A dict of arrays [N] or [N,F]:
    ``sign`` (int8: +1 det > 0, -1 det < 0, 0 a miss by the edge functions or det == 0), ``t`` (clamped), ``off`` (the box rule
    refuses the pair), ``bary`` and ``point`` [...,3]."""
    with np.errstate(all="ignore"):
        kz, kx, ky = ray_axes(d, faults)
        dz = _ax(d, kz)
        Sx, Sy, Sz = _ax(d, kx) / dz, _ax(d, ky) / dz, 1.0 / dz
        ex = (lambda v: v[:, None]) if a.ndim == 3 else (lambda v: v)
        oo = o[:, None, :] if a.ndim == 3 else o
        dd = d[:, None, :] if a.ndim == 3 else d

        def shear(X):
            Xp = X - oo
            xz = _ax(Xp, kz)
            return _ax(Xp, kx) - ex(Sx) * xz, _ax(Xp, ky) - ex(Sy) * xz, ex(Sz) * xz

        Ax, Ay, Az = shear(a)
        Bx, By, Bz = shear(b)
        Cx, Cy, Cz = shear(c)
        U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        if "zeros_outside" in faults:
            miss = ~(((U > 0) & (V > 0) & (W > 0)) | ((U < 0) & (V < 0) & (W < 0)))
        else:
            miss = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        miss = miss | (det == 0) | np.isnan(det)
        t = ((U * Az + V * Bz) + W * Cz) / det
        zlo, zhi = np.where(Az < Bz, Az, Bz), np.where(Az > Bz, Az, Bz)
        zlo, zhi = np.where(Cz < zlo, Cz, zlo), np.where(Cz > zhi, Cz, zhi)
        if "no_clamp" not in faults:
            t = np.where(t < zlo, zlo, t)
            t = np.where(t > zhi, zhi, t)
        point = oo + t[..., None] * dd
        lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
        m = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.abs(c))
        ao = np.abs(o)
        scale = ex((ao[:, 0] + ao[:, 1]) + ao[:, 2]) + ((m[..., 0] + m[..., 1]) + m[..., 2])
        tol = (TOL * scale)[..., None]
        off = ~miss & ((point < lo - tol) | (point > hi + tol) | np.isnan(point)).any(-1)
        if "no_box_rule" in faults:
            off = np.zeros_like(off)
        sign = np.where(miss, 0, np.where(det > 0, 1, -1)).astype(np.int8)
        return {"sign": sign, "t": t, "off": off, "bary": np.stack([U / det, V / det, W / det], -1), "point": point}


def pair_table(origins, dirs, verts, faces, faults=(), chunk=1 << 19):
    """(T [N,F] float64, S [N,F] int8, OFF [N,F] bool, degenerate count): every ray against every face.  S is 0 for a miss, for a
    degenerate face and for a bad ray; OFF marks the pairs the box rule refuses (their S is 0 too)."""
    o, d, v = widen(origins).reshape(-1, 3), widen(dirs).reshape(-1, 3), widen(verts).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    N, F = len(o), len(f)
    T, S, OFF = np.full((N, F), np.nan), np.zeros((N, F), dtype=np.int8), np.zeros((N, F), dtype=bool)
    if F == 0:
        return T, S, OFF, 0
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    dead = dr.zero_normal(a, b, c)[1]
    good = ~bad_rays(o, d)
    rows = max(1, chunk // F)
    for i in range(0, N, rows):
        p = pair_arith(o[i:i + rows], d[i:i + rows], a[None], b[None], c[None], faults)
        keep = good[i:i + rows, None] & ~dead[None]
        OFF[i:i + rows] = p["off"] & keep
        S[i:i + rows] = np.where(keep & ~p["off"], p["sign"], 0)
        T[i:i + rows] = p["t"]
    return T, S, OFF, int(dead.sum())


def accepted(table, t_min, t_max, cull, faults=()):
    """[N,F] bool: the pairs that are hits inside the window and on the wanted side."""
    T, S = table[0], table[1]
    with np.errstate(all="ignore"):
        ok = (S != 0) & (T >= t_min) & ((T < t_max) if "tmax_exclusive" in faults else (T <= t_max))
    if "cull_swapped" in faults and cull is not None:
        cull = "front" if cull == "back" else "back"
    if cull == "back":
        ok &= S > 0
    elif cull == "front":
        ok &= S < 0
    return ok


def _pick(t_row, ok_row, ids, which, faults):
    """(face, t) among the candidate faces ``ids`` of one ray: the smaller (``last``: the larger) t, then the lower index."""
    ids = ids[ok_row[ids]]
    if len(ids) == 0:
        return -1, np.nan
    t = t_row[ids]
    m = t.max() if which == "last" else t.min()
    tied = ids[t == m]
    return int(tied.max() if "tie_high" in faults else tied.min()), float(t_row[tied.max() if "tie_high" in faults else tied.min()])


def _finish(origins, dirs, verts, faces, best, faults):
    o, d, v = widen(origins).reshape(-1, 3), widen(dirs).reshape(-1, 3), widen(verts).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    N = len(o)
    bad, hit = bad_rays(o, d), best >= 0
    t64 = np.where(bad, np.nan, np.inf)
    bary, point, front = np.full((N, 3), np.nan), np.full((N, 3), np.nan), np.zeros(N, dtype=bool)
    if hit.any():
        tri = f[best[hit]]
        p = pair_arith(o[hit], d[hit], v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]], faults)
        t64[hit], bary[hit], point[hit], front[hit] = p["t"], p["bary"], p["point"], p["sign"] > 0
    with np.errstate(all="ignore"):
        return {"t": t64.astype(np.float32), "t64": t64, "face": best.astype(np.int32), "hit": hit, "front": front,
                "bary": bary.astype(np.float32), "point": point.astype(np.float32)}


def _which(which, faults):
    if which not in WHICH:
        raise ValueError(which)
    return "first" if "last_as_first" in faults else which


def brute_force(origins, dirs, verts, faces, t_min=0.0, t_max=np.inf, which="first", cull=None, faults=(), table=None):
    """What mesh.ray_cast returns (NumPy arrays, ``counts`` with the grid-independent counters) from all N x F pairs."""
    which = _which(which, faults)
    table = table if table is not None else pair_table(origins, dirs, verts, faces, faults)
    ok = accepted(table, t_min, t_max, cull, faults)
    N, F = ok.shape
    best = np.full(N, -1, dtype=np.int64)
    if F:
        key = np.where(ok, table[0], -np.inf if which == "last" else np.inf)
        key = -key if which == "last" else key
        arg = (F - 1 - np.argmin(key[:, ::-1], 1)) if "tie_high" in faults else np.argmin(key, 1)
        best = np.where(ok.any(1), arg, -1)
    out = _finish(origins, dirs, verts, faces, best, faults)
    out["counts"] = {"bad_rays": int(bad_rays(widen(origins).reshape(-1, 3), widen(dirs).reshape(-1, 3)).sum()), "degenerate_faces": table[3]}
    return out


def grid_walk(origins, dirs, verts, faces, n, t_min=0.0, t_max=np.inf, which="first", cull=None, faults=(), table=None):
    """What mesh.ray_cast returns at grid ``n``, by the kernel's walk: the slabs of cells along kz in ray order (``last``: reversed), in
    each the index rectangle of the ray's footprint widened by the slack, and the stop at the slab whose parameter range lies strictly
    beyond the best hit.  ``counts`` also holds ``face_tests``, ``max_slabs`` and ``off_box``.  The pair arithmetic comes from pair_table (a
    function of the pair alone)."""
    which = _which(which, faults)
    table = table if table is not None else pair_table(origins, dirs, verts, faces, faults)
    ok = accepted(table, t_min, t_max, cull, faults)
    T, OFF = table[0], table[2]
    o, d = widen(origins).reshape(-1, 3), widen(dirs).reshape(-1, 3)
    grid = dr.grid_of(verts, n)
    origin, cell, slack, n = grid
    start, pair_face, _ = dr.bin_faces(verts, faces, grid, faults)
    N = len(o)
    best = np.full(N, -1, dtype=np.int64)
    tests = off_box = max_slabs = 0
    good = ~bad_rays(o, d)
    kzs, kxs, kys = ray_axes(np.where(good[:, None], d, 1.0), faults)
    top = origin + n.astype(np.float64) * cell
    M = np.maximum(np.abs(origin), np.abs(top))
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(good):
            kz, kx, ky = int(kzs[i]), int(kxs[i]), int(kys[i])
            Sz = 1.0 / d[i, kz]
            ao = np.abs(o[i])
            R = ((ao[0] + ao[1]) + ao[2]) + ((M[0] + M[1]) + M[2])
            s = np.zeros(3) if "no_slack" in faults else slack + SLACK * R
            Wt = abs(Sz) * s[kz]
            forward = (Sz > 0) == (which == "first")
            bf, bt, slabs = -1, np.nan, 0
            for step in range(int(n[kz])):
                j = step if forward else int(n[kz]) - 1 - step
                plo, phi = origin[kz] + float(j) * cell[kz], origin[kz] + float(j + 1) * cell[kz]
                e, x = ((plo - o[i, kz]) * Sz, (phi - o[i, kz]) * Sz) if Sz > 0 else ((phi - o[i, kz]) * Sz, (plo - o[i, kz]) * Sz)
                lo_t, hi_t = e - Wt, x + Wt
                if which == "first":
                    if (bf >= 0 and bt < lo_t) or lo_t > t_max:
                        break
                else:
                    if (bf >= 0 and bt > hi_t) or hi_t < t_min:
                        break
                ta, tb = max(lo_t, t_min), min(hi_t, t_max)
                if not ta <= tb:
                    continue
                slabs += 1
                r = {}
                for k in (kx, ky):
                    pa, pb = o[i, k] + ta * d[i, k], o[i, k] + tb * d[i, k]
                    r[k] = (int(dr.cell_index(min(pa, pb) - s[k], origin[k], cell[k], n[k])), int(dr.cell_index(max(pa, pb) + s[k], origin[k], cell[k], n[k])))
                r[kz] = (j, j)
                gx, gy, gz = np.meshgrid(*(np.arange(r[k][0], r[k][1] + 1) for k in range(3)), indexing="ij")
                cid = ((gx * n[1] + gy) * n[2] + gz).reshape(-1)
                ids = np.concatenate([pair_face[start[k]:start[k + 1]] for k in cid]) if len(cid) else np.zeros(0, dtype=np.int64)
                tests += len(ids)
                off_box += int(OFF[i, ids].sum())
                f, t = _pick(T[i], ok[i], ids, which, faults)
                if f >= 0 and (bf < 0 or (t > bt if which == "last" else t < bt) or (t == bt and ((f > bf) if "tie_high" in faults else (f < bf)))):
                    bf, bt = f, t
                if bf >= 0 and "stop_first_hit" in faults:
                    break
            best[i] = bf
            max_slabs = max(max_slabs, slabs)
    out = _finish(origins, dirs, verts, faces, best, faults)
    out["counts"] = {"bad_rays": int((~good).sum()), "degenerate_faces": table[3], "face_tests": tests, "max_slabs": max_slabs, "off_box": off_box}
    return out


def ray_bounds(origins, dirs, verts, faces, near, far, margin, faults=(), table=None):
    """What mesh.ray_bounds returns: float32 arithmetic on the float32 ``t`` of a first and a last cast over [near, far]."""
    table = table if table is not None else pair_table(origins, dirs, verts, faces, faults)
    first = brute_force(origins, dirs, verts, faces, near, far, "first", None, faults, table)
    last = brute_force(origins, dirs, verts, faces, near, far, "last", None, faults, table)
    n32, f32, m32 = np.float32(near), np.float32(far), np.float32(margin)
    hit = first["hit"]
    with np.errstate(all="ignore"):
        lo = np.where(hit, np.maximum(first["t"] - m32, n32), n32).astype(np.float32)
        hi = np.where(hit, np.minimum(last["t"] + m32, f32), f32).astype(np.float32)
    return {"near": lo, "far": hi, "hit": hit}


# ---- the comparison the GPU tests use ---------------------------------------------------------------------------------------------------
TYPES = {"t": np.float32, "t64": np.float64, "face": np.int32, "hit": np.bool_, "front": np.bool_, "bary": np.float32, "point": np.float32}


def mismatches(got, want, counters=COUNTERS):
    """The keys of ``got`` (ray_cast's dict with its tensors on the host, or one of the restatements') that are not ``want``'s in dtype,
    shape or any bit (a NaN equals a NaN), and the counters that differ."""
    bad = [k for k, dt in TYPES.items() if np.asarray(got[k]).dtype != dt or not dr._same(got[k], want[k])]
    return bad + [k for k in counters if int(got["counts"][k]) != int(want["counts"][k])]


def bounds_mismatches(got, want):
    return [k for k, dt in (("near", np.float32), ("far", np.float32), ("hit", np.bool_))
            if np.asarray(got[k]).dtype != dt or not dr._same(got[k], want[k])]


# ---- the catalogue of ray sets ----------------------------------------------------------------------------------------------------------
FIELD_CASES = tuple(name for name, _ in dr.CASES)
AIMED = {"sphere": 1001, "torus": 399, "two_spheres": 401}
AXIS_RAYS = {"sphere": 63, "torus": 65, "two_spheres": 130}
_cache = {}


def cube_axis_rays():
    """(origins, dirs, inside [N]) the rays from 2 before the unit cube along all six +-axis directions over CUBE_LATTICE^2; ``inside``:
    the ray meets the cube (0 <= the other two coordinates <= 1, edges and corners included)."""
    g = np.array(wr.CUBE_LATTICE, dtype=np.float32)
    u, v = (x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij"))
    os_, ds = [], []
    for a in range(3):
        for sgn in (1.0, -1.0):
            o = np.zeros((len(u), 3), dtype=np.float32)
            o[:, (a + 1) % 3], o[:, (a + 2) % 3], o[:, a] = u, v, -2.0 if sgn > 0 else 3.0
            d = np.zeros_like(o)
            d[:, a] = sgn
            os_.append(o), ds.append(d)
    inside = np.tile((u >= 0) & (u <= 1) & (v >= 0) & (v <= 1), 6)
    return np.concatenate(os_), np.concatenate(ds), inside


def _cube_diagonals():
    o, d = [], []
    for c in np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64):       # through two opposite corners
        u = 2 * c - 1
        o.append(c + 2 * u), d.append(-0.5 * u)
    for a in range(3):                                                                                     # through the midpoints of two opposite edges
        for su in (0, 1):
            for sv in (0, 1):
                m = np.full(3, 0.5)
                m[(a + 1) % 3], m[(a + 2) % 3] = su, sv
                u = 2 * m - 1
                u[a] = 0
                o.append(m + 2 * u), d.append(-3.0 * u)
    for z in (0.0, 0.25, 1.0):                                                                             # along the diagonal of a face, through an edge
        o.append(np.array([-1.0, -1.0, z])), d.append(np.array([1.0, 1.0, 0.0]))
        o.append(np.array([-1.0, 2.0, z])), d.append(np.array([2.0, -2.0, 0.0]))
    o.append(np.array([-1.0, 0.5, -0.25])), d.append(np.array([4.0, 0.0, 1.0]))                            # oblique, through the -x face
    o.append(np.array([0.1, 0.5, -1.0])), d.append(np.array([0.1, 0.0, 1.0]))
    return np.array(o, dtype=np.float32), np.array(d, dtype=np.float32)


def _cube_surface():
    o = [(0.5, 0.5, 0.0), (0.5, 0.5, 1.0), (0.5, 0.5, 1.0), (0.25, 0.0, 0.25), (0.5, 0.5, 2.0), (0.5, 0.5, -1.0), (2.0, 0.5, 0.5), (0.0, 0.0, 0.0)]
    d = [(0, 0, 1), (0, 0, 1), (0, 0, -1), (0.5, 1, 0.25), (0, 0, 1), (0, 0, -1), (1, 0.25, 0), (1, 1, 1)]
    rng = np.random.default_rng(5)
    inside = rng.uniform(0.05, 0.95, (40, 3))
    o, d = np.array(o, dtype=np.float64), np.array(d, dtype=np.float64)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    return (np.concatenate([o, np.repeat(np.array([[0.5, 0.5, 0.5]]), 6, 0), inside]).astype(np.float32),
            np.concatenate([d, axes, rng.standard_normal((40, 3)) * rng.uniform(0.1, 10, (40, 1))]).astype(np.float32))


def _cube_random_axis(n=83, seed=11):
    """Axis rays at random offsets: the three depths of a face are equal, and the quotient's rounding is what the clamp removes."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.2, 1.2, (n, 3))
    a = rng.integers(0, 3, n)
    sgn = rng.choice([-1.0, 1.0], n)
    d = np.zeros((n, 3))
    d[np.arange(n), a] = sgn * rng.uniform(0.3, 3.0, n)
    o[np.arange(n), a] = np.where(sgn > 0, -rng.uniform(1, 3, n), 1 + rng.uniform(1, 3, n))
    return o.astype(np.float32), d.astype(np.float32)


def aimed_rays(verts, n, seed):
    """Origins on the sphere of two box diagonals around the box centre, directions toward uniformly drawn points of the box, un-normalised."""
    rng = np.random.default_rng(seed)
    v = widen(verts)
    lo, hi = v.min(0), v.max(0)
    centre, diag = (lo + hi) / 2, np.linalg.norm(hi - lo)
    u = rng.standard_normal((n, 3))
    o = centre + 2 * diag * u / np.linalg.norm(u, axis=1, keepdims=True)
    target = rng.uniform(lo, hi, (n, 3))
    return o.astype(np.float32), ((target - o) * rng.uniform(0.2, 3.0, (n, 1))).astype(np.float32)


def lattice_axis_rays(name, n):
    """Rays from the extraction's own lattice points (wind_reference.field_case) along +-axes: through mesh vertices and along edges."""
    _, _, q, _ = wr.field_case(name)
    q = q[::len(q) // n][:n]
    d = np.zeros((len(q), 3), dtype=np.float32)
    k = np.arange(len(q))
    d[k, k % 3] = np.where((k // 3) % 2 == 0, 1.0, -1.0)
    return q.astype(np.float32), d


def slanted():
    """A cube (0.25, 0.75)^3 and one large slanted face behind it whose index box is the whole grid: the far face is met in the first slab."""
    v, f = wr.cube(0.25, 0.75)
    big = np.array([(-6.5, -5.0, -1.6), (7.5, -5.0, 5.4), (0.5, 8.0, 1.9)], dtype=np.float32)
    return wr.merged((v, f), (big, np.array([(0, 1, 2)], dtype=np.int32)))


def specks(scale=2.0 ** -55, n_faces=800, n_rays=61):
    """The unit cube with a cloud of faces of size ``scale`` at its corner (0, 0, 0), and rays that pass the cloud at up to 0.4: for a ray
    that far from a face that small the edge functions are rounding noise, their signs agree now and then, and the box rule is what
    refuses the pair.  (mesh, rays)"""
    rng = np.random.default_rng(4)
    tri = (rng.uniform(-1, 1, (n_faces, 1, 3)) * scale + rng.uniform(-1, 1, (n_faces, 3, 3)) * scale).astype(np.float32)
    cloud = (tri.reshape(-1, 3), np.arange(3 * n_faces, dtype=np.int32).reshape(n_faces, 3))
    o = np.concatenate([rng.uniform(-0.3, 0.3, (n_rays, 2)), np.full((n_rays, 1), -2.0)], 1)
    d = np.concatenate([rng.uniform(-0.05, 0.05, (n_rays, 2)), np.ones((n_rays, 1))], 1) * rng.uniform(0.5, 2, (n_rays, 1))
    return wr.merged(wr.cube(), cloud), (o.astype(np.float32), d.astype(np.float32))


def catalogue():
    """The ray sets of the tests: a list of dicts ``name, verts, faces, origins, dirs, t_min, t_max``."""
    if "catalogue" in _cache:
        return _cache["catalogue"]
    out = []

    def add(name, mesh, rays, t_min=0.0, t_max=np.inf):
        out.append({"name": name, "verts": np.asarray(mesh[0], dtype=np.float32), "faces": np.asarray(mesh[1], dtype=np.int32),
                    "origins": np.asarray(rays[0], dtype=np.float32), "dirs": np.asarray(rays[1], dtype=np.float32), "t_min": t_min, "t_max": t_max})

    cube = wr.cube()
    co, cd, _ = cube_axis_rays()
    add("cube_axes", cube, (co, cd))
    add("cube_diagonals", cube, _cube_diagonals())
    add("cube_surface", cube, _cube_surface())
    add("cube_random_axis", cube, _cube_random_axis())
    for k, (t0, t1) in enumerate(((2.5, 10.0), (0.0, 2.0), (0.0, 1.9990234375), (2.0, 3.0), (3.0, np.inf), (2.25, 2.75))):
        add(f"cube_window{k}", cube, (co[:36], cd[:36]), t0, t1)
    bo, bd = co[:65].copy(), cd[:65].copy()
    bo[3, 1], bo[10, 0], bd[17, 2], bd[20, 0] = np.nan, np.inf, np.nan, -np.inf
    bd[30] = 0.0
    bd[31] = (0.0, -0.0, 0.0)
    add("bad_rays", cube, (bo, bd))
    for name in FIELD_CASES:
        v, f, _, _ = wr.field_case(name)
        add(f"aimed_{name}", (v, f), aimed_rays(v, AIMED[name], seed=len(name)))
        add(f"axes_{name}", (v, f), lattice_axis_rays(name, AXIS_RAYS[name]))
    v, f, _, i = dr.case("sphere")                                                       # two degenerate faces in front
    ao, ad = aimed_rays(v, 62, seed=3)
    extra = np.array([(0.0, 1.25, -3.0), (0.25, 1.25, -3.0), (0.3, 1.25, -3.0)], dtype=np.float32)      # onto the collinear face
    add("degenerate", (v, f), (np.concatenate([ao, extra, v[i:i + 1] - np.float32([0, 0, 3])]), np.concatenate([ad, np.tile(np.float32([0, 0, 1]), (4, 1))])))
    sv, sf, sq, _ = wr.sliver()
    add("sliver", (sv, sf), (np.concatenate([sq, sq, [[1.0, 1.0, 0.0]]]), np.float32([(0, 0, 1), (0, 0, 1), (0, 0, -2), (0, 0, -2), (-1e-3, 0, 1)])))
    add("single", (sv, sf), (sq[:1], np.float32([(0, 0, 0.5)])))
    add("coincident_cubes", wr.merged(cube, cube), (co[:72], cd[:72]))
    add("inward_cube", wr.cube(inward=True), (co[:36], cd[:36]))
    add("slanted", slanted(), (np.float32([(0.5, 0.5, -2.0), (0.5, 0.5, 6.0), (0.3, 0.6, -2.0)]), np.float32([(0, 0, 1), (0, 0, -1), (0.05, 0, 1)])))
    add("specks", *specks())
    _cache["catalogue"] = out
    return out


def table_of(case, faults=()):
    """The pair table of a catalogue member, computed once per set of faults."""
    key = (case["name"], tuple(sorted(faults)))
    if key not in _cache:
        _cache[key] = pair_table(case["origins"], case["dirs"], case["verts"], case["faces"], faults)
    return _cache[key]

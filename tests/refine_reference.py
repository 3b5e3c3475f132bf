"""NumPy float32 restatement of the vertex refinement (include/mofanerf_hip.h, mofa_iso_edge_ids / mofa_edge_* / mofa_fd_*): the same edge
decoding, points, bracket updates, placement and normals, every float32 operation rounded separately and float64 only where the header
says so.  Test code, not product: the GPU output must equal it bit for bit.

``fault=`` turns one line of the arithmetic into a plausible mistake; the CPU tests show that each mistake breaks a bit comparison or
the radial bound on the very inputs the GPU tests use, i.e. that those inputs can tell the kernels from their near misses.
"""
import numpy as np

import mt_reference as mt

F32 = np.float32
NO_STRADDLE, NON_FINITE, REFUSED, ZERO_NORMAL = range(4)          # MOFA_REFINE_* words of `counts`
FAULTS = ("tm_is_tlo", "swap_sides", "pb_interp", "clamp_u", "flip_normal", "h_isotropic")


def inside(s, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(s, dtype=F32) >= F32(level)            # (NaN: False)


def iso_edge_ids(grid, level):
    """The edge id of every vertex of mt.marching_tets(grid, level, ...), in its order (increasing)."""
    ins = inside(grid, level)
    nx, ny, nz = ins.shape
    flags = np.zeros((nx, ny, nz, 7), dtype=bool)
    for d, (dx, dy, dz) in enumerate(mt.DIRS):
        flags[:nx - dx, :ny - dy, :nz - dz, d] = ins[:nx - dx, :ny - dy, :nz - dz] != ins[dx:, dy:, dz:]
    return np.nonzero(flags.reshape(-1))[0].astype(np.int64)


def edge_ends(edge_ids, res):
    """(a [n,3], b [n,3], ok [n]): the lattice indices of each edge's two ends; ok is False for an id outside the grid or an edge leaving it."""
    e = np.asarray(edge_ids, dtype=np.int64)
    nx, ny, nz = (int(v) for v in res)
    ok = (e >= 0) & (e < 7 * nx * ny * nz)
    e = np.where(ok, e, 0)
    idx, d = e // 7, e % 7
    a = np.stack([idx // (ny * nz), (idx // nz) % ny, idx % nz], 1)
    b = a + mt.DIRS[d]
    ok &= (b < np.array([nx, ny, nz])).all(1)
    return a, b, ok


def _coord(lo, step, i):
    return F32(lo) + i.astype(F32) * F32(step)


def _edge_point(a, b, lo, step, t):
    p = np.empty((len(a), 3), dtype=F32)
    for c in range(3):
        pa, pb = _coord(lo[c], step[c], a[:, c]), _coord(lo[c], step[c], b[:, c])
        p[:, c] = pa + t * (pb - pa)
    return p


def bracket_mid(t_lo, t_hi, fault=None):
    return t_lo.copy() if fault == "tm_is_tlo" else F32(0.5) * (t_lo + t_hi)


def edge_points(res, lo, step, edge_ids, t_lo, t_hi, first, n, mode, pts, counts, fault=None):
    """pts[:n] (float32 [>= n, 3], written in place where the edge is one of the grid's) for vertices first .. first+n-1."""
    sl = slice(first, first + n)
    a, b, ok = edge_ends(np.asarray(edge_ids)[sl], res)
    counts[REFUSED] += int((~ok).sum())
    if mode == 2:
        new = _edge_point(a, b, lo, step, bracket_mid(t_lo[sl], t_hi[sl], fault))
    elif mode == 1 and fault == "pb_interp":
        new = _edge_point(a, b, lo, step, np.ones(n, dtype=F32))
    else:
        ends = a if mode == 0 else b
        new = np.stack([_coord(lo[c], step[c], ends[:, c]) for c in range(3)], 1)
    pts[:n][ok] = new[ok]
    return pts


def bracket_init(s_a, s_b, level, counts):
    s_a, s_b = np.asarray(s_a, dtype=F32), np.asarray(s_b, dtype=F32)
    counts[NO_STRADDLE] += int((inside(s_a, level) == inside(s_b, level)).sum())
    counts[NON_FINITE] += int((~np.isfinite(s_a)).sum() + (~np.isfinite(s_b)).sum())
    return np.zeros(len(s_a), dtype=F32), np.ones(len(s_a), dtype=F32), s_a.copy(), s_b.copy()


def bracket_update(s_m, level, t_lo, t_hi, s_lo, s_hi, counts, fault=None):
    """The four bracket arrays after one midpoint (new arrays)."""
    s_m = np.asarray(s_m, dtype=F32)
    fin = np.isfinite(s_m)
    counts[NON_FINITE] += int((~fin).sum())
    t_m = bracket_mid(t_lo, t_hi, fault)
    low = inside(s_m, level) == inside(s_lo, level)
    if fault == "swap_sides":
        low = ~low
    lo_w, hi_w = fin & low, fin & ~low
    return (np.where(lo_w, t_m, t_lo), np.where(hi_w, t_m, t_hi), np.where(lo_w, s_m, s_lo), np.where(hi_w, s_m, s_hi))


def edge_place(res, lo, step, edge_ids, t_lo, t_hi, s_lo, s_hi, level, verts, counts, fault=None):
    a, b, ok = edge_ends(edge_ids, res)
    counts[REFUSED] += int((~ok).sum())
    with np.errstate(all="ignore"):
        u = (F32(level) - s_lo) / (s_hi - s_lo)
        if fault == "clamp_u":
            u = np.clip(u, F32(0), F32(0.5))
        t = t_lo + u * (t_hi - t_lo)
        new = _edge_point(a, b, lo, step, t)
    verts[ok] = new[ok]
    return verts


def fd_points(verts, h, fault=None):
    """[6 n, 3]: v + h_x e_x, v - h_x e_x, then y, then z, per vertex."""
    v = np.asarray(verts, dtype=F32)
    h = np.asarray(h, dtype=F32)
    if fault == "h_isotropic":
        h = np.full(3, h[0], dtype=F32)
    pts = np.repeat(v[:, None, :], 6, 1)
    for c in range(3):
        pts[:, 2 * c, c] = v[:, c] + h[c]
        pts[:, 2 * c + 1, c] = v[:, c] - h[c]
    return pts.reshape(-1, 3)


def fd_normals(s, h, counts, fault=None):
    s = np.asarray(s, dtype=F32).reshape(-1, 6)
    h = np.asarray(h, dtype=F32)
    with np.errstate(all="ignore"):
        g = np.stack([(s[:, 2 * c] - s[:, 2 * c + 1]) / (F32(2) * h[c]) for c in range(3)], 1)
        g64 = g.astype(np.float64)
        norm = np.sqrt(g64[:, 0] * g64[:, 0] + g64[:, 1] * g64[:, 1] + g64[:, 2] * g64[:, 2])
        ok = np.isfinite(g).all(1) & (norm > 0)
        n = (g64 if fault == "flip_normal" else -g64) / norm[:, None]
    counts[ZERO_NORMAL] += int((~ok).sum())
    return np.where(ok[:, None], n, 0.0).astype(F32)


def refine(density_np, edge_ids, res, lo, step, level, iterations, fault=None):
    """mesh.refine_vertices: (verts, (t_lo, t_hi, s_lo, s_hi), counts) with density_np(pts float32 [n,3]) -> float32 [n]."""
    e = np.asarray(edge_ids, dtype=np.int64)
    V = len(e)
    counts = np.zeros(4, dtype=np.int64)
    pts = np.zeros((V, 3), dtype=F32)
    s_a = density_np(edge_points(res, lo, step, e, None, None, 0, V, 0, pts, counts, fault).copy())
    s_b = density_np(edge_points(res, lo, step, e, None, None, 0, V, 1, pts, counts, fault).copy())
    br = bracket_init(s_a, s_b, level, counts)
    for _ in range(iterations):
        s_m = density_np(edge_points(res, lo, step, e, br[0], br[1], 0, V, 2, pts, counts, fault).copy())
        br = bracket_update(s_m, level, *br, counts, fault)
    verts = edge_place(res, lo, step, e, *br, level, np.zeros((V, 3), dtype=F32), counts, fault)
    return verts, br, counts


def density_normals(density_np, verts, step, h_frac=0.5, fault=None):
    h = (F32(h_frac) * np.asarray(step, dtype=F32)).astype(F32)
    counts = np.zeros(4, dtype=np.int64)
    return fd_normals(density_np(fd_points(verts, h, fault)), h, counts, fault), counts


# ---- the sharp ball: sigma(p) = (R / |p - c|)^8 - 1, from +, -, *, / and sqrt only, op by op -------------------------------------------
BALL_R = 0.6
BALL_C = (0.03, -0.02, 0.01)
BALL_GRIDS = ((17, 17, 17), (17, 21, 13))                        # on [-1, 1]^3, level 0


def ball_ops(x, y, z, cx, cy, cz, R, one, sqrt):
    """The field from its coordinates, in whatever array library the arguments live in: every operation a separate, rounded call."""
    dx, dy, dz = x - cx, y - cy, z - cz
    r = sqrt(dx * dx + dy * dy + dz * dz)
    q = R / r
    q2 = q * q
    q4 = q2 * q2
    return q4 * q4 - one


def ball_np(p):
    p = np.asarray(p, dtype=F32)
    with np.errstate(all="ignore"):
        return ball_ops(p[:, 0], p[:, 1], p[:, 2], F32(BALL_C[0]), F32(BALL_C[1]), F32(BALL_C[2]), F32(BALL_R), F32(1), np.sqrt).astype(F32)


def ball_torch(p):
    """The same operations as torch tensors on p's device (float32 constants as tensors, so nothing is computed in another format)."""
    import torch
    k = torch.tensor([*BALL_C, BALL_R, 1.0], dtype=torch.float32, device=p.device)
    return ball_ops(p[:, 0], p[:, 1], p[:, 2], k[0], k[1], k[2], k[3], k[4], torch.sqrt)


def ball_grid(res):
    lo, step = mt.cube_grid(res)
    return ball_np(mt.grid_points(res, lo, step)).reshape(res), lo, step


def radial_error(verts):
    """| |v - c| - R | in float64."""
    v = np.asarray(verts, dtype=np.float64)
    return np.abs(np.linalg.norm(v - np.array(BALL_C, dtype=np.float64), axis=1) - BALL_R)


def radial_bound(edge_ids, res, lo, step, iterations):
    """2^-k |edge| + 8 2^-24 max|coord| per vertex.  A segment whose ends lie on opposite sides of a sphere crosses it once; bisection
    keeps that crossing inside the bracket, the placed vertex lies in the bracket, and r is 1-Lipschitz: the vertex is within the
    bracket's length, 2^-k |edge|, of the sphere.  The second term covers the float32 rounding of the points and of the field's r (a few
    ulp of a coordinate of size <= max|coord|)."""
    a, b, ok = edge_ends(edge_ids, res)
    assert ok.all()
    pa, pb = (np.stack([_coord(lo[c], step[c], q[:, c]) for c in range(3)], 1).astype(np.float64) for q in (a, b))
    return 2.0 ** -iterations * np.linalg.norm(pb - pa, axis=1) + 8 * 2.0 ** -24 * np.maximum(np.abs(pa).max(1), np.abs(pb).max(1))


# measured on the CPU (test_refine_reference_cpu.test_ball_normals_point_radially prints and checks them): the largest angle, in radians,
# between the float64 central-difference direction at h_frac = 0.5 and the radial direction on the refined ball meshes, and between the
# float32 restatement's normals and that float64 direction
FD_ANGLE_F64 = 0.0870            # (17 x 21 x 13: 0.08697; 17^3: 0.05718 — h is half a cell of a field that falls as r^-8)
FD_ANGLE_F32_SLACK = 1.5e-6      # (1.48e-6; 1.30e-6)
NORMAL_TOL = 2 * (FD_ANGLE_F64 + FD_ANGLE_F32_SLACK)


def angle(a, b):
    """The angle between unit vectors, in float64, robust near 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 2 * np.arcsin(np.clip(np.linalg.norm(a - b, axis=-1) / 2, 0, 1))


# ---- the inputs of the per-kernel bit comparisons (shared by the CPU fault tests and the GPU tests) ----------------------------------
# A lattice on which p_a + 1 (p_b - p_a) is NOT p_b for the edges that leave sample 0 of each axis (found by search: on lattices of the
# grid formula that happens only where |lo| is far below the step, because everywhere else p_b - p_a is exact).
KERNEL_RES = (28, 10, 22)
KERNEL_BOUNDS = ((-0.0003006054612342268, -0.0003380553680472076, -0.00034364438033662736),
                 (1.6890870332717896, 2.2506580352783203, 0.3304902911186218))
KERNEL_SIZES = (1, 255, 257, 1000)
KERNEL_FIRST = 37


def kernel_grid():
    lo, hi = (np.asarray(b, dtype=F32) for b in KERNEL_BOUNDS)
    step = ((hi - lo) / (np.asarray(KERNEL_RES, dtype=F32) - F32(1))).astype(F32)
    return lo, step


def kernel_edges(n, seed):
    """first + n edge ids: random edges of the grid, then (from `first` on) one edge per direction that ends on the grid's last row,
    and — for n >= 255 — edge ids outside the grid, edges that leave it, and the 7 edges out of sample (0, 0, 0)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = KERNEL_RES
    total = KERNEL_FIRST + n
    i, j, k = rng.integers(0, nx - 1, total), rng.integers(0, ny - 1, total), rng.integers(0, nz - 1, total)
    e = 7 * ((i * ny + j) * nz + k) + rng.integers(0, 7, total)
    if n >= 7:
        for d in range(7):                                         # the last usable lower end in every direction
            dx, dy, dz = mt.DIRS[d]
            e[KERNEL_FIRST + d] = 7 * (((nx - 1 - dx) * ny + ny - 1 - dy) * nz + nz - 1 - dz) + d
    if n >= 255:
        last = (nx * ny * nz - 1) * 7
        e[KERNEL_FIRST + 10:KERNEL_FIRST + 17] = [-1, 7 * nx * ny * nz, last + 0, last + 6, 7 * (nz - 1) + 2, 2 ** 40, -2 ** 62]
        e[KERNEL_FIRST + 20:KERNEL_FIRST + 27] = np.arange(7)      # the edges that leave sample (0, 0, 0)
    return e.astype(np.int64)


def kernel_brackets(n, seed, level):
    """Random brackets after 0 .. 20 halvings with densities on either side of the level in both orders, and midpoint densities that
    include the level itself and (n >= 255) NaN and infinities."""
    rng = np.random.default_rng(seed + 1)
    total = KERNEL_FIRST + n
    halvings = rng.integers(0, 21, total)
    width = np.ldexp(F32(1), -halvings).astype(F32)
    t_lo = (rng.integers(0, 2 ** halvings).astype(F32) * width).astype(F32)
    t_hi = (t_lo + width).astype(F32)
    rising = rng.integers(0, 2, total).astype(bool)                # the surface entering (s_lo < level <= s_hi) or leaving
    below = (F32(level) - rng.random(total).astype(F32) * F32(3) - F32(1e-3)).astype(F32)
    above = (F32(level) + rng.random(total).astype(F32) * F32(3)).astype(F32)
    s_lo, s_hi = np.where(rising, below, above).astype(F32), np.where(rising, above, below).astype(F32)
    s_m = (F32(level) + (rng.random(total).astype(F32) - F32(0.5))).astype(F32)
    s_m[KERNEL_FIRST::5] = F32(level)
    if n >= 255:
        s_m[[3, 100, 200]] = [np.nan, np.inf, -np.inf]
    return t_lo, t_hi, s_lo, s_hi, s_m

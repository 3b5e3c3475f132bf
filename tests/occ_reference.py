"""NumPy float32 restatement of the occupancy grid and of the kept flag of a sample (mofanerf_amd/csrc/mofa_occ.hip).

The lattice has ``n = (nx, ny, nz)`` samples, sample (i,j,k) at ``lo + (i,j,k) * step``, hence ``n - 1`` cells per axis.
  cells    cell (i,j,k) is occupied iff one of its 8 corner samples is ``> threshold`` (NaN is not); then dilation: a cell is occupied
           iff some cell within Chebyshev distance ``dilate`` (clipped at the borders) was.
  kept     p = o + d * z (multiply and add rounded separately);  per axis t = (p - lo) / step in float32;
           inside = t >= 0 and t <= float32(n - 1) (NaN: outside);  c = min(int(t), n - 2);  kept = inside on all axes and cells[c].
"""
import numpy as np


def cells_from_grid(grid, threshold):
    """[nx-1, ny-1, nz-1] bool: one of the 8 corner samples is > threshold."""
    g = np.asarray(grid, dtype=np.float32)
    above = g > np.float32(threshold)
    nx, ny, nz = g.shape
    out = np.zeros((nx - 1, ny - 1, nz - 1), dtype=bool)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                out |= above[a:nx - 1 + a, b:ny - 1 + b, c:nz - 1 + c]
    return out


def dilate_cells(cells, dilate):
    """Chebyshev dilation by ``dilate`` cells, clipped at the borders (separable: one maximum per axis)."""
    out = np.asarray(cells, dtype=bool).copy()
    d = int(dilate)
    for axis in range(3):
        src = out.copy()
        n = src.shape[axis]
        for off in range(1, d + 1):
            if off >= n:
                break
            lo_sl, hi_sl = [slice(None)] * 3, [slice(None)] * 3
            lo_sl[axis], hi_sl[axis] = slice(0, n - off), slice(off, n)
            out[tuple(lo_sl)] |= src[tuple(hi_sl)]
            out[tuple(hi_sl)] |= src[tuple(lo_sl)]
    return out


def occupancy(grids, threshold, dilate):
    """Cells of the union of several density grids (one grid or a list), dilated."""
    if isinstance(grids, np.ndarray) and grids.ndim == 3:
        grids = [grids]
    cells = None
    for g in grids:
        c = cells_from_grid(g, threshold)
        cells = c if cells is None else cells | c
    return dilate_cells(cells, dilate)


def points(o, d, z):
    """p [R,S,3] = o + d * z in float32, the product and the sum rounded separately; z [R,S] or one shared row [S]."""
    o, d, z = (np.asarray(v, dtype=np.float32) for v in (o, d, z))
    if z.ndim == 1:
        z = np.broadcast_to(z[None, :], (o.shape[0], z.shape[0]))
    prod = (d[:, None, :] * z[:, :, None]).astype(np.float32)
    return (o[:, None, :] + prod).astype(np.float32)


def kept(o, d, z, lo, step, n, cells):
    """[R,S] bool: the kept flag of every sample of a pass."""
    p = points(o, d, z)
    lo, step = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(step, dtype=np.float32).reshape(3)
    cells = np.asarray(cells, dtype=bool)
    keep = np.ones(p.shape[:2], dtype=bool)
    idx = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            t = ((p[..., a] - lo[a]).astype(np.float32) / step[a]).astype(np.float32)
            inside = (t >= np.float32(0)) & (t <= np.float32(n[a] - 1))
            keep &= inside
            idx.append(np.minimum(np.where(inside, t, np.float32(0)).astype(np.int64), n[a] - 2))
    return keep & cells[idx[0], idx[1], idx[2]]


def ball_grid(n, lo, step, centre, radius):
    """Density grid r^2 - |p - c|^2 at the lattice points lo + (i,j,k) * step (float32 coordinates, the product and the sum rounded
    separately as mofa_grid_points forms them; the field itself in float64, rounded once)."""
    lo, step = np.asarray(lo, dtype=np.float32).reshape(3), np.asarray(step, dtype=np.float32).reshape(3)
    ax = [(lo[a] + (np.arange(n[a], dtype=np.float32) * step[a]).astype(np.float32)).astype(np.float32).astype(np.float64) for a in range(3)]
    x, y, zz = np.meshgrid(*ax, indexing="ij")
    c = np.asarray(centre, dtype=np.float64)
    return (float(radius) ** 2 - ((x - c[0]) ** 2 + (y - c[1]) ** 2 + (zz - c[2]) ** 2)).astype(np.float32)

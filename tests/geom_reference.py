"""NumPy restatements of the surface buffers of the geometry render (``mofa_depth_median``, ``mofa_point_normals``), written from their
specification and not from the kernels.

* The median: fp64 prefix sums ``C_i = w_0 + ... + w_i``.  An fp32 sum of exactly ``w_0..w_i`` — in any association — lies within
  ``eps = (S-1) 2^-24 sum|w|`` of ``C_i``, so an implementation may report index ``i`` iff ``C[i] >= t - eps`` and (``i = 0`` or
  ``C[i-1] < t + eps``) hold for it and no earlier index was certain (``C[j] >= t + eps`` for a ``j < i``); it may report -1 iff no
  ``C[j]`` is certain.  Where every partial sum is exact in fp32 the window is one index wide and the answer is ``median_exact``'s.
* The normals: the stencil in ``np.float32``, one rounding per operation, pixel by pixel.

``fault=`` builds a deliberately wrong variant for tests/test_geom_reference_cpu.py, which shows that the comparisons used on the GPU
see each of them."""
import numpy as np


# ---- median ---------------------------------------------------------------------------------------------------------------------------
def rows_of(z, R, S):
    z = np.asarray(z)
    return np.broadcast_to(z, (R, S)) if z.ndim == 1 else z


def median_exact(weights, z, threshold):
    """(index int32 [R], depth float32 [R]) from fp64 prefix sums: the first i with C_i >= threshold, -1 and z[S-1] if there is none (a NaN
    weight makes every later C_i NaN, which compares false)."""
    w = np.asarray(weights, np.float64)
    R, S = w.shape
    zr = rows_of(z, R, S)
    with np.errstate(invalid="ignore"):
        hit = np.cumsum(w, -1) >= np.float64(np.float32(threshold))
    index = np.where(hit.any(-1), hit.argmax(-1), -1).astype(np.int32)
    depth = zr[np.arange(R), np.where(index < 0, S - 1, index)].astype(np.float32)
    return index, depth


def median_eps(weights):
    w = np.asarray(weights, np.float64)
    return (w.shape[1] - 1) * 2.0 ** -24 * np.abs(w).sum(-1)


def median_admissible(weights, threshold):
    """bool [R, S + 1]: column i < S — index i may be reported; column S — -1 may be reported.  Rows with a NaN weight are not handled
    here (use median_exact on them)."""
    w = np.asarray(weights, np.float64)
    R, S = w.shape
    t = np.float64(np.float32(threshold))
    C = np.cumsum(w, -1)
    eps = median_eps(w)[:, None]
    certain = C >= t + eps                                            # every correct fp32 prefix sum reaches the threshold here
    before = np.concatenate([np.zeros((R, 1), bool), np.logical_or.accumulate(certain, -1)[:, :-1]], -1)       # ... at an earlier index
    ok = (C >= t - eps) & ~before
    return np.concatenate([ok, ~certain.any(-1, keepdims=True)], -1)


def median_check(weights, z, threshold, index, depth):
    """The window rule for every ray: returns (bad rays, share of rays with more than one admissible answer)."""
    w = np.asarray(weights, np.float64)
    R, S = w.shape
    zr = rows_of(z, R, S)
    adm = median_admissible(w, threshold)
    index = np.asarray(index)
    in_range = (index >= -1) & (index < S)
    col = np.where(index < 0, S, np.clip(index, 0, S - 1))
    good = in_range & adm[np.arange(R), col]
    want_depth = zr[np.arange(R), np.where(index < 0, S - 1, np.clip(index, 0, S - 1))].astype(np.float32)
    good &= np.asarray(depth, np.float32).view(np.uint32) == want_depth.view(np.uint32)
    return np.flatnonzero(~good), float((adm.sum(-1) > 1).mean())


def composite_weights(sigma, dist):
    """Alpha-compositing weights of densities sigma [R,S] at constant spacing: w_i = alpha_i prod_{j<i} (1 - alpha_j), in fp64, as float32."""
    alpha = 1.0 - np.exp(-np.maximum(np.asarray(sigma, np.float64), 0.0) * dist)
    T = np.cumprod(np.concatenate([np.ones_like(alpha[:, :1]), 1.0 - alpha[:, :-1]], -1), -1)
    return (alpha * T).astype(np.float32)


# ---- normals --------------------------------------------------------------------------------------------------------------------------
FAULTS = ("swap", "no_flip", "one_sided", "strict")


def point_normals(points, acc, rays_d, acc_min, fault=None):
    """(normals float32 [H,W,3], valid uint8 [H,W]).  ``fault``: 'swap' (dv x du), 'no_flip' (never turned to the camera), 'one_sided'
    (a forward difference where a central one is due), 'strict' (usable iff acc > acc_min)."""
    assert fault is None or fault in FAULTS
    f = np.float32
    P, A, D = np.asarray(points, f), np.asarray(acc, f), np.asarray(rays_d, f)
    H, W = A.shape
    acc_min = f(acc_min)
    with np.errstate(invalid="ignore"):
        usable = (A > acc_min) if fault == "strict" else (A >= acc_min)
    N, V = np.zeros((H, W, 3), f), np.zeros((H, W), np.uint8)

    def diff(r, c, dr, dc):
        prev = 0 <= r - dr and 0 <= c - dc and usable[r - dr, c - dc]
        nxt = r + dr < H and c + dc < W and usable[r + dr, c + dc]
        if prev and nxt and fault != "one_sided":
            return P[r + dr, c + dc] - P[r - dr, c - dc]
        if nxt:
            return P[r + dr, c + dc] - P[r, c]
        if prev:
            return P[r, c] - P[r - dr, c - dc]
        return None

    with np.errstate(all="ignore"):
        for r in range(H):
            for c in range(W):
                if not usable[r, c]:
                    continue
                du, dv = diff(r, c, 0, 1), diff(r, c, 1, 0)
                if du is None or dv is None:
                    continue
                if fault == "swap":
                    du, dv = dv, du
                nx = f(f(du[1] * dv[2]) - f(du[2] * dv[1]))
                ny = f(f(du[2] * dv[0]) - f(du[0] * dv[2]))
                nz = f(f(du[0] * dv[1]) - f(du[1] * dv[0]))
                length = np.sqrt(f(f(f(nx * nx) + f(ny * ny)) + f(nz * nz)))
                if not length > 0:
                    continue
                n = np.array([f(nx / length), f(ny / length), f(nz / length)], f)
                s = f(f(f(n[0] * D[r, c, 0]) + f(n[1] * D[r, c, 1])) + f(n[2] * D[r, c, 2]))
                if s > 0 and fault != "no_flip":
                    n = -n
                N[r, c], V[r, c] = n, 1
    return N, V


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))

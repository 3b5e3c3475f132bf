"""Two NumPy statements of the resampler (``mofa_sample_pdf_merge`` / ``mofa_sample_pdf``: inverse-cdf sampling, the merge with the coarse
positions, the spread of the new samples), neither of which calls the library, and the batches the tests run them on.

(a) THE WINDOW, from the specification (tools/run_nerf_helpers.py:203-247 of the reference), in fp64.  With ``w' = w + (double)1e-5f``,
    ``C_0 = 0``, ``C_k = sum_{i<k} w'_i / sum w'``, the fp32 bin edges ``b`` and ``eps = 4 * 2^-24``, a sample ``s`` for ``u`` is admissible
    iff, for some bin k with ``C_k - eps <= u <= C_{k+1} + eps`` and ``den = C_{k+1} - C_k``,
      divide branch  ``den >= 1e-5 - 2 eps``  and  ``|s - (b_k + (u - C_k) / den * (b_{k+1} - b_k))| <= (b_{k+1} - b_k) 3 eps / den + 4 * 2^-24 max|b|``
      unit branch    ``den <= 1e-5 + 2 eps``  and  ``|s - (b_k + (u - C_k) (b_{k+1} - b_k))| <= (b_{k+1} - b_k) eps + 4 * 2^-24 max|b|``
    or (top edge) ``u >= C_{B-1} - eps`` and ``s == b_{B-1}`` exactly.
    eps is derived, not measured: three fp32 roundings per pdf entry (the add, the rounded sum, the division) move C_k by at most
    ``3 * 2^-24 C_k``, and the final rounding of a prefix that was accumulated above fp32 adds ``2^-25``.  It therefore covers an implementation
    that accumulates the prefix above fp32 — the kernel and torch's CPU ``cumsum`` both do.  A sequential fp32 ``cumsum`` is a legitimate
    variant that needs ``(k + 3) 2^-24`` at bin k (``eps=`` takes it; with ``4 * 2^-24`` a prototype put 14 of 16,384 of its samples outside).
    Within ``2 eps`` of the 1e-5 threshold BOTH branches are admissible: the window cannot tell ``<`` from ``<=`` there, the bits can.
    NaN rows are not handled here.

(b) THE RESTATEMENT, in ``np.float32`` with one rounding per operation:
      bins = 0.5f * (z[i+1] + z[i])  (or the given bins)        wp = fl(w + 1e-5f)  over the interior weights only
      wsum = (float)(fp64 sum of wp)                            pdf = fl(wp / wsum)
      cdf_0 = 0, cdf_k = (float)(fp64 sum of pdf_0 .. pdf_{k-1})
      lo = first index with cdf > u, below = max(lo - 1, 0), above = min(lo, B - 1)
      den = fl(c1 - c0), replaced by 1 when < 1e-5f             t = fl(fl(u - c0) / den)            s = fl(b0 + fl(t * fl(b1 - b0)))
    The kernel takes its fp64 sums in another association (a lane-strided sum for wsum, a 64-wide scan plus a carry for the prefixes), so
    ``decided`` says per ray whether every rounded sum is the same in ANY association: either all terms are multiples of ``2^-q`` and the
    total is below ``2^52 * 2^-q`` (every association is exact), or the exact sum (integers) times ``1 -/+ (n + 1) 2^-53`` rounds to one
    float.  A batch holds decided rows only; ``build`` re-draws a row that is not.

Then the merge (a stable sort of ``cat(z, samples)``, NaN last in index order), ``z_std`` (the fp64 population standard deviation) and a
flag for whether a ray's new samples are non-decreasing, which decides the merge path the kernel takes.

``fault=`` builds a deliberately wrong variant for tests/test_pdf_reference_cpu.py, which shows that the comparisons used on the GPU see
each of them.

THE BATCHES (``batches()``) are the smallest shapes at which this kernel can go wrong: the seams of the 64-wide cdf scan, the 4 / 2 / 1
rays-per-block boundaries of the 64 KiB of LDS, ray counts that fill no block.  Conditions, asserted for every batch by the CPU file:
no undecided row; in an aimed batch with Ni >= 2 at least one ray merges along the sorted path and one along the general path from
unsorted ``u``; at least 5 % of the aimed samples take the unit branch.  At Ni = 1 a ray is sorted whatever ``u`` is.

The third path — the general merge from SORTED ``u`` with finite samples — is the sharp input for the kernel's sorted-run check: the
samples are in order but for ONE adjacent pair, by an ulp.  It arises at a bin edge: ``fl(b0 + fl(t * fl(b1 - b0)))`` with ``t`` just
below 1 can exceed ``b1`` when ``fl(b1 - b0)`` was rounded up, and the next ``u`` gives ``b1`` itself.  With the positions of this model's
cameras (8 to 26) neighbouring bin edges lie within a factor 2, ``b1 - b0`` is exact and no such ray was found among 2,007 aimed rays
(S in {5, 17, 66, 131}, all finite weight patterns); there NaN rays alone take the path.  With coarse positions that span several binades
(``coarse_z('binades')``: log-uniform in 0.05 .. 100) about one aimed ray in 5,000 has such a pair: a search of seeds 0 .. 5999 (S in
{4, 5, 6, 9, 17}, Ni = 64, 42,318 rays) found eight, and ``inversion_batches`` builds four of them, each also with its pair placed inside,
across and just behind a 64-lane stride of the check and at the row's end.  In those batches the third path's condition holds and is
asserted.
"""
import os

import numpy as np

F = np.float32
EPS = 4.0 * 2.0 ** -24
TINY = F(1e-5)
LDS_FLOATS = 16384
FAULTS_SAMPLE = ("left", "exterior", "no_branch", "le_branch", "carry", "no_clamp", "coarse_bins", "neighbour_u", "ray_shift", "fp32_cdf")
FAULTS_STD = ("unbiased",)
FAULTS_MERGE = ("drop_tie", "assume_sorted")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rows_of(a, R):
    a = np.asarray(a)
    return np.broadcast_to(a, (R, a.shape[-1])) if a.ndim == 1 else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def bits_differing(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def midpoints(z):
    z = np.asarray(z, F)
    return (F(0.5) * (z[..., 1:] + z[..., :-1])).astype(F)


def rays_per_block(S, Ni):
    per = 3 * S + Ni
    return 4 if per * 4 <= LDS_FLOATS else (2 if per * 2 <= LDS_FLOATS else 1)


# ---- (a) the window ---------------------------------------------------------------------------------------------------------------------
def window_ratio(bins, bin_weights, u, samples, eps=EPS):
    """err / tolerance of the best admissible reading of every sample, float64 [R, Ni]: admissible iff <= 1 (0 at the top edge, inf where no
    bin and branch accepts the sample, NaN samples included).  ``bins [R,B] or [B]``, ``bin_weights [R,B-1]``, ``u [R,Ni] or [Ni]``;
    ``eps``: a number, or a function of the bin index (``lambda k: (k + 3) * 2.0 ** -24``)."""
    wts = np.asarray(bin_weights, np.float64)
    R, NW = wts.shape
    B = NW + 1
    bins, u, s = rows_of(bins, R).astype(np.float64), rows_of(u, R).astype(np.float64), np.asarray(samples, np.float64)
    assert bins.shape == (R, B) and s.shape == u.shape
    k_all = np.arange(NW)
    e_bin = np.full(NW, float(eps)) if not callable(eps) else np.asarray([float(eps(k + 1)) for k in k_all])      # the bin's upper edge
    e_max = float(e_bin.max())
    out = np.full(s.shape, np.inf)
    with np.errstate(all="ignore"):
        for r in range(R):
            wp = wts[r] + float(TINY)
            C = np.concatenate([[0.0], np.cumsum(wp) / wp.sum()])
            b, ur, sr = bins[r], u[r], s[r]
            slack = 4.0 * 2.0 ** -24 * np.abs(b).max()
            k_lo = np.clip(np.searchsorted(C[1:] + e_max, ur, "left"), 0, NW - 1)       # the first bin whose upper edge reaches u
            k_hi = np.clip(np.searchsorted(C[:-1] - e_max, ur, "right") - 1, 0, NW - 1)  # the last bin whose lower edge does
            best = np.full(ur.shape, np.inf)
            for d in range(int((k_hi - k_lo).max()) + 1 if ur.size else 0):
                k = np.minimum(k_lo + d, NW - 1)
                e = e_bin[k]
                inside = (k_lo + d <= k_hi) & (C[k] - e <= ur) & (ur <= C[k + 1] + e)
                den, width = C[k + 1] - C[k], b[k + 1] - b[k]
                for ok, want, tol in ((den >= 1e-5 - 2 * e, b[k] + (ur - C[k]) / den * width, width * 3 * e / den + slack),
                                      (den <= 1e-5 + 2 * e, b[k] + (ur - C[k]) * width, width * e + slack)):
                    err = np.abs(sr - want)
                    ratio = np.where(err == 0, 0.0, err / tol)
                    best = np.fmin(best, np.where(inside & ok & np.isfinite(ratio), ratio, np.inf))
            top = (ur >= C[NW] - e_bin[NW - 1]) & (sr == b[NW])
            out[r] = np.where(top, 0.0, best)
    return out


# ---- (b) the restatement ----------------------------------------------------------------------------------------------------------------
def _round_f32(N, e):
    """N * 2^e (N a positive integer) rounded to the nearest float32, ties to even; normal range only."""
    bl = N.bit_length()
    if bl > 24:
        shift = bl - 24
        q, rem, half = N >> shift, N & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
        N, e = q, e + shift
    assert e + N.bit_length() > -125
    return float(np.ldexp(float(N), e))


def _sums_decided(terms):
    """Are float32(fp64 sum of terms[:k]) for every k = 1..n, taken in ANY association, all decided?  Non-negative finite float32 terms."""
    t = np.asarray(terms, F)
    assert np.all(t >= 0) and np.all(np.isfinite(t))
    n = t.size
    m, ex = np.frexp(t.astype(np.float64))
    unit = np.where(t > 0, ex - 24, 10_000)                            # t is a multiple of 2^unit
    q = np.minimum.accumulate(unit)
    prefix = np.cumsum(t.astype(np.float64))
    exact = prefix < np.ldexp(1.0, np.minimum(q, 900) + 52)           # by induction every partial sum below is an integer under 2^52 units
    if exact.all():
        return True
    e_min = int(unit.min())
    ints = [int(round(float(mi) * 2 ** 24)) << int(ui - e_min) if ti > 0 else 0 for mi, ui, ti in zip(m, unit, t)]
    total = 0
    for k in range(n):
        total += ints[k]
        if exact[k] or total == 0:
            continue
        lo = _round_f32(total * ((1 << 53) - (k + 2)), e_min - 53)
        hi = _round_f32(total * ((1 << 53) + (k + 2)), e_min - 53)
        if lo != hi:
            return False
        assert float(F(prefix[k])) == lo                              # the sequential fp64 sum is one of the associations
    return True


def decided(bin_weights):
    """bool [R]: every rounded fp64 sum of the restatement (wsum, then each cdf prefix) is the same in any association.  A row with a NaN is
    decided: all its samples are NaN whatever the sums give."""
    w = np.asarray(bin_weights, F)
    out = np.ones(w.shape[0], bool)
    for r in range(w.shape[0]):
        if not np.isfinite(w[r]).all():
            continue
        wp = (w[r] + TINY).astype(F)
        if not _sums_decided(wp):                                      # only the last prefix (the total) is used; the others are stricter
            out[r] = False
            continue
        pdf = (wp / F(wp.astype(np.float64).sum())).astype(F)
        out[r] = _sums_decided(pdf)
    return out


def cdf_bits(bin_weights, fault=None):
    """float32 [R, B]: the restated cdf."""
    w = np.asarray(bin_weights, F)
    with np.errstate(invalid="ignore"):
        wp = (w + TINY).astype(F)
        wsum = wp.astype(np.float64).sum(-1).astype(F)
        pdf = (wp / wsum[:, None]).astype(F)
        if fault == "fp32_cdf":
            acc = np.zeros(w.shape[0], F)
            run = np.empty_like(pdf)
            for k in range(pdf.shape[1]):
                acc = (acc + pdf[:, k]).astype(F)
                run[:, k] = acc
        elif fault == "carry":                                         # every chunk of 64 prefixes starts again from zero
            run = np.concatenate([np.cumsum(pdf[:, c:c + 64].astype(np.float64), -1) for c in range(0, pdf.shape[1], 64)], -1).astype(F)
        elif fault and fault.startswith("carry@"):                     # the carry into the chunk that starts at ONE seam is lost
            c = int(fault[6:])
            run = np.cumsum(pdf.astype(np.float64), -1)
            run[:, c:c + 64] = np.cumsum(pdf[:, c:c + 64].astype(np.float64), -1)
            run = run.astype(F)
        else:
            run = np.cumsum(pdf.astype(np.float64), -1).astype(F)
    return np.concatenate([np.zeros((w.shape[0], 1), F), run], -1)


def sample_bits(bins, bin_weights, u, fault=None):
    """(samples float32 [R, Ni], unit bool [R, Ni]): the plain form on given bins; ``unit`` marks the samples of the 1e-5 branch."""
    assert fault is None or fault in FAULTS_SAMPLE or fault.startswith("carry@")
    w = np.asarray(bin_weights, F)
    R, NW = w.shape
    B = NW + 1
    bins, u = rows_of(np.asarray(bins, F), R), rows_of(np.asarray(u, F), R)
    if fault == "neighbour_u":
        u = np.roll(u, -1, 0)
    cdf = cdf_bits(w, fault)
    pad = 1 if fault == "no_clamp" else 0                              # what lies behind the row is modelled as zeros
    cdf_p = np.concatenate([cdf, np.zeros((R, pad), F)], -1)
    bins_p = np.concatenate([bins, np.zeros((R, pad), F)], -1)
    s, unit = np.empty(u.shape, F), np.zeros(u.shape, bool)
    with np.errstate(all="ignore"):
        for r in range(R):
            if np.isnan(cdf[r]).any():                                  # a NaN weight makes wsum NaN and with it every cdf entry but the first
                s[r] = np.nan
                continue
            lo = np.searchsorted(cdf[r], u[r], "left" if fault == "left" else "right")
            below, above = np.maximum(lo - 1, 0), (lo if fault == "no_clamp" else np.minimum(lo, B - 1))
            c0, c1, b0, b1 = cdf_p[r][below], cdf_p[r][above], bins_p[r][below], bins_p[r][above]
            den = (c1 - c0).astype(F)
            small = np.zeros_like(den, bool) if fault == "no_branch" else (den <= TINY if fault == "le_branch" else den < TINY)
            den = np.where(small, F(1.0), den).astype(F)
            t = ((u[r] - c0).astype(F) / den).astype(F)
            s[r] = (b0 + (t * (b1 - b0).astype(F)).astype(F)).astype(F)
            unit[r] = small
    return s, unit


def resample(z, weights, u, fault=None):
    """The merge form's samples: (z_samples float32 [R, Ni], unit bool [R, Ni]) from coarse positions ``z [R,S] or [S]`` and their weights
    ``[R,S]`` — the bins are the mid-points, the bin weights the interior weights."""
    w = np.asarray(weights, F)
    R, S = w.shape
    z, u = rows_of(np.asarray(z, F), R), rows_of(np.asarray(u, F), R)
    if fault == "ray_shift":                                           # ray r works on the inputs of the ray one block further on
        by = rays_per_block(S, u.shape[-1]) % R
        z, w, u = np.roll(z, -by, 0), np.roll(w, -by, 0), np.roll(u, -by, 0)
    bins = z[:, :S - 1] if fault == "coarse_bins" else midpoints(z)
    inner = w[:, :S - 2] if fault == "exterior" else w[:, 1:S - 1]
    return sample_bits(bins, inner, u, None if fault in ("ray_shift", "coarse_bins", "exterior") else fault)


def merge(z, samples, fault=None, fill=np.nan):
    """float32 [R, S + Ni]: the stable sort of cat(z, samples) — equal values in index order, NaN last in index order.  'drop_tie' ranks by
    the count of smaller values alone, so the members of a tie claim one slot and the others keep ``fill``; 'assume_sorted' merges every ray
    by the binary-search ranks that hold for two sorted runs (coarse e: e + #(samples < v), sample j: j + #(coarse <= v)) — a sorted-run
    check that sees nothing."""
    assert fault is None or fault in FAULTS_MERGE
    s = np.asarray(samples, F)
    both = np.concatenate([rows_of(np.asarray(z, F), s.shape[0]), s], -1)
    out = np.full(both.shape, fill, F)
    for r in range(both.shape[0]):
        v = both[r]
        nan = np.isnan(v)
        num = np.flatnonzero(~nan)
        if fault == "drop_tie":
            rank = np.searchsorted(np.sort(v[num]), v[num], "left")
            out[r, rank] = v[num]
            continue
        if fault == "assume_sorted":
            S = v.size - s.shape[1]
            with np.errstate(invalid="ignore"):
                rank = np.concatenate([np.arange(S) + (v[None, S:] < v[:S, None]).sum(-1), np.arange(s.shape[1]) + (v[None, :S] <= v[S:, None]).sum(-1)])
            out[r, rank] = v
            continue
        order = np.concatenate([num[np.argsort(v[num], kind="stable")], np.flatnonzero(nan)])
        out[r] = v[order]
    return out


def z_std(samples, fault=None):
    """float64 [R]: the population standard deviation of each ray's samples ('unbiased': divided by Ni - 1)."""
    assert fault is None or fault in FAULTS_STD
    s = np.asarray(samples, np.float64)
    with np.errstate(all="ignore"):
        var = ((s - s.mean(-1, keepdims=True)) ** 2).sum(-1) / (s.shape[-1] - (1 if fault == "unbiased" else 0))
        return np.sqrt(var)


def std_within_an_ulp(got, want64):
    """bool [R]: float32 ``got`` within one fp32 ulp of the rounded fp64 value, NaN meeting NaN."""
    got, w = np.asarray(got, F), np.asarray(want64, np.float64).astype(F)
    near = (got >= np.nextafter(w, F(-np.inf))) & (got <= np.nextafter(w, F(np.inf)))
    return np.where(np.isnan(w), np.isnan(got), near)


def non_decreasing(samples):
    """bool [R]: the kernel merges such a ray by binary search (the sorted path); every other ray, NaN rays included, by rank."""
    s = np.asarray(samples, F)
    with np.errstate(invalid="ignore"):
        return np.all(s[:, :-1] <= s[:, 1:], -1)


# ---- the batches ------------------------------------------------------------------------------------------------------------------------
SEAMS = ((4, 1), (5, 2), (65, 64), (66, 64), (67, 65), (130, 63), (131, 128), (257, 200))
BLOCKS = ((1000, 1096), (1000, 1097), (2000, 2192), (2000, 2193), (4096, 4096))
PATTERNS = ("zero", "spike_first", "spike_mid", "spike_last", "only_w0", "only_wlast", "empty_half", "opaque_front", "plain", "times_1000",
            "times_1e-6", "threshold", "nan_interior", "nan_w0")


def weights_row(pattern, S, rng):
    """One row of S coarse weights.  'threshold': pdf_0 == 1e-5f exactly (the first bin's weight is 0 and the sum rounds to 1), the one
    place where ``den < 1e-5f`` and ``den <= 1e-5f`` differ — the cdf's grid near 1 holds no difference equal to 1e-5f."""
    w = np.zeros(S, F)
    NW = S - 2
    if pattern == "spike_first":
        w[1] = rng.uniform(1.5, 4.0)
    elif pattern == "spike_mid":
        w[1 + NW // 2] = rng.uniform(1.5, 4.0)
    elif pattern == "spike_last":
        w[S - 2] = rng.uniform(1.5, 4.0)
    elif pattern == "only_w0":
        w[0] = 1.0
    elif pattern == "only_wlast":
        w[S - 1] = 1.0
    elif pattern == "empty_half":
        w[S // 2:] = rng.uniform(0, 1, S - S // 2) ** 4
    elif pattern == "opaque_front":
        w[1:] = (0.9 * 0.1 ** np.arange(S - 1, dtype=np.float64)).astype(F)    # acc = 1 within five samples; every later bin is below 1e-5
    elif pattern in ("plain", "times_1000", "times_1e-6", "nan_interior", "nan_w0"):
        w[:] = rng.uniform(0, 1, S) ** 4 / S * {"times_1000": 1000.0, "times_1e-6": 1e-6}.get(pattern, 1.0)
        if pattern == "nan_interior":
            w[1 + int(rng.integers(0, NW))] = np.nan
        if pattern == "nan_w0":
            w[0] = np.nan
    elif pattern == "threshold":
        j = 2 + int(rng.integers(0, NW - 1))
        start = F(1.0 - NW * 1e-5)
        for step in range(-64, 65):
            w[j] = start + F(step) * np.spacing(start)
            wp = (w[1:S - 1] + TINY).astype(F)
            if F(wp.astype(np.float64).sum()) == F(1.0):
                break
        else:
            raise AssertionError("no weight makes the sum round to 1")
        assert (wp / F(1.0)).astype(F)[0] == TINY
    else:
        assert pattern == "zero", pattern
    return w


def coarse_z(kind, R, S, rng):
    if kind == "lindisp":                                              # uniform in disparity between 8 and 26, one shared row
        t = np.linspace(0.0, 1.0, S)
        return (1.0 / (1.0 / 8.0 * (1.0 - t) + 1.0 / 26.0 * t)).astype(F)
    if kind == "shared":
        return np.sort(rng.uniform(8, 26, S)).astype(F)
    if kind == "binades":                                              # near << far: neighbouring bin edges more than a factor 2 apart
        return np.sort(np.exp(rng.uniform(np.log(0.05), np.log(100.0), (R, S))), -1).astype(F)
    z = np.sort(rng.uniform(8, 26, (R, S)), -1).astype(F)
    if kind == "repeated":                                             # zero-width bins
        z[:, 1::3] = z[:, 0:-1:3]
    return z


def aimed_u(cdf_row, Ni, rng, ordered, first_bin=None):
    """For every bin k: cdf_k, the float below it, the bin's middle, the float below cdf_{k+1} — tiled to Ni, or truncated to Ni values
    from ``first_bin`` on (if None: drawn among the bins below the 1e-5 threshold, among all bins where there is none)."""
    c = np.asarray(cdf_row, F)
    if first_bin is None:
        small = np.flatnonzero((c[1:] - c[:-1]).astype(F) < TINY)
        first_bin = int(rng.choice(small)) if small.size else int(rng.integers(0, c.size - 1))
    a = np.stack([c[:-1], np.nextafter(c[:-1], F(0)), (F(0.5) * (c[:-1] + c[1:])).astype(F), np.nextafter(c[1:], F(0))], -1).reshape(-1)
    if a.size > Ni:
        start = min(4 * first_bin, a.size - Ni)
        a = a[start:start + Ni]
    else:
        a = np.resize(a, Ni)
    return np.sort(a) if ordered else a


def draw_u(kind, R, Ni, rng):
    if kind == "linspace":
        return np.linspace(0.0, 1.0, Ni, dtype=F)                       # one shared row; u = 1 exactly at its end (u = 0 alone at Ni = 1)
    u = rng.uniform(0, 1, (R, Ni)).astype(F)
    if kind == "sorted":
        u = np.sort(u, -1)
    if kind == "duplicates":
        u = u[:, rng.integers(0, max(Ni // 3, 1), Ni)]
    if kind == "shared":
        u = u[0]
    return u


def build(name, S, Ni, patterns, z_kind, u_kind, seed, rows=None):
    """One batch: dict(name, S, Ni, R, z [R,S] or [S], w [R,S], u [R,Ni] or [Ni], patterns, aimed).  A row whose sums are not decided is
    drawn again; ``rows``: recorded (z, w) rows instead of patterns."""
    rng = np.random.default_rng(seed)
    if rows is not None:
        z, w = np.asarray(rows[0], F), np.asarray(rows[1], F)
        R = w.shape[0]
        assert decided(w[:, 1:S - 1]).all(), name
    else:
        R = len(patterns)
        z = coarse_z(z_kind, R, S, rng)
        w = np.empty((R, S), F)
        for r, p in enumerate(patterns):
            for attempt in range(20):
                w[r] = weights_row(p, S, rng)
                if decided(w[r:r + 1, 1:S - 1])[0]:
                    break
            else:
                raise AssertionError(f"{name}: no decided row for {p}")
    if u_kind.startswith("aimed"):
        cdf = cdf_bits(w[:, 1:S - 1])
        assert not np.isnan(cdf).any(), name
        u = np.stack([aimed_u(cdf[r], Ni, rng, ordered=(u_kind == "aimed_sorted" or (u_kind == "aimed" and r % 2 == 1)),
                              first_bin=0 if patterns and patterns[r] == "threshold" else None) for r in range(R)])    # its threshold bin is bin 0
    else:
        u = draw_u(u_kind, R, Ni, rng)
    if patterns and "zero" in patterns:                                # w[0] and w[S-1] are not read: on the zero row's z and u such a row
        for r, p in enumerate(patterns):                               # must give the zero row's samples
            if p in ("only_w0", "only_wlast"):
                for a in (z, u):
                    if a.ndim == 2:
                        a[r] = a[patterns.index("zero")]
    return dict(name=name, S=S, Ni=Ni, R=R, z=z, w=w, u=u, patterns=tuple(patterns or ()), aimed=u_kind.startswith("aimed"))


def _take(offset, R):
    return [PATTERNS[(offset + j) % len(PATTERNS)] for j in range(R)]


FINITE = ("opaque_front", "threshold", "spike_mid", "plain", "empty_half", "zero", "times_1000", "spike_first", "times_1e-6")
_cache = {}


def batches():
    """Every batch, built once and shared (read-only) by the tests."""
    if "all" in _cache:
        return _cache["all"]
    out = []
    for i, (S, Ni) in enumerate(SEAMS):
        tag, sd = f"{S}+{Ni}", 1000 * i
        out += [build(f"{tag} all patterns, linspace u", S, Ni, list(PATTERNS), "rows", "linspace", sd + 1),
                build(f"{tag} 9 rays, shared z, unsorted u", S, Ni, _take(0, 9), "shared", "uniform", sd + 2),
                build(f"{tag} 5 rays, repeated z, sorted u", S, Ni, _take(5, 5), "repeated", "sorted", sd + 3),
                build(f"{tag} 3 rays, lindisp z, duplicate u", S, Ni, _take(10, 3), "lindisp", "duplicates", sd + 4),
                build(f"{tag} 2 NaN rays, one shared unsorted u", S, Ni, _take(12, 2), "rows", "shared", sd + 5),
                build(f"{tag} 1 ray, linspace u", S, Ni, _take(7, 1), "rows", "linspace", sd + 6),
                build(f"{tag} 9 rays, aimed u", S, Ni, list(FINITE), "rows", "aimed", sd + 7),
                build(f"{tag} 5 rays, shared z, aimed u", S, Ni, list(FINITE[:5]), "shared", "aimed", sd + 8)]
    for i, (S, Ni) in enumerate(BLOCKS):
        tag, sd = f"{S}+{Ni}", 100_000 + 1000 * i
        out += [build(f"{tag} 3 rays, linspace u", S, Ni, ["plain", "opaque_front", "spike_mid"], "rows", "linspace", sd + 1),
                build(f"{tag} 3 rays, unsorted u", S, Ni, ["times_1000", "nan_interior", "empty_half"], "shared", "uniform", sd + 2),
                build(f"{tag} 3 rays, aimed u", S, Ni, ["opaque_front", "threshold", "plain"], "rows", "aimed", sd + 3)]
    for i, (fx, R) in enumerate((("e2e_small.npz", 9), ("e2e_long.npz", 5))):
        g = np.load(os.path.join(GOLDEN, fx))
        zc, wc = g["z_coarse"], g["weights_coarse"]
        S, Ni = zc.shape[1], g["z_samples"].shape[1]
        c = cdf_bits(wc[:, 1:S - 1])                                  # the rays with the most bins under the threshold, and a few from across
        dense = np.argsort(-((c[:, 1:] - c[:, :-1]).astype(F) < TINY).sum(-1), kind="stable")[:R - R // 4]     # the frame (empty at its rim)
        pick = np.concatenate([dense, np.setdiff1d(np.linspace(0, zc.shape[0] - 1, R).astype(int), dense)[:R // 4]])
        out += [build(f"{fx} {R} recorded rays, linspace u", S, Ni, None, None, "linspace", 200_000 + i, rows=(zc[pick], wc[pick])),
                build(f"{fx} {R} recorded rays, aimed u", S, Ni, None, None, "aimed", 200_010 + i, rows=(zc[pick], wc[pick]))]
    out += inversion_batches()
    _cache["all"] = out
    return out


def inversions(samples_row):
    """indices j with s[j] > s[j + 1]"""
    s = np.asarray(samples_row, F)
    return np.flatnonzero(s[:-1] > s[1:])


INVERSION_SEEDS = ((126, 5), (711, 5), (2433, 17), (4701, 17))            # found by a search over seeds 0 .. 5999 (see the module's docstring)
PLACED_NI = 130


def inversion_batches():
    """The third merge path with numbers.  Per (seed, S) of INVERSION_SEEDS two batches: the aimed batch over coarse positions that span
    several binades, whose ray 3 (sorted ``u``) has ONE adjacent pair of samples in the wrong order, by an ulp at a bin edge; and that ray
    four times at Ni = 130 with the pair's ``u`` values placed among sorted uniform ones so that the pair sits at elements (62, 63),
    (63, 64) and (64, 65) of the ray's S + Ni positions — inside a 64-lane stride of the kernel's sorted-run check, across it, and at the
    start of the next — and at the row's very end."""
    out = []
    for seed, S in INVERSION_SEEDS:
        b = build(f"{S}+64 9 rays, z over binades, aimed u (seed {seed})", S, 64, list(FINITE), "binades", "aimed", seed)
        b["third_path"] = True
        s = resample(b["z"], b["w"], b["u"])[0]
        r = 3
        j = inversions(s[r])
        assert j.size == 1, (seed, S, j)
        ua, ub = b["u"][r, j[0]], b["u"][r, j[0] + 1]
        rng = np.random.default_rng(seed + 1)
        places = (62 - S, 63 - S, 64 - S, PLACED_NI - 2)
        u = np.empty((len(places), PLACED_NI), F)
        for i, at in enumerate(places):
            below = np.sort(rng.uniform(0, ua, at)).astype(F)
            above = np.sort(rng.uniform(ub, 1, PLACED_NI - 2 - at)).astype(F)
            u[i] = np.concatenate([below[below < ua], [ua] * int((below >= ua).sum()), [ua, ub], [ub] * int((above <= ub).sum()), above[above > ub]])
        n = len(places)
        placed = dict(name=f"{S}+{PLACED_NI} {n} rays, the inverted pair of seed {seed} placed", S=S, Ni=PLACED_NI, R=n, z=np.repeat(b["z"][r:r + 1], n, 0),
                      w=np.repeat(b["w"][r:r + 1], n, 0), u=u, patterns=(b["patterns"][r],) * n, aimed=False, third_path=True, placed=places)
        out += [b, placed]
    return out


_ref_cache = {}


def reference(batch):
    """The restatement of one batch, computed once: dict(samples, unit, sorted)."""
    key = batch["name"]
    if key not in _ref_cache:
        s, unit = resample(batch["z"], batch["w"], batch["u"])
        for a in (s, unit):
            a.setflags(write=False)
        _ref_cache[key] = dict(samples=s, unit=unit, sorted=non_decreasing(s))
    return _ref_cache[key]


def finite_rows(batch):
    return np.isfinite(batch["w"][:, 1:batch["S"] - 1]).all(-1)


def search_sorted_u_unsorted_samples(n_rays=2000, seed=77, z_kinds=("rows", "rows", "repeated"), sample_counts=(5, 17, 66, 131)):
    """How many of ``n_rays`` aimed, finite rays have sorted ``u`` and samples that are NOT non-decreasing (see the module's docstring)."""
    rng = np.random.default_rng(seed)
    found = done = 0
    while done < n_rays:
        S = int(rng.choice(sample_counts))
        Ni = int(rng.choice([2, 64, 200]))
        b = build("search", S, Ni, list(FINITE), str(rng.choice(z_kinds)), "aimed_sorted", int(rng.integers(1 << 30)))
        found += int((~non_decreasing(resample(b["z"], b["w"], b["u"])[0])).sum())
        done += b["R"]
    return found, done

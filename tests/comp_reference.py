"""Plain fp64 restatement of raw2outputs (models/render_class.py:440-482) and of its analytic backward (tests only): NumPy, no call into
the library.  Next to every result stands a per-element first-order bound E on the error of an fp32 evaluation of the same formula, and
the comparison of tests/test_gpu_composite.py is  |got - ref| <= C * E + TINY  on EVERY element (NaN must meet NaN).

The backward is the formula above k_composite_backward:  dL/dalpha_j = G_j T_j - (sum_{i>j} G_i w_i) / (1 - alpha_j + 1e-10),  with
G_i = dL/dw_i collected from rgb, depth, acc, disp and the explicit weights gradient, the white-background term folded into g_acc.

The bound chain (U = 2^-24, n = S/64 + 8 roundings allowed to a sum, every E absolute):
  x = relu(sigma) dist, e = exp(-x), a = 1 - e, m = e + 1e-10, T = exclusive product of m, w = a T
  ca      = min(U, e) + U e (3 x + 2)         an fp32 1 - expf(-x), including its rounding to exactly 1 once e < U/2
  relm    = U + ca / m,  kappa_i = sum_{k<i} (relm_k + U)
  EW      = w (kappa + 2U) + T ca
  Esum(v) = sum(EW |v|) + n U sum(w |v|)      (+ 3U for the fp32 sigmoid where v is a colour)
  EG      = 3U sum|g_c| c + E(g_depth') z + E(g_acc') + 6U Gabs
  EA_j    = sum_{i>j} (EG_i w_i + |G_i| EW_i) + n U sum_{i>j} |G_i w_i|
  Edalpha = EG T + |G| T (kappa + U) + EA / m + |A| / m (relm + 2U) + 2U (|G| T + |A| / m)
  Edsigma = [sigma > 0] (Edalpha dist e + (|G| T + |A| / m) dist (ca + 4U e))
  E(d_raw rgb) = EW |g_c| c (1 - c) + U w |g_c| c (2 + 8 (1 - c))     c (1 - c) of an fp32 sigmoid: 1 - c is no better than c
  E(d_rays_d)  = the Edsigma pieces with relu(sigma) dlt in place of dist, + n U sum|terms|, times |d_a| / |d|  (+ 5U |value|)
TINY = 8 * 2^-126: fp32 results below the smallest normal lose relative precision or are flushed.

MEASURED (the inputs are make_batch's, all nine sample counts, noise / white background / shared z on and off):
  the restatement against fp64 autograd through oracle.raw2outputs: 1.7e-15 of each tensor's scale
  the reference's own fp32 arithmetic (oracle.raw2outputs in torch.float32 with torch autograd, on the CPU), worst |err| / (E + TINY):
    weights 1.00, rgb 0.16, acc 0.14, depth 0.15, disp 0.05, d_raw rgb 1.00, d_raw sigma 0.97, d_rays_d 0.08
  The 1.00 is attained, not approached: where fp32 rounds alpha to exactly 1 and fp64 does not, err = e T = E.  None of these elements is
  subnormal.  With an allowance of 8U w |g_c| c (1 - c) for the sigmoid the colour channels of d_raw gave 2.45 (S = 2, c = 0.954, w = 1,
  value 1.8e-2: 1 - c has c's absolute error, not (1 - c)'s relative one), hence the term above; with it that element gives 0.46.
  C = 4.0 is four times the worst ratio: the device's expf differs from the host's by a few ulp and it multiplies and adds in tree order.
  the device (MI355X, mofa_composite_forward / mofa_composite_backward over the 72 cases of tests/test_gpu_composite.py), worst ratio:
    weights 1.00, rgb 0.18, acc 0.18, depth 0.18, disp 0.06, d_raw rgb 1.00, d_raw sigma 1.00, d_rays_d 1.00
  (1.00 again where alpha is exactly 1 in fp32: the backward's keep = 1 - alpha is then 0, and err = |value| = E.)
"""
import numpy as np

U = 2.0 ** -24
TINY = 8 * 2.0 ** -126
C = 4.0                  # |got - ref| <= C * E + TINY: four times the worst ratio of the reference's own fp32 arithmetic (see MEASURED)

SAMPLE_COUNTS = (2, 3, 64, 65, 128, 129, 256, 257, 513)
X_OPAQUE = 60.0          # exp(-60) = 9e-27: fp32 and fp64 agree that 1 - alpha + 1e-10 is 1e-10


def n_sum(S):
    return S / 64.0 + 8.0


def _excl_prefix(a, op):
    """exclusive running sum / product along the last axis"""
    first = np.zeros_like(a[..., :1]) if op is np.cumsum else np.ones_like(a[..., :1])
    return np.concatenate([first, op(a, -1)[..., :-1]], -1)


def _excl_suffix_sum(a):
    """out_j = sum_{i > j} a_i, summed from the back (no subtraction: a_j may be 1e10 times what lies behind it)"""
    incl = np.cumsum(a[..., ::-1], -1)[..., ::-1]
    return np.concatenate([incl[..., 1:], np.zeros_like(a[..., :1])], -1)


class Forward:
    """Values (fp64) and bounds of raw2outputs.  raw [R,S,4], z [R,S] or a shared row [S], rays_d [R,3], noise [R,S] or None."""

    def __init__(self, raw, z, rays_d, noise=None, white=False):
        raw, z, d = np.asarray(raw, np.float64), np.asarray(z, np.float64), np.asarray(rays_d, np.float64)
        R, S = raw.shape[:2]
        z = np.broadcast_to(z, (R, S))
        self.R, self.S, self.white, self.z, self.d = R, S, bool(white), z, d
        n = self.n = n_sum(S)
        self.dnorm = np.sqrt((d * d).sum(-1))
        self.dlt = np.concatenate([z[:, 1:] - z[:, :-1], np.full((R, 1), 1e10)], -1)
        self.dist = dist = self.dlt * self.dnorm[:, None]
        self.sg = sg = raw[..., 3] + (0.0 if noise is None else np.asarray(noise, np.float64))
        self.x = x = np.maximum(sg, 0.0) * dist
        self.e = e = np.exp(-x)
        self.a = a = 1.0 - e                                      # as raw2outputs forms it: 1e-16 absolute, against a bound of 3U T
        self.m = m = e + 1e-10
        self.T = T = _excl_prefix(m, np.cumprod)
        self.w = w = a * T
        self.c = c = 1.0 / (1.0 + np.exp(-raw[..., :3]))
        self.ca = ca = np.minimum(U, e) + U * e * (3.0 * x + 2.0)
        self.relm = relm = U + ca / m
        self.kappa = kappa = _excl_prefix(relm + U, np.cumsum)
        self.EW = EW = w * (kappa + 2 * U) + T * ca

        def esum(v):
            return (EW * np.abs(v)).sum(-1) + n * U * (w * np.abs(v)).sum(-1)

        self.acc, self.Eacc = w.sum(-1), esum(np.ones_like(w))
        self.depth, self.Edepth = (w * z).sum(-1), esum(z)
        self.rgb = (w[..., None] * c).sum(1)
        self.Ergb = np.stack([esum(c[..., k]) + 3 * U * (w * c[..., k]).sum(-1) for k in range(3)], -1)
        if white:
            self.rgb = self.rgb + (1.0 - self.acc)[:, None]
            self.Ergb = self.Ergb + self.Eacc[:, None] + 2 * U * (np.abs(1.0 - self.acc)[:, None] + np.abs(self.rgb))
        self.live = live = self.acc > 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            q = self.depth / self.acc                                               # 0/0 -> NaN, and max() propagates it
            self.disp = np.where(live, 1.0 / np.maximum(1e-10, q), np.nan)
            Eq = self.Edepth / self.acc + self.depth * self.Eacc / self.acc ** 2 + U * np.abs(q)
            self.Edisp = np.where(live, Eq / q ** 2 + 2 * U * np.abs(self.disp), 0.0)


def backward(F, g_rgb, g_disp=None, g_acc=None, g_depth=None, g_weights=None):
    """-> d_raw [R,S,4], E(d_raw), d_rays_d [R,3], E(d_rays_d).  An absent gradient is zero.  A ray with acc == 0 and g_disp != 0 is NaN
    wherever the chain rule multiplies through 0/0: d_rays_d, and d_raw[..., 3] where sigma > 0 (nowhere, on such a ray)."""
    R, S, n = F.R, F.S, F.n
    zero = np.zeros(R)
    g_rgb = np.asarray(g_rgb, np.float64)
    g_disp, g_acc, g_depth = (zero if g is None else np.asarray(g, np.float64) for g in (g_disp, g_acc, g_depth))
    g_w = np.zeros((R, S)) if g_weights is None else np.asarray(g_weights, np.float64)
    w, T, m, e, c, z, EW = F.w, F.T, F.m, F.e, F.c, F.z, F.EW
    with np.errstate(invalid="ignore", divide="ignore"):
        t_d = np.where(F.live, -F.acc / F.depth ** 2, 0.0)                          # d disp / d depth, d disp / d acc  (disp = acc / depth)
        t_a = np.where(F.live, 1.0 / F.depth, 0.0)
        Et_d = np.where(F.live, F.Eacc / F.depth ** 2 + 2 * F.acc * F.Edepth / np.abs(F.depth) ** 3 + 3 * U * np.abs(t_d), 0.0)
        Et_a = np.where(F.live, F.Edepth / F.depth ** 2 + 2 * U * np.abs(t_a), 0.0)
    poison = np.where(~F.live & (g_disp != 0.0), np.nan, 0.0)
    gdep = g_depth + g_disp * t_d + poison
    gacc = g_acc + g_disp * t_a + poison
    Egdep = np.abs(g_disp) * Et_d + 2 * U * (np.abs(g_depth) + np.abs(g_disp * t_d))
    Egacc = np.abs(g_disp) * Et_a + 2 * U * (np.abs(g_acc) + np.abs(g_disp * t_a))
    if F.white:
        gacc = gacc - g_rgb.sum(-1)
        Egacc = Egacc + 4 * U * np.abs(g_rgb).sum(-1)
    gc = (g_rgb[:, None, :] * c).sum(-1)
    gc_abs = (np.abs(g_rgb)[:, None, :] * c).sum(-1)
    G = g_w + gc + gdep[:, None] * z + gacc[:, None]
    Gabs = np.abs(g_w) + gc_abs + np.abs(gdep)[:, None] * np.abs(z) + np.abs(gacc)[:, None]
    EG = 3 * U * gc_abs + Egdep[:, None] * np.abs(z) + Egacc[:, None] + 6 * U * Gabs
    A = _excl_suffix_sum(G * w)
    EA = _excl_suffix_sum(EG * w + np.abs(G) * EW) + n * U * _excl_suffix_sum(np.abs(G * w))
    GT, Am = np.abs(G) * T, np.abs(A) / m
    dalpha = G * T - A / m
    Edalpha = EG * T + GT * (F.kappa + U) + EA / m + Am * (F.relm + 2 * U) + 2 * U * (GT + Am)
    pos = F.sg > 0.0
    d_raw, E_raw = np.zeros((R, S, 4)), np.zeros((R, S, 4))
    d_raw[..., 3] = np.where(pos, dalpha * F.dist * e, 0.0)
    E_raw[..., 3] = np.where(pos, Edalpha * F.dist * e + (GT + Am) * F.dist * (F.ca + 4 * U * e), 0.0)
    d_raw[..., :3] = w[..., None] * g_rgb[:, None, :] * c * (1.0 - c)
    # c = 1 / (1 + expf(-v)): the add and the divide give 2U c, an expf good to 2 ulp 4U c (1 - c); 1 - c inherits that ABSOLUTE error, so
    # c (1 - c) carries U c (2 + 4 (1 - c)) + 2U c (1 - c), and the two multiplications by w and g_c another 2U c (1 - c)
    E_raw[..., :3] = np.abs(g_rgb)[:, None, :] * (EW[..., None] * c * (1.0 - c) + U * w[..., None] * c * (2.0 + 8.0 * (1.0 - c)))
    rs = np.maximum(F.sg, 0.0)
    terms = dalpha * rs * e * F.dlt                                                  # d L / d |rays_d|, sample by sample
    dn = terms.sum(-1)
    Edn = (Edalpha * rs * F.dlt * e + (GT + Am) * rs * F.dlt * (F.ca + 4 * U * e)).sum(-1) + n * U * np.abs(terms).sum(-1)
    unit = F.d / F.dnorm[:, None]
    d_rd = dn[:, None] * unit
    E_rd = Edn[:, None] * np.abs(unit) + 5 * U * np.abs(d_rd)
    return d_raw, E_raw, d_rd, E_rd


# ---- the comparison -------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, E):
    """worst |got - ref| / (E + TINY) over the elements; inf where the NaN patterns differ"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    nan = np.isnan(ref)
    if (np.isnan(got) != nan).any():
        return float("inf")
    r = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, ref)) / (np.where(nan, 0.0, E) + TINY))
    return float(r.max())


def assert_inside(got, ref, E, what, c=None):
    """EVERY element of got within C * E + TINY of ref, NaN exactly where ref is NaN; returns the worst |err| / (E + TINY)."""
    c = C if c is None else c
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), f"{what}: NaN pattern differs ({int(np.isnan(got).sum())} NaN, want {int(nan.sum())})"
    err = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, ref)))
    lim = c * np.where(nan, 0.0, E) + TINY
    bad = ~(err <= lim)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements over the bound, worst err / bound = {float((err / lim).max()):.3e} "
                           f"at {np.unravel_index(int(np.argmax(err / lim)), err.shape)}")
    return ratio(got, ref, E)


# ---- the inputs: one batch per sample count ---------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def make_batch(S, noise=False, shared_z=False):
    """Explicit rays for S samples, the same on every run (seeded by S).  Every family states x = sigma * dist, and each sigma is set from
    the ray's actual fp32 dist.  fp32 arrays: raw [R,S,4], z [R,S] or [S], rays_d [R,3], noise [R,S] or None, the five upstream gradients
    g_rgb / g_disp / g_acc / g_depth / g_weights; `z_rows` [R,S] are the per-ray rows (z is z_rows[0] when shared); `family` names each ray; `behind_run` [R,S] marks the samples behind the long opaque run.
    The ray count is odd, so the last block of four rays is never full."""
    rng = np.random.default_rng(7000 + S)
    fam, rows = [], []                                           # per ray: the family's name, a function (dist [S]) -> sigma [S]

    def neg(k):
        return -rng.uniform(0.05, 3.0, k)

    def thin(dist):
        return 10.0 ** rng.uniform(-6, -3, S) / dist

    def moderate(dist):
        return rng.normal(0, 1.2, S)

    def empty(dist):
        return neg(S)

    def zero(dist):
        return np.zeros(S)

    def surface(p, k):
        def f(dist):
            s = neg(S)
            small = rng.uniform(size=S) < 0.3
            s[small] = (10.0 ** rng.uniform(-3, -1, S) / dist)[small]
            if p >= 1:
                s[p - 1] = 0.05 / dist[p - 1]                    # the sample in front of a surface always sees it
            s[p:p + k] = X_OPAQUE / dist[p:p + k]
            s[p + k:] = rng.normal(0, 1.2, S - p - k)
            return s
        return f

    def nearly_opaque(dist):
        s = neg(S)
        at = rng.choice(S, min(6, S), replace=False)
        s[at] = rng.uniform(3, 20, at.size) / dist[at]
        return s

    def last_only(dist):
        s = neg(S)
        s[-1] = 1e-9
        return s

    run0 = S // 3

    def long_run(dist):
        s = rng.normal(0, 1.2, S)
        s[run0:run0 + 8] = X_OPAQUE / dist[run0:run0 + 8]
        return s

    for name, f in (("thin", thin), ("thin", thin), ("moderate", moderate), ("moderate", moderate), ("moderate", moderate),
                    ("moderate", moderate), ("empty", empty), ("empty", empty), ("zero", zero)):
        fam.append(name), rows.append(f)
    places = sorted({p for p in (0, 1, S // 2, 63, 64, 127, 128, 255, 256) if p < S})
    for k in (1, 2, 3):
        for p in sorted(set(places) | {q for q in (S - 1 - k, S - 1) if q >= 0}):
            if p + k <= S:
                fam.append(f"surface p={p} k={k}"), rows.append(surface(p, k))
    for name, f in (("nearly opaque", nearly_opaque), ("nearly opaque", nearly_opaque), ("last only", last_only)):
        fam.append(name), rows.append(f)
    if S >= 64:
        fam.append("long opaque run"), rows.append(long_run)
    if len(rows) % 2 == 0:
        fam.append("moderate"), rows.append(moderate)
    R = len(rows)

    z = _f32(8.0 + 18.0 * (np.arange(S)[None, :] + 0.8 * rng.uniform(size=(R, S))) / S)   # strictly increasing, dlt >= 0.2 * 18 / S
    d = _f32(rng.normal(size=(R, 3)) + np.where(rng.uniform(size=(R, 3)) < 0.5, 0.4, -0.4))
    nz = _f32(rng.uniform(-0.5, 0.5, (R, S)))
    raw = _f32(rng.normal(0, 1.2, (R, S, 4)))
    zz = z[0] if shared_z else z
    zr = np.broadcast_to(zz, (R, S))
    dnorm = np.sqrt((d * d).sum(-1, dtype=np.float32), dtype=np.float32)
    dlt = np.concatenate([zr[:, 1:] - zr[:, :-1], np.full((R, 1), 1e10, np.float32)], -1).astype(np.float32)
    dist = (dlt * dnorm[:, None]).astype(np.float64)
    behind = np.zeros((R, S), bool)
    for r in range(R):
        sigma = _f32(rows[r](dist[r]))
        if fam[r] not in ("moderate", "empty"):
            nz[r, -1] = 0.0                                      # a sigma of 1e-9 .. 1e-17 at the 1e10 distance does not survive an added noise
        if fam[r] == "zero":
            raw[r, :, 3] = -nz[r] if noise else 0.0              # raw + noise == 0 exactly
        else:
            raw[r, :, 3] = sigma - nz[r] if noise else sigma
        if fam[r] == "long opaque run":
            behind[r, run0 + 8:] = True
    g = {k: _f32(rng.normal(size=sh)) for k, sh in (("g_rgb", (R, 3)), ("g_disp", (R,)), ("g_acc", (R,)), ("g_depth", (R,)),
                                                     ("g_weights", (R, S)))}
    return dict(S=S, R=R, raw=raw, z=_f32(zz), z_rows=z, rays_d=d, noise=nz if noise else None, family=fam, behind_run=behind, **g)

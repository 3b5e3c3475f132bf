"""Plain fp64 restatements of the backward kernels' arithmetic (tests only): the panel layout, the mask-only tape's bit layout, one
function per operation of the backward C ABI, and next to every result the conditioning term sum |a b| of the same contraction, which is
what the rounding-level bound of tests/test_gpu_bwd_kernels.py is stated in.  torch only (any device), no call into the library; the CPU
file tests/test_bwd_reference_cpu.py shows that every fault these comparisons are meant to see does break the bound."""
import torch

C_CONTRACTION = 1e-6      # |got - ref64| <= C * sum |a b| + TINY per element: an fp32 FMA chain (test_layer0_positional_encoding_fused's constant);
TINY = 1e-30              # a random contraction is expected near 2^-24 sum |a b| = 6e-8, so C leaves about an order of magnitude
U32 = 2.0 ** -24          # unit roundoff of fp32
# The positional-encoding backward adds C_PE * U32 * sum_f 2^f (|g_sin| + |g_cos|) for the device sincosf at arguments up to 2^9 |x|.
# Measured on MI355X over the cases of tests/test_gpu_bwd_kernels.py::test_pe_backward_and_panels: worst |err| / (U32 * that sum) = 1.953
# (d_pts, n_freqs = 4, 9 x 130 samples; the summed ray outputs stay below 0.38); the constant is 4x that ratio, because the sin / cos
# error varies with the argument.  (The contraction term alone already covered every error of that run.)
C_PE = 7.8
ROW_TILE = 256


def round_up(v, m):
    return (v + m - 1) // m * m


# ---- panel layout: a matrix [rows, K] is K/16 panels of [rows][16] floats, 4-float chunks swizzled by the row ------------------------------
def panel_offset(rows, row, k):
    """Float offset of element (row, k) in a panel buffer of `rows` rows (include/mofanerf_hip.h, "Panel layout"); ints or tensors."""
    return (k // 16) * rows * 16 + row * 16 + ((((k % 16) // 4) ^ ((row // 4) % 4)) * 4) + k % 4


def _swizzle(t):
    """[R, P, 4, 4] (row, panel, chunk, element): chunk c of row r <-> chunk c ^ ((r >> 2) & 3).  Its own inverse."""
    R = t.shape[0]
    sw = (torch.arange(R, device=t.device) // 4) % 4
    idx = torch.arange(4, device=t.device)[None, :] ^ sw[:, None]                      # [R, 4]
    return torch.gather(t, 2, idx[:, None, :, None].expand_as(t))


def pack_panels(x, rows_padded, k_padded=None, row_fill=0.0, col_fill=0.0):
    """Logical [rows, k] -> flat panel buffer [k_padded / 16][rows_padded][16]; rows >= rows hold row_fill, columns >= k col_fill."""
    rows, k = x.shape
    kp = round_up(k, 16) if k_padded is None else k_padded
    full = torch.full((rows_padded, kp), float(col_fill), dtype=x.dtype, device=x.device)
    full[rows:, :] = row_fill
    full[:rows, :k] = x
    return _swizzle(full.reshape(rows_padded, kp // 16, 4, 4)).permute(1, 0, 2, 3).reshape(-1).contiguous()


def unpack_panels(p, rows_padded, k_padded):
    """Flat panel buffer -> logical [rows_padded, k_padded] (inverse of pack_panels)."""
    t = p.reshape(k_padded // 16, rows_padded, 4, 4).permute(1, 0, 2, 3)
    return _swizzle(t).reshape(rows_padded, k_padded).contiguous()


def swap_chunk_with_neighbour(p, rows_padded, row, k):
    """A copy of panel buffer p with the 4-float chunk that holds (row, k) exchanged with its swizzle neighbour (chunk ^ 1)."""
    q = p.clone()
    a = panel_offset(rows_padded, row, k - k % 4)
    b = panel_offset(rows_padded, row, (k - k % 4) ^ 4)
    q[a:a + 4], q[b:b + 4] = p[b:b + 4], p[a:a + 4]
    return q


# ---- mask-only tape: float offset o of a panel buffer <-> bit ((o & 255) >> 2) of 64-bit word (o >> 8) * 4 + (o & 3) -------------------------
def mask_bit_position(o):
    return (o >> 8) * 4 + (o & 3), (o & 255) >> 2


def mask_bits(flags):
    """flags: bool per float offset of a panel buffer (a multiple of 256 long) -> int64 words of the mask-only tape."""
    f = flags.reshape(-1, 64, 4).to(torch.int64)                                       # [block, bit, word]
    return (f << torch.arange(64, device=f.device, dtype=torch.int64)[None, :, None]).sum(1).reshape(-1).contiguous()


def mask_flags(words):
    """int64 words -> bool per float offset (inverse of mask_bits)."""
    w = words.reshape(-1, 1, 4)
    return (((w >> torch.arange(64, device=w.device, dtype=torch.int64)[None, :, None]) & 1) != 0).reshape(-1)


# ---- how mofa_weight_grad splits the points (wg_plan / wg_split / wg_split_rows, csrc/mofa_bwd.hip and csrc/mofa_common.h) ----------------
def wg_plan(n_points, n_padded, k_padded):
    tn = 128 if n_padded % 128 == 0 else 64
    tk = 256 if (tn == 128 and k_padded % 256 == 0) else (128 if k_padded % 128 == 0 else 64)
    out_tiles = (n_padded // tn) * (k_padded // tk)
    m_tiles = (n_points + ROW_TILE - 1) // ROW_TILE
    mpx = (m_tiles + 7) // 8
    want = max(1, (128 + out_tiles - 1) // out_tiles)
    spt = max(1, (mpx + want - 1) // want)
    nspx = (mpx + spt - 1) // spt
    full, rem = divmod(m_tiles, mpx)
    total = full * nspx + (rem + spt - 1) // spt
    splits = []
    for s in range(total):
        x, j = divmod(s, nspx)
        first = x * mpx + j * spt
        end = min(first + spt, min((x + 1) * mpx, m_tiles))
        splits.append((first, end - first))                                            # row tiles [first, first + count)
    return dict(tn=tn, tk=tk, m_tiles=m_tiles, mpx=mpx, spt=spt, nspx=nspx, total=total, splits=splits)


# ---- the operations: (result, sum |a b|) in fp64 ------------------------------------------------------------------------------------------
def weight_grad(g, x, n_points):
    """dW = G^T X over the first n_points rows and db = sum_m G: (dW [N, K], cond_dW, db [N], cond_db)."""
    g, x = g[:n_points].double(), x[:n_points].double()
    return g.T @ x, g.abs().T @ x.abs(), g.sum(0), g.abs().sum(0)


def backward_data(g, w, dx_old=None, mask=None, accumulate=False):
    """dX = (dX_old * accumulate + G W) * (mask > 0) — accumulate first, then mask.  g [M, N], w [N, K] (the forward weight block)."""
    g, w = g.double(), w.double()
    val, cond = g @ w, g.abs() @ w.abs()
    if accumulate:
        val, cond = val + dx_old.double(), cond + dx_old.double().abs()
    if mask is not None:
        val = torch.where(mask > 0, val, torch.zeros_like(val))
    return val, cond


def head_backward(d_raw, raw_off, n_out, w, n_points, m_padded, dx_old=None, mask=None, accumulate=False):
    """Head backward: rows < n_points get d_raw[:, off:off+n_out] @ w (w [n_out, K]), rows beyond contribute zero; then as backward_data."""
    g = torch.zeros(m_padded, n_out, dtype=torch.float64, device=w.device)
    g[:n_points] = d_raw[:n_points, raw_off:raw_off + n_out].double()
    return backward_data(g, w, dx_old, mask, accumulate)


def head_weight_grad(d_raw, raw_off, n_out, x, n_points):
    g, x = d_raw[:n_points, raw_off:raw_off + n_out].double(), x[:n_points].double()
    return g.T @ x, g.abs().T @ x.abs()


def bias_grad_rays(g, n_rays, S):
    g = g[:n_rays * S].double().reshape(n_rays, S, -1)
    return g.sum(1), g.abs().sum(1)


def points_from_rays(o, d, z):
    """The fp32 points o + d z with the multiply and the add rounded separately, as the kernels form them: [n_rays * S, 3]."""
    assert o.dtype == d.dtype == z.dtype == torch.float32
    prod = d[:, None, :] * z[:, :, None]
    return (o[:, None, :] + prod).reshape(-1, 3)


def pe_features(x, n_freqs):
    """[x, sin(2^0 x), cos(2^0 x), sin(2^1 x), ...] of fp32 points x [M, 3] in fp64 (2^f x is exact in fp32)."""
    x = x.double()
    out = [x]
    for f in range(n_freqs):
        out += [torch.sin(x * 2.0 ** f), torch.cos(x * 2.0 ** f)]
    return torch.cat(out, -1)


def pe_panels(x, n_freqs, m_padded, k_padded):
    """mofa_pe_panels as a logical matrix [m_padded, k_padded]: the features of the points, zero in the padding rows and features."""
    out = torch.zeros(m_padded, k_padded, dtype=torch.float64, device=x.device)
    out[:x.shape[0], :3 + 6 * n_freqs] = pe_features(x, n_freqs)
    return out


def pe_point_backward(dpe, x, n_freqs):
    """gx = g_id + sum_f 2^f (g_sin cos(2^f x) - g_cos sin(2^f x)) per point: (gx [M, 3], sum |terms|, sum_f 2^f (|g_sin| + |g_cos|))."""
    x, dpe = x.double(), dpe[:x.shape[0]].double()
    gx, cond, trig = dpe[:, 0:3].clone(), dpe[:, 0:3].abs(), torch.zeros_like(x)
    for f in range(n_freqs):
        fr = 2.0 ** f
        gs, gc = dpe[:, 3 + 6 * f:6 + 6 * f], dpe[:, 6 + 6 * f:9 + 6 * f]
        sn, cs = torch.sin(x * fr), torch.cos(x * fr)
        gx = gx + fr * (gs * cs - gc * sn)
        cond = cond + fr * ((gs * cs).abs() + (gc * sn).abs())
        trig = trig + fr * (gs.abs() + gc.abs())
    return gx, cond, trig


def pe_ray_backward(dpe, o, d, z, n_freqs):
    """d_rays_o = sum_s gx, d_rays_d = sum_s gx z over the fp32 points of every ray: ((d_o, cond, trig), (d_d, cond, trig))."""
    R, S = z.shape
    gx, cond, trig = (t.reshape(R, S, 3) for t in pe_point_backward(dpe, points_from_rays(o, d, z), n_freqs))
    zz = z.double()[:, :, None]
    return (gx.sum(1), cond.sum(1), trig.sum(1)), ((gx * zz).sum(1), (cond * zz.abs()).sum(1), (trig * zz.abs()).sum(1))


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------------
def bound(cond, trig=None, c=C_CONTRACTION):
    b = c * cond + TINY
    return b if trig is None else b + C_PE * U32 * trig


def worst_ratio(got, ref, cond):
    """max over the elements of |got - ref| / sum |a b| (elements whose conditioning term is zero must be exact)."""
    err = (got.double() - ref).abs()
    return float((err / cond.clamp_min(1e-300)).max()) if err.numel() else 0.0


def exceeds(got, ref, lim):
    """Does any element of `got` miss the bound?  (NaN counts as a miss.)"""
    err = (got.double() - ref).abs()
    return bool((~(err <= lim)).any())


def assert_close(got, ref, cond, what, trig=None):
    """EVERY element of got within bound(cond, trig) of the fp64 reference; prints and returns the worst err / sum |a b|."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    lim = bound(cond, trig)
    err = (got.double() - ref).abs()
    ratio = worst_ratio(got, ref, cond)
    print(f"{what}: worst err / sum|ab| = {ratio:.3e}")
    bad = ~(err <= lim)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements over the bound, worst err / bound = {float((err / lim)[bad].nan_to_num(float('inf')).max()):.3e}"
    return ratio

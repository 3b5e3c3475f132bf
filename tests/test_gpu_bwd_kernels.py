"""The backward kernels one by one, through the C ABI, against the fp64 restatements of tests/bwd_reference.py.

Every operation here is linear in its inputs with the mask given, so it is held to a rounding-level bound, per element and for EVERY
element: |got - ref64| <= 1e-6 * sum |a b| + tiny for the contractions (bwd_reference.C_CONTRACTION), plus a term for the device's
sincosf in the positional-encoding backward (bwd_reference.C_PE).  Inputs are asymmetric random; every output sits between two guard
regions that must come back bit-identical and is pre-filled with a sentinel; padding rows (m >= n_points) of the input panels hold large
finite values; every call runs twice and must repeat bit for bit.  tests/test_bwd_reference_cpu.py shows on the CPU that a dropped point,
a dropped split, exchanged operands, a shifted column offset, one mask bit, one swizzled chunk and a wrong accumulate / mask order each
break these bounds.  Each test prints its worst err / sum |a b|."""
import numpy as np
import pytest
import torch

import bwd_reference as br
from mofanerf_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e11          # guard regions and never-written outputs
BIG = 3e30               # padding rows of input panels: finite, and ruinous if a kernel lets them through


def L():
    return lib.load()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, device=DEV) * scale


def _mask_like(gen, *shape):
    """a saved activation: negative values, positive values and exact zeros (the mask is > 0, not >= 0)"""
    m = _randn(gen, *shape)
    m[torch.rand(*shape, generator=gen, device=DEV) < 0.1] = 0.0
    return m


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class Guarded:
    """n elements between two guard regions (each at least `guard` elements: a row tile / one ld row); .out is what the kernel gets."""

    def __init__(self, n, guard=4096, fill=float("nan"), dtype=torch.float32):
        self.n, self.g = n, br.round_up(max(guard, 4096), 64)
        self.sent = SENT if dtype == torch.float32 else 0x5A5A5A5A5A5A5A5A
        self.buf = torch.full((n + 2 * self.g,), self.sent, dtype=dtype, device=DEV)
        self.out = self.buf[self.g:self.g + n]
        self.out.fill_(fill)

    def set(self, values):
        self.out.copy_(values.reshape(-1))
        return self

    def ptr(self):
        return self.out.data_ptr()

    def check(self):
        want = torch.full((self.g,), self.sent, dtype=self.buf.dtype, device=DEV)
        assert _same_bits(self.buf[:self.g], want) and _same_bits(self.buf[self.g + self.n:], want), "a guard region was written"
        return self.out


def _twice(run):
    """run() -> tuple of output tensors (fresh buffers each time): both runs bit for bit the same; returns the first"""
    a, b = run(), run()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert _same_bits(x, y), "two runs differ"
    return a


# ---- mofa_weight_grad ---------------------------------------------------------------------------------------------------------------------
WG_VARIANTS = {(256, 512): (128, 256), (128, 384): (128, 128), (128, 192): (128, 64), (192, 128): (64, 128), (192, 192): (64, 64)}


def _weight_grad(N, K, n, seed, n_out=None, ncols=None, ld=None, col0=0, tiles=None, splits=None):
    """One mofa_weight_grad call checked in full: dW (every element of the [n_out, ncols] block, nothing outside it), db over all N
    columns, the same dW with bias_out = NULL, the split count the workspace query implies."""
    n_out, ncols, ld = n_out or N, ncols or K, ld or K
    gen = _gen(seed)
    Mp = br.round_up(n, 256)
    g, x = _randn(gen, n, N), _randn(gen, n, K)
    gp, xp = br.pack_panels(g, Mp, row_fill=BIG), br.pack_panels(x, Mp, row_fill=-BIG)
    plan = br.wg_plan(n, N, K)
    ws_floats = L().mofa_weight_grad_workspace_floats(n, N, K)
    assert ws_floats == plan["total"] * N * (K + 1), (ws_floats, plan)
    if tiles is not None:
        assert (plan["tn"], plan["tk"]) == tiles, plan
    if splits is not None:
        assert plan["total"] == splits, plan
    st = lib.stream()

    def run(with_bias=True):
        ws = Guarded(ws_floats)                       # NaN: a partial the first stage left out shows in the second
        dst, db = Guarded(N * ld, guard=ld, fill=SENT), Guarded(N, fill=SENT)
        lib.check(L().mofa_weight_grad(lib.ptr(gp), N, lib.ptr(xp), K, Mp, n, n_out, ncols, dst.ptr(), ld, col0,
                                       db.ptr() if with_bias else None, ws.ptr(), st), "weight_grad")
        torch.cuda.synchronize()
        ws.check()
        return dst.check().reshape(N, ld), db.check()

    dst, db = _twice(run)
    dst_nb, db_nb = run(False)
    assert _same_bits(dst_nb, dst) and (db_nb == SENT).all()           # bias_out = NULL: the same dW, bias_out's place untouched
    dw, cond, dbr, cond_b = br.weight_grad(g, x, n)
    what = f"weight_grad {N}x{K} <{plan['tn']},{plan['tk']}> n={n} splits={plan['total']}"
    br.assert_close(dst[:n_out, col0:col0 + ncols], dw[:n_out, :ncols], cond[:n_out, :ncols], what + " dW")
    br.assert_close(db, dbr, cond_b, what + " db")
    outside = dst.clone()
    outside[:n_out, col0:col0 + ncols] = SENT
    assert (outside == SENT).all(), "dst written outside rows < n_out, columns [col0, col0 + ncols)"
    return dst, db


@pytest.mark.parametrize("n", [112, 256 * 9 - 5, 256 * 17])
@pytest.mark.parametrize("N,K", list(WG_VARIANTS))
def test_weight_grad_every_tile_variant(N, K, n):
    """The five k_wgrad<TN,TK> instantiations (wg_plan picks them by shape) x one row tile / a short last XCD range with the batch
    ending inside a 16- and a 32-point chunk / three tiles per range; one split per row tile (1, 9, 17 splits)."""
    _weight_grad(N, K, n, seed=N + K + n, tiles=WG_VARIANTS[(N, K)], splits=(n + 255) // 256)


@pytest.mark.parametrize("pipe", ["0", "1"])
@pytest.mark.parametrize("n", [16 * 250, 16 * 250 - 5])
def test_weight_grad_pipelined_and_plain_chunk_loop(n, pipe, knob):
    """k_wgrad<128,256>: whole 16-point chunks take the software-pipelined loop, a ragged last chunk the plain one; MOFA_PIPE=0 the plain
    one everywhere."""
    knob("MOFA_PIPE", pipe)
    _weight_grad(256, 512, n, seed=n, tiles=(128, 256), splits=16)


def test_weight_grad_shipped_skip_layer_shape():
    """1024 x 2048 (the fine network's skip layer) at 256 * 17 - 5 points: the one case here where a split holds more than one row tile
    (spt = 2: splits of 2 and 1 tiles in each XCD range, 11 splits)."""
    assert br.wg_plan(256 * 17 - 5, 1024, 2048)["spt"] == 2
    _weight_grad(1024, 2048, 256 * 17 - 5, seed=5, tiles=(128, 256), splits=11)


def test_weight_grad_sub_block_of_a_wider_matrix():
    """n_out = 250, ncols = 500 into dst with ld = 600 at col0 = 37: everything outside rows < n_out, columns [col0, col0 + ncols) untouched."""
    _weight_grad(256, 512, 256 * 9 - 5, seed=6, n_out=250, ncols=500, ld=600, col0=37)


# ---- mofa_pack_panels_t + mofa_layer_backward_data / _bits --------------------------------------------------------------------------------
@pytest.mark.parametrize("Mp", [256, 256 * 5])
@pytest.mark.parametrize("gk,ko", [(64, 64), (48, 128), (256, 384), (1024, 192), (128, 1024)])
def test_backward_data_against_fp64(gk, ko, Mp):
    """dX = (dX_old * accumulate + G W) * (mask > 0) for all four of {accumulate} x {mask}; W is a block of a wider matrix, narrower than
    both paddings (n_out < g_k, ncols < k_out_padded), so the packed transpose must hold zeros there: G is non-zero in every column."""
    gen = _gen(gk + ko + Mp)
    st = lib.stream()
    n_out, ncols, col0 = gk - 3, ko - 35, 13
    ld = ncols + 21
    w = _randn(gen, n_out, ld, scale=gk ** -0.5)
    wt = Guarded(ko * gk)
    lib.check(L().mofa_pack_panels_t(lib.ptr(w), n_out, ld, col0, ncols, wt.ptr(), ko, gk, st), "pack_panels_t")
    torch.cuda.synchronize()
    wl = torch.zeros(gk, ko, device=DEV)
    wl[:n_out, :ncols] = w[:, col0:col0 + ncols]
    assert _same_bits(wt.check(), br.pack_panels(wl.T.contiguous(), ko))          # rows = forward inputs, contraction = forward outputs
    g, old, mask = _randn(gen, Mp, gk), _randn(gen, Mp, ko), _mask_like(gen, Mp, ko)
    gp, oldp, maskp = br.pack_panels(g, Mp), br.pack_panels(old, Mp), br.pack_panels(mask, Mp)
    words = br.mask_bits(maskp > 0)
    worst = 0.0
    for acc in (0, 1):
        for masked in (False, True):
            def run(bits=False):
                dx = Guarded(Mp * ko).set(oldp) if acc else Guarded(Mp * ko)
                if bits:
                    lib.check(L().mofa_layer_backward_data_bits(lib.ptr(gp), gk, wt.ptr(), words.data_ptr(), acc, dx.ptr(), Mp, ko, st), "bwd_bits")
                else:
                    lib.check(L().mofa_layer_backward_data(lib.ptr(gp), gk, wt.ptr(), lib.ptr(maskp) if masked else None, acc, dx.ptr(),
                                                           Mp, ko, st), "bwd")
                torch.cuda.synchronize()
                return (dx.check(),)
            (dx,) = _twice(run)
            ref, cond = br.backward_data(g, wl, old, mask if masked else None, bool(acc))
            worst = max(worst, br.assert_close(br.unpack_panels(dx, Mp, ko), ref, cond, f"backward_data g_k={gk} k_out={ko} Mp={Mp} acc={acc} mask={masked}"))
            if masked:
                assert _same_bits(run(bits=True)[0], dx), "the bit-mask form differs from the float-mask form"
    wt.check()


# ---- mofa_layer_forward_masked ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Np,K", [(128, 64), (192, 64), (128, 48), (64, 64), (128, 32), (128, 1024)])
def test_layer_forward_masked_bits(Np, K):
    """The mask-writing forward (the contiguous-store epilogue at 128 x 64 and 128 x 1024, the pass over y elsewhere — the 64-feature tile, an odd panel
    count, fewer than four panels; tests/test_gpu_fwd_kernels.py repeats the word-for-word check at every shape of its layer test): y bit-identical to
    mofa_layer_forward, every word of mask_bits_out = (y > 0) per the tape's layout, and the bits fed to the backward give what y gives."""
    gen = _gen(Np + K)
    st = lib.stream()
    M, Mp, n_out, k_in = 700, 768, Np - 3, K - 1
    x, w, b = _randn(gen, M, k_in), _randn(gen, n_out, k_in, scale=k_in ** -0.5), _randn(gen, n_out)
    xp = br.pack_panels(x, Mp, k_padded=K, row_fill=0.5)
    wp = br.pack_panels(w, Np, k_padded=K)
    wp_lib = Guarded(Np * K)
    lib.check(L().mofa_pack_panels(lib.ptr(w), n_out, k_in, 0, k_in, wp_lib.ptr(), Np, 0, K, st), "pack_panels")
    torch.cuda.synchronize()
    assert _same_bits(wp_lib.check(), wp)
    bp = torch.zeros(Np, device=DEV)
    bp[:n_out] = b

    def run(masked=True):
        y, bits = Guarded(Mp * Np), Guarded(Mp * Np // 64, dtype=torch.int64, fill=0x33)
        if masked:
            lib.check(L().mofa_layer_forward_masked(lib.ptr(xp), K, None, 0, lib.ptr(wp), lib.ptr(bp), 0, 1, y.ptr(), Mp, Np, 1, bits.ptr(), st), "fwd_masked")
        else:
            lib.check(L().mofa_layer_forward(lib.ptr(xp), K, None, 0, lib.ptr(wp), lib.ptr(bp), 0, 1, y.ptr(), Mp, Np, 1, st), "fwd")
        torch.cuda.synchronize()
        return y.check(), bits.check()

    y, bits = _twice(run)
    assert _same_bits(run(False)[0], y)
    assert torch.equal(bits, br.mask_bits(y > 0))                      # every word, padding rows included
    yl = br.unpack_panels(y, Mp, Np)
    ref = torch.relu(x.double() @ w.double().T + b.double())
    cond = x.double().abs() @ w.double().abs().T + b.double().abs()
    br.assert_close(yl[:M, :n_out], ref, cond, f"layer_forward_masked {Np}x{K}")
    assert (yl[:M, n_out:] == 0).all()
    gk = 64                                                            # dX-shaped buffer = y's shape: k_out_padded = Np
    gp, wt = _randn(gen, Mp * gk), _randn(gen, Np * gk, scale=1 / 8)
    outs = []
    for use_bits in (False, True):
        dx = Guarded(Mp * Np)
        if use_bits:
            lib.check(L().mofa_layer_backward_data_bits(lib.ptr(gp), gk, lib.ptr(wt), bits.data_ptr(), 0, dx.ptr(), Mp, Np, st), "bwd_bits")
        else:
            lib.check(L().mofa_layer_backward_data(lib.ptr(gp), gk, lib.ptr(wt), lib.ptr(y), 0, dx.ptr(), Mp, Np, st), "bwd")
        torch.cuda.synchronize()
        outs.append(dx.check())
    assert _same_bits(outs[0], outs[1]) and not torch.isnan(outs[0]).any()


# ---- heads --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 700])
@pytest.mark.parametrize("kp", [64, 528])
@pytest.mark.parametrize("raw_off,n_out", [(0, 3), (3, 1)])
def test_head_backward_and_weight_grad(raw_off, n_out, kp, n):
    gen = _gen(raw_off + kp + n)
    st = lib.stream()
    Mp = br.round_up(n, 256)
    d_raw = torch.full((Mp, 4), BIG, device=DEV)                       # rows >= n_points are never to be read
    d_raw[:n] = _randn(gen, n, 4)
    w = _randn(gen, n_out, kp, scale=1 / 8)
    old, mask = _randn(gen, Mp, kp), _mask_like(gen, Mp, kp)
    oldp, maskp = br.pack_panels(old, Mp), br.pack_panels(mask, Mp)
    words = br.mask_bits(maskp > 0)
    for acc in (0, 1):
        for masked in (False, True):
            def run(bits=False):
                dx = Guarded(Mp * kp).set(oldp) if acc else Guarded(Mp * kp)
                if bits:
                    lib.check(L().mofa_head_backward_bits(lib.ptr(d_raw), raw_off, n_out, lib.ptr(w), kp, words.data_ptr(), acc, dx.ptr(), Mp, n, st), "head_bwd_bits")
                else:
                    lib.check(L().mofa_head_backward(lib.ptr(d_raw), raw_off, n_out, lib.ptr(w), kp, lib.ptr(maskp) if masked else None, acc,
                                                     dx.ptr(), Mp, n, st), "head_bwd")
                torch.cuda.synchronize()
                return (dx.check(),)
            (dx,) = _twice(run)
            ref, cond = br.head_backward(d_raw, raw_off, n_out, w, n, Mp, old, mask if masked else None, bool(acc))
            br.assert_close(br.unpack_panels(dx, Mp, kp), ref, cond, f"head_backward off={raw_off} n_out={n_out} kp={kp} n={n} acc={acc} mask={masked}")
            if masked:
                assert _same_bits(run(bits=True)[0], dx)
    # the head's weight gradient: ncols < k_padded into a wider dst (ld > ncols)
    x = _randn(gen, n, kp)
    xp = br.pack_panels(x, Mp, row_fill=BIG)
    ncols, ld = kp - 5, kp + 4

    def run_wg():
        dst = Guarded(n_out * ld, guard=ld, fill=SENT)
        lib.check(L().mofa_head_weight_grad(lib.ptr(d_raw), raw_off, n_out, lib.ptr(xp), kp, Mp, n, ncols, dst.ptr(), ld, st), "head_wgrad")
        torch.cuda.synchronize()
        return (dst.check().reshape(n_out, ld),)

    (dst,) = _twice(run_wg)
    dw, cond = br.head_weight_grad(d_raw, raw_off, n_out, x, n)
    br.assert_close(dst[:, :ncols], dw[:, :ncols], cond[:, :ncols], f"head_weight_grad off={raw_off} n_out={n_out} kp={kp} n={n}")
    assert (dst[:, ncols:] == SENT).all()


# ---- per-ray column sums ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S,N", [(1, 1, 64), (37, 33, 128), (9, 128, 512)])
def test_bias_grad_rays(R, S, N):
    gen = _gen(R + S + N)
    Mp = br.round_up(R * S, 256)
    g = _randn(gen, R * S, N)
    gp = br.pack_panels(g, Mp, row_fill=BIG)

    def run():
        out = Guarded(R * N, guard=N)
        lib.check(L().mofa_bias_grad_rays(lib.ptr(gp), Mp, R, S, N, out.ptr(), lib.stream()), "bias_grad_rays")
        torch.cuda.synchronize()
        return (out.check().reshape(R, N),)

    (out,) = _twice(run)
    ref, cond = br.bias_grad_rays(g, R, S)
    br.assert_close(out, ref, cond, f"bias_grad_rays R={R} S={S} N={N}")


# ---- positional encoding: backward (rays, explicit points) and the feature panels ---------------------------------------------------------
@pytest.mark.parametrize("R,S,zs", [(1, 1, 1), (5, 37, 41), (9, 130, 130), (130, 64, 64)])
@pytest.mark.parametrize("nf", [0, 4, 10, 16])
def test_pe_backward_and_panels(nf, R, S, zs):
    """gx = g_id + sum_f 2^f (g_sin cos(2^f x) - g_cos sin(2^f x)) at the fp32 points x = o + d z; d_rays_o = sum_s gx, d_rays_d = sum_s gx z.
    Bound: 1e-6 * sum |terms| + C_PE * 2^-24 * sum_f 2^f (|g_sin| + |g_cos|), the second term for the device sincosf at arguments up to
    2^9 |x| (2^15 |x| at 16 frequencies).  Measured on MI355X: worst |err| / (2^-24 * sum_f 2^f (|g_sin| + |g_cos|)) = 1.953 (d_pts at n_freqs = 4, 9 x 130; <= 0.38 for
    the summed ray outputs); C_PE = 7.8 = 4 x that ratio (bwd_reference.C_PE).  Worst err / sum |terms|: 1.5e-7.  (5, 37) runs with z_row_stride > S;
    S = 130: a lane takes several samples; 130 rays: more than one block's waves."""
    gen = _gen(nf + R + S)
    st = lib.stream()
    n, kp = R * S, L().mofa_pe_k_padded(nf)
    assert kp == (64 if nf <= 10 else 128)                                             # 16 frequencies: 99 features in 8 panels
    Mp = br.round_up(n, 256)
    o = torch.rand(R, 3, generator=gen, device=DEV) * 6 - 3
    d = _randn(gen, R, 3, scale=0.6)
    zfull = torch.full((R, zs), BIG, device=DEV)
    zfull[:, :S] = torch.sort(torch.rand(R, S, generator=gen, device=DEV) * 18 + 8, -1)[0]
    z = zfull[:, :S].contiguous()
    feats = 3 + 6 * nf
    dpe = _randn(gen, n, feats)
    dpe_p = br.pack_panels(dpe, Mp, k_padded=kp, row_fill=BIG, col_fill=-BIG)          # padding rows AND padding features must not be read
    pts = br.points_from_rays(o, d, z).contiguous()

    def run():
        do, dd, dp = Guarded(R * 3), Guarded(R * 3), Guarded(n * 3)
        lib.check(L().mofa_pe_backward(lib.ptr(dpe_p), Mp, lib.ptr(o), lib.ptr(d), lib.ptr(zfull), zs, R, S, nf, do.ptr(), dd.ptr(), st), "pe_backward")
        lib.check(L().mofa_pe_backward_points(lib.ptr(dpe_p), Mp, lib.ptr(pts), n, nf, dp.ptr(), st), "pe_backward_points")
        torch.cuda.synchronize()
        return do.check().reshape(R, 3), dd.check().reshape(R, 3), dp.check().reshape(n, 3)

    do, dd, dp = _twice(run)
    (go, co, to), (gd, cd, td) = br.pe_ray_backward(dpe, o, d, z, nf)
    gx, cx, tx = br.pe_point_backward(dpe, pts, nf)
    for got, ref, cond, trig, name in ((dp, gx, cx, tx, "d_pts"), (do, go, co, to, "d_rays_o"), (dd, gd, cd, td, "d_rays_d")):
        if nf:
            err = (got.double() - ref).abs()
            print(f"pe_backward nf={nf} R={R} S={S} {name}: worst err / (2^-24 sum_f 2^f (|g_sin| + |g_cos|)) = {float((err / (br.U32 * trig)).max()):.3e}, "
                  f"after the contraction term {float(((err - br.bound(cond)).clamp_min(0) / (br.U32 * trig)).max()):.3e}")
        br.assert_close(got, ref, cond, f"pe_backward nf={nf} R={R} S={S} {name}", trig=trig)
    if nf == 0:
        assert torch.equal(dp, dpe[:, :3])                                             # identity features only: exact
    # the explicit-points form ran on the same fp32 points: its sums over the samples match the ray form to summation rounding
    dps, zz = dp.double().reshape(R, S, 3), z.double()[:, :, None]
    br.assert_close(do, dps.sum(1), dps.abs().sum(1), f"pe_backward nf={nf} R={R} S={S} sum_s d_pts vs d_rays_o")
    br.assert_close(dd, (dps * zz).sum(1), (dps * zz).abs().sum(1), f"pe_backward nf={nf} R={R} S={S} sum_s d_pts z vs d_rays_d")

    # the feature panels, from the rays and from the explicit points
    def run_panels():
        a, b = Guarded(Mp * kp), Guarded(Mp * kp)
        lib.check(L().mofa_pe_panels(lib.ptr(o), lib.ptr(d), lib.ptr(zfull), zs, None, n, S, nf, Mp, a.ptr(), st), "pe_panels")
        lib.check(L().mofa_pe_panels(None, None, None, 0, lib.ptr(pts), n, S, nf, Mp, b.ptr(), st), "pe_panels/pts")
        torch.cuda.synchronize()
        return a.check(), b.check()

    a, b = _twice(run_panels)
    assert _same_bits(a, b)
    pan, ref = br.unpack_panels(a, Mp, kp), br.pe_panels(pts, nf, Mp, kp)
    assert torch.equal(pan[:n, :3], pts)
    # k_pe_panels writes 0 to the padding features (columns 3 + 6 n_freqs .. k_padded) and to the padding rows: the first layer's packed
    # weights are zero-padded there too (mofa_pack_panels), so neither side of the product relies on the other
    assert (pan[:, feats:] == 0).all() and (pan[n:] == 0).all()
    err = float((pan.double() - ref).abs().max())
    print(f"pe_panels nf={nf} R={R} S={S}: max abs err {err:.3e}")
    assert err <= 3e-7                                                                 # sinf / cosf of the exact fp32 argument: <= 2 ulp of a value in [-1, 1]


# ---- the padding-row promise mofa_weight_grad relies on ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipe", ["0", "1"])
def test_forward_forms_leave_finite_padding_rows_for_the_weight_gradient(pipe, knob):
    """mofa_weight_grad multiplies the padding rows of X in the batch's last chunk by zeroed rows of G, so a non-finite value there would
    reach dW as 0 * NaN ("padding rows ... must be finite").  Both forward forms (MOFA_PIPE=0 / 1) keep that promise: layer 0 from rays, layer 0 through mofa_pe_panels and
    a following layer, each into NaN-filled buffers, leave no non-finite value in any row; the weight gradient taken from those buffers
    is the fp64 one."""
    knob("MOFA_PIPE", pipe)
    gen = _gen(77)
    st = lib.stream()
    R, S, N, nf = 7, 100, 128, 10
    n, Mp = R * S, 768
    o = torch.rand(R, 3, generator=gen, device=DEV) * 6 - 3
    d = _randn(gen, R, 3, scale=0.6)
    z = torch.sort(torch.rand(R, S, generator=gen, device=DEV) * 18 + 8, -1)[0].contiguous()
    w0, b0 = _randn(gen, N, 63, scale=1 / 8), _randn(gen, N)
    w1, b1 = _randn(gen, N, N, scale=N ** -0.5), _randn(gen, N)
    w0p, w1p = br.pack_panels(w0, N, k_padded=64), br.pack_panels(w1, N)
    y0, pan, y0b, y1 = Guarded(Mp * N), Guarded(Mp * 64), Guarded(Mp * N), Guarded(Mp * N)
    lib.check(L().mofa_layer0_forward(lib.ptr(o), lib.ptr(d), lib.ptr(z), S, None, n, S, nf, lib.ptr(w0p), lib.ptr(b0), y0.ptr(), Mp, N, None, st), "layer0")
    lib.check(L().mofa_pe_panels(lib.ptr(o), lib.ptr(d), lib.ptr(z), S, None, n, S, nf, Mp, pan.ptr(), st), "pe_panels")
    lib.check(L().mofa_layer_forward(pan.ptr(), 64, None, 0, lib.ptr(w0p), lib.ptr(b0), 0, 1, y0b.ptr(), Mp, N, 1, st), "layer0 via panels")
    lib.check(L().mofa_layer_forward(y0.ptr(), N, None, 0, lib.ptr(w1p), lib.ptr(b1), 0, 1, y1.ptr(), Mp, N, 1, st), "layer1")
    torch.cuda.synchronize()
    for buf in (y0, pan, y0b, y1):
        assert torch.isfinite(buf.check()).all()
    g = _randn(gen, n, N)
    gp = br.pack_panels(g, Mp, row_fill=BIG)
    ws = Guarded(L().mofa_weight_grad_workspace_floats(n, N, N))
    dw = Guarded(N * N, fill=SENT)
    lib.check(L().mofa_weight_grad(lib.ptr(gp), N, y1.ptr(), N, Mp, n, N, N, dw.ptr(), N, 0, None, ws.ptr(), st), "weight_grad")
    torch.cuda.synchronize()
    ref, cond, _, _ = br.weight_grad(g, br.unpack_panels(y1.out, Mp, N), n)
    br.assert_close(dw.check().reshape(N, N), ref, cond, f"weight_grad from forward buffers MOFA_PIPE={pipe}")

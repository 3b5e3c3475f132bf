"""The comparator of tests/test_gpu_bwd_kernels.py must be able to fail.  For every backward operation: the fp64 restatement
(tests/bwd_reference.py) at one of the GPU test's shapes, an honest fp32 evaluation that passes the GPU test's bound, and the faults
such kernels usually have — a dropped point, a dropped split, exchanged operands, a column offset off by one, one mask bit, one
swizzled chunk, accumulate ignored, accumulate and mask in the other order — each of which must EXCEED that bound.  Runs on the CPU."""
import torch

import bwd_reference as br


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _over(got, ref, cond, trig=None):
    """worst |got - ref| / bound"""
    return float(((got.double() - ref).abs() / br.bound(cond, trig)).max())


def test_layout_helpers_round_trip():
    gen = torch.Generator().manual_seed(1)
    for rows, k, rp in ((300, 63, 512), (256, 128, 256), (93, 250, 128)):
        x = _rand(gen, rows, k)
        kp = br.round_up(k, 16)
        p = br.pack_panels(x, rp, row_fill=7.0, col_fill=-3.0)
        assert p.shape == (rp * kp,)
        full = br.unpack_panels(p, rp, kp)
        assert torch.equal(full[:rows, :k], x) and (full[rows:] == 7.0).all() and (full[:rows, k:] == -3.0).all()
        r, c = torch.meshgrid(torch.arange(rows), torch.arange(k), indexing="ij")          # the documented address formula, every element
        assert torch.equal(p[br.panel_offset(rp, r, c)], x)
        assert br.panel_offset(rp, 5, 7) == 5 * 16 + ((1 ^ 1) * 4) + 3
        q = br.swap_chunk_with_neighbour(p, rp, 17, 33 % k)
        assert int((q != p).sum()) in range(1, 9) and torch.equal(br.swap_chunk_with_neighbour(q, rp, 17, 33 % k), p)
    flags = torch.rand(256 * 12, generator=gen) > 0.5
    words = br.mask_bits(flags)
    assert words.dtype == torch.int64 and words.shape == (12 * 4,)
    assert torch.equal(br.mask_flags(words), flags)
    for o in (0, 1, 3, 4, 255, 256, 1023, 256 * 12 - 1):                                   # float offset o <-> bit ((o & 255) >> 2) of word (o >> 8) * 4 + (o & 3)
        one = torch.zeros(256 * 12, dtype=torch.bool)
        one[o] = True
        w, b = br.mask_bit_position(o)
        assert (w, b) == ((o >> 8) * 4 + (o & 3), (o & 255) >> 2)
        want = torch.zeros(48, dtype=torch.int64)
        want[w] = (1 << b) if b < 63 else -(1 << 63)
        assert torch.equal(br.mask_bits(one), want), o


def test_split_plan_matches_the_issue_cases():
    """tile variant and split count of every weight-gradient shape of the GPU test (mofa_weight_grad_workspace_floats confirms them there)"""
    want = {(256, 512): (128, 256), (128, 384): (128, 128), (128, 192): (128, 64), (192, 128): (64, 128), (192, 192): (64, 64)}
    for (n, k), tiles in want.items():
        for pts, total in ((112, 1), (256 * 9 - 5, 9), (256 * 17, 17)):
            p = br.wg_plan(pts, n, k)
            assert (p["tn"], p["tk"]) == tiles and p["total"] == total and p["spt"] == 1, (n, k, pts, p)
    p = br.wg_plan(256 * 17 - 5, 1024, 2048)                 # the one case where a split holds two row tiles: splits of 2 and 1 tiles per range
    assert (p["tn"], p["tk"], p["spt"], p["total"]) == (128, 256, 2, 11)
    assert p["splits"] == [(0, 2), (2, 1), (3, 2), (5, 1), (6, 2), (8, 1), (9, 2), (11, 1), (12, 2), (14, 1), (15, 2)]


def test_weight_gradient_comparator_sees_every_fault():
    gen = torch.Generator().manual_seed(2)
    N, K, n = 256, 512, 256 * 17
    Mp = br.round_up(n, 256)
    g, x = _rand(gen, Mp, N), _rand(gen, Mp, K)
    dw, cond, db, cond_b = br.weight_grad(g, x, n)
    honest = g[:n].T @ x[:n]                                  # an fp32 evaluation passes
    assert not br.exceeds(honest, dw, br.bound(cond)) and not br.exceeds(g[:n].sum(0), db, br.bound(cond_b))
    # the last point dropped: more than two orders over the bound, dW and db
    dw1, _, db1, _ = br.weight_grad(g, x, n - 1)
    assert _over(dw1, dw, cond) > 100 and _over(db1, db, cond_b) > 100
    # one point too many (a padding row read)
    g2, x2 = torch.cat([g, _rand(gen, 1, N)]), torch.cat([x, _rand(gen, 1, K)])
    assert _over(br.weight_grad(g2, x2, n + 1)[0], dw, cond) > 100
    # one split's row tiles left out of the second stage
    plan = br.wg_plan(n, N, K)
    assert plan["total"] == 17
    for s in (0, 7, plan["total"] - 1):
        first, count = plan["splits"][s]
        gz = g.clone()
        gz[first * 256:(first + count) * 256] = 0
        dws, _, dbs, _ = br.weight_grad(gz, x, n)
        assert _over(dws, dw, cond) > 100 and _over(dbs, db, cond_b) > 100, s
    # one 4-float chunk of X (of G) exchanged with its swizzle neighbour, in one row
    xs = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(x, Mp), Mp, 1000, 37), Mp, K)
    assert br.exceeds(br.weight_grad(g, xs, n)[0], dw, br.bound(cond))
    gs = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(g, Mp), Mp, n - 1, 200), Mp, N)
    assert br.exceeds(br.weight_grad(gs, x, n)[0], dw, br.bound(cond))
    # col0 shifted by one: the sub-block case (n_out 250, ncols 500, ld 600, col0 37)
    def place(col0):
        dst = torch.full((256, 600), -7.25e11, dtype=torch.float64)
        dst[:250, col0:col0 + 500] = dw[:250, :500]
        return dst
    lim = torch.full((256, 600), br.TINY, dtype=torch.float64)
    lim[:250, 37:537] = br.bound(cond[:250, :500])
    assert not br.exceeds(place(37), place(37), lim) and br.exceeds(place(38), place(37), lim)
    # G and X exchanged / the result transposed (a square shape of the GPU test: 192 x 192 at 112 points)
    g, x = _rand(gen, 256, 192), _rand(gen, 256, 192)
    dw, cond, _, _ = br.weight_grad(g, x, 112)
    assert _over(br.weight_grad(x, g, 112)[0], dw, cond) > 100 and _over(dw.T, dw, cond) > 100


def test_backward_data_comparator_sees_every_fault():
    gen = torch.Generator().manual_seed(3)
    M, gk, ko = 256, 64, 64
    g, w, old = _rand(gen, M, gk), _rand(gen, gk, ko, scale=1 / 8), _rand(gen, M, ko)
    mask = _rand(gen, M, ko)
    mask[torch.rand(M, ko, generator=gen) < 0.1] = 0.0        # negative, positive and exact zeros
    ref, cond = br.backward_data(g, w, old, mask, True)
    lim = br.bound(cond)
    honest = torch.where(mask > 0, old + g @ w, torch.zeros(()))
    assert not br.exceeds(honest, ref, lim)
    assert br.exceeds(br.backward_data(g, w.T, old, mask, True)[0], ref, lim)               # the weight transposed
    assert br.exceeds(br.backward_data(g, w, old, mask, False)[0], ref, lim)                # accumulate ignored
    assert br.exceeds(br.backward_data(g, w, None, None, False)[0], ref, lim)               # ... and the mask
    other = old.double() + br.backward_data(g, w, None, mask, False)[0]                     # mask first, then accumulate
    assert br.exceeds(other, ref, lim)
    ge0 = torch.where(mask >= 0, (old.double() + g.double() @ w.double()), torch.zeros((), dtype=torch.float64))
    assert br.exceeds(ge0, ref, lim)                                                        # >= 0 instead of > 0
    # one mask bit flipped, through the tape's bit layout (the element with the largest unmasked value)
    full = br.backward_data(g, w, old, None, True)[0]
    r, k = divmod(int(full.abs().argmax()), ko)
    o = int(br.panel_offset(M, r, k))
    words = br.mask_bits(br.pack_panels(mask, M) > 0)
    wi, bit = br.mask_bit_position(o)
    words[wi] ^= (1 << bit) if bit < 63 else -(1 << 63)
    flipped = br.unpack_panels(br.mask_flags(words).float(), M, ko)
    assert int((flipped != (mask > 0).float()).sum()) == 1 and flipped[r, k] != float(mask[r, k] > 0)
    assert br.exceeds(br.backward_data(g, w, old, flipped, True)[0], ref, lim)
    # one 4-float chunk of the result exchanged with its swizzle neighbour
    sw = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(full, M), M, r, k), M, ko)
    assert br.exceeds(sw, full, br.bound(cond))
    # the transposed pack with col0 off by one (W 61 x 50 inside a wider matrix: n_out < g_k, ncols < k_out_padded, zero padding)
    big = _rand(gen, 61, 80, scale=1 / 8)
    def wt(col0):
        z = torch.zeros(gk, ko)
        z[:61, :50] = big[:, col0:col0 + 50]
        return z
    ref2, cond2 = br.backward_data(g, wt(13))
    assert br.exceeds(br.backward_data(g, wt(14))[0], ref2, br.bound(cond2))
    junk = wt(13)
    junk[61:, :] = 1.0                                                                       # padded operand entries not zero
    assert br.exceeds(br.backward_data(g, junk)[0], ref2, br.bound(cond2))


def test_head_comparators_see_every_fault():
    gen = torch.Generator().manual_seed(4)
    n, Mp, K = 700, 768, 64
    d_raw, x = _rand(gen, Mp, 4), _rand(gen, Mp, K)
    w, old, mask = _rand(gen, 4, K, scale=1 / 8), _rand(gen, Mp, K), _rand(gen, Mp, K)
    for off, n_out in ((0, 3), (3, 1)):
        ref, cond = br.head_backward(d_raw, off, n_out, w[:n_out], n, Mp, old, mask, True)
        lim = br.bound(cond)
        assert (ref[n:] == torch.where(mask[n:] > 0, old[n:].double(), torch.zeros((), dtype=torch.float64))).all()   # rows >= n_points: old, masked
        assert br.exceeds(br.head_backward(d_raw, off, n_out, w[:n_out], n + 1, Mp, old, mask, True)[0], ref, lim)    # a padding row read
        assert br.exceeds(br.head_backward(d_raw, off, n_out, w[:n_out], n - 1, Mp, old, mask, True)[0], ref, lim)
        assert br.exceeds(br.head_backward(d_raw, off, n_out, w[:n_out], n, Mp, old, mask, False)[0], ref, lim)
        assert br.exceeds(old.double() + br.head_backward(d_raw, off, n_out, w[:n_out], n, Mp, None, mask, False)[0], ref, lim)
        shifted = (off + 1) % (5 - n_out)
        assert br.exceeds(br.head_backward(d_raw, shifted, n_out, w[:n_out], n, Mp, old, mask, True)[0], ref, lim)    # raw_off off by one
        dw, cw = br.head_weight_grad(d_raw, off, n_out, x, n)
        assert not br.exceeds(d_raw[:n, off:off + n_out].T @ x[:n], dw, br.bound(cw))
        assert _over(br.head_weight_grad(d_raw, off, n_out, x, n - 1)[0], dw, cw) > 100                                 # the last point dropped
        assert _over(br.head_weight_grad(d_raw, shifted, n_out, x, n)[0], dw, cw) > 100
        xs = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(x, Mp), Mp, 333, 21), Mp, K)
        assert br.exceeds(br.head_weight_grad(d_raw, off, n_out, xs, n)[0], dw, br.bound(cw))


def test_ray_sum_comparator_sees_every_fault():
    gen = torch.Generator().manual_seed(5)
    R, S, N = 37, 33, 128
    g = _rand(gen, br.round_up(R * S, 256), N)
    ref, cond = br.bias_grad_rays(g, R, S)
    assert not br.exceeds(g[:R * S].reshape(R, S, N).sum(1), ref, br.bound(cond))
    dropped = g[:R * S].reshape(R, S, N)[:, :-1].double().sum(1)                             # the last sample of every ray
    assert _over(dropped, ref, cond) > 100
    assert br.exceeds(br.bias_grad_rays(g, R, S + 1)[0], ref, br.bound(cond))               # rays cut at the wrong stride
    gs = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(g, g.shape[0]), g.shape[0], 40, 77), g.shape[0], N)
    assert br.exceeds(br.bias_grad_rays(gs, R, S)[0], ref, br.bound(cond))


def test_positional_encoding_backward_comparator_sees_every_fault():
    gen = torch.Generator().manual_seed(6)
    R, S, nf = 5, 37, 10
    o = (torch.rand(R, 3, generator=gen) * 6 - 3)
    d = _rand(gen, R, 3, scale=0.6)
    z = torch.sort(torch.rand(R, S, generator=gen) * 18 + 8, -1)[0]
    dpe = _rand(gen, 256, 64)
    (go, co, to), (gd, cd, td) = br.pe_ray_backward(dpe, o, d, z, nf)
    pts = br.points_from_rays(o, d, z)
    gx, cx, tx = br.pe_point_backward(dpe, pts, nf)
    assert torch.equal(gx.reshape(R, S, 3).sum(1), go)
    # an honest fp32 evaluation (fp32 sin / cos of the exact fp32 argument) passes
    g32 = dpe[:R * S, :3].clone()
    for f in range(nf):
        a = pts * float(2 ** f)
        g32 += float(2 ** f) * (dpe[:R * S, 3 + 6 * f:6 + 6 * f] * torch.cos(a) - dpe[:R * S, 6 + 6 * f:9 + 6 * f] * torch.sin(a))
    assert not br.exceeds(g32, gx, br.bound(cx, tx))
    # the point not rounded to fp32 (o + d z in one fused or wider operation): 2^9 amplifies half an ulp of x far over the bound
    wide = (o.double()[:, None] + d.double()[:, None] * z.double()[:, :, None]).reshape(-1, 3)
    assert br.exceeds(br.pe_point_backward(dpe, wide, nf)[0], gx, br.bound(cx, tx))
    # sin and cos gradients exchanged; one frequency too few; the last sample of a ray dropped; z of the neighbouring sample
    swapped = dpe.clone()
    for f in range(nf):
        swapped[:, 3 + 6 * f:6 + 6 * f], swapped[:, 6 + 6 * f:9 + 6 * f] = dpe[:, 6 + 6 * f:9 + 6 * f], dpe[:, 3 + 6 * f:6 + 6 * f]
    assert br.exceeds(br.pe_point_backward(swapped, pts, nf)[0], gx, br.bound(cx, tx))
    assert br.exceeds(br.pe_point_backward(dpe, pts, nf - 1)[0], gx, br.bound(cx, tx))
    assert br.exceeds(gx.reshape(R, S, 3)[:, :-1].sum(1), go, br.bound(co, to))
    assert br.exceeds((gx.reshape(R, S, 3) * z.double().roll(1, 1)[:, :, None]).sum(1), gd, br.bound(cd, td))
    sw = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(dpe, 256), 256, 100, 1), 256, 64)
    assert br.exceeds(br.pe_ray_backward(sw, o, d, z, nf)[0][0], go, br.bound(co, to))
    # the feature panels: zero in the padding rows and in the padding features (what the zero-padded packed weights of layer 0 assume)
    pan = br.pe_panels(pts, nf, 256, 64)
    assert (pan[R * S:] == 0).all() and (pan[:, 63:] == 0).all() and torch.equal(pan[:R * S, :3], pts.double())
    assert torch.equal(pan[:R * S, 3:6], torch.sin(pts.double())) and torch.equal(pan[:R * S, 60:63], torch.cos(pts.double() * 512))

"""The forward kernels one by one, through the C ABI, against the fp64 restatements of tests/fwd_reference.py — and the whole network layer
by layer, from its own tape.

Every output element is held to a rounding-level bound: |got - ref64| <= 1e-6 * (sum |a b| + |bias|) + tiny (bwd_reference.C_CONTRACTION),
plus C_PE * 2^-24 * sum |w| over the sine / cosine features where the device's sinf / cosf enter (bwd_reference.C_PE).  Inputs are
asymmetric random from a seeded device generator; every output sits between two guard regions that must come back bit-identical and is
pre-filled with NaN or a sentinel; padding rows of input panels hold +-BIG (rows are independent: the valid rows must not notice); a
bias buffer is followed by NaN; every call runs twice and must repeat bit for bit.  tests/test_fwd_reference_cpu.py shows on the CPU
that a dropped column or panel, exchanged weight blocks, a shifted offset, a wrong bias row, a missing clamp, a wrong activation, a wrong
feature order or frequency, one swizzled chunk and a tape slot off by one layer each break these bounds.  Each test prints its worst
err / sum |a b|."""
import pytest
import torch

import bwd_reference as br
import fwd_reference as fr
from mofanerf_amd import lib
from test_gpu_bwd_kernels import BIG, SENT, Guarded, _same_bits, _twice

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def L():
    return lib.load()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, device=DEV) * scale


def _then_nan(values, extra=512):
    """`values` followed by NaN in one buffer: an over-read reaches the output as NaN"""
    buf = torch.full((values.numel() + extra,), NAN, device=DEV)
    buf[:values.numel()] = values.reshape(-1)
    return buf


def _padded(values, n_padded):
    out = torch.zeros(*values.shape[:-1], n_padded, device=DEV)
    out[..., :values.shape[-1]] = values
    return out


def _rays(gen, R, S):
    """o in +-3, |d| about 0.6, z in [8, 26]: coordinates up to about 20, encoding arguments up to 2^15 times that"""
    o = torch.rand(R, 3, generator=gen, device=DEV) * 6 - 3
    d = _randn(gen, R, 3, scale=0.6)
    z = torch.sort(torch.rand(R, S, generator=gen, device=DEV) * 18 + 8, -1)[0].contiguous()
    return o, d, z


# ---- a. mofa_layer_forward / _masked ------------------------------------------------------------------------------------------------------
def _layer_case(k1, k2, Np, Mp, relu, div=0):
    """One layer checked in full: y (every valid row; with a per-ray bias EVERY row, see below), its padding features, the mask words."""
    M = Mp - 68
    k1l, k2l, n_out = fr.logical(k1, k2, Np)
    gen = _gen(k1 + k2 + Np + Mp + relu + div)
    st = lib.stream()
    x1, x2 = _randn(gen, M, k1l), (_randn(gen, M, k2l) if k2 else None)
    w, b = _randn(gen, n_out, k1l + k2l, scale=(k1l + k2l) ** -0.5), _randn(gen, n_out)
    x1p = br.pack_panels(x1, Mp, k_padded=k1, row_fill=BIG, col_fill=0.5)          # (the packed weight is zero in the padding columns)
    x2p = br.pack_panels(x2, Mp, k_padded=k2, row_fill=-BIG, col_fill=0.5) if k2 else None
    wp = br.pack_panels(w[:, :k1l].contiguous(), Np, k_padded=k1)
    if k2:
        wp = torch.cat([wp, br.pack_panels(w[:, k1l:].contiguous(), Np, k_padded=k2)])
    if div:
        rows = -(-M // div)                                                        # exactly the rows the valid points need, NaN behind them
        bias_rows = _randn(gen, rows, n_out)
        bp = _then_nan(_padded(bias_rows, Np), extra=4 * Np)
    else:
        rows, bias_rows = 1, None
        bp = _then_nan(_padded(b, Np))

    def run(masked=False):
        y, bits = Guarded(Mp * Np), Guarded(Mp * Np // 64, dtype=torch.int64, fill=0x33)
        if masked:
            lib.check(L().mofa_layer_forward_masked(lib.ptr(x1p), k1, lib.ptr(x2p), k2, lib.ptr(wp), lib.ptr(bp), div, rows, y.ptr(), Mp, Np, relu,
                                                    bits.ptr(), st), "layer_forward_masked")
        else:
            lib.check(L().mofa_layer_forward(lib.ptr(x1p), k1, lib.ptr(x2p), k2, lib.ptr(wp), lib.ptr(bp), div, rows, y.ptr(), Mp, Np, relu, st),
                      "layer_forward")
        torch.cuda.synchronize()
        return y.check(), bits.check()

    y, _ = _twice(run)
    yl = br.unpack_panels(y, Mp, Np)
    what = f"layer_forward {k1}+{k2}->{Np} Mp={Mp} relu={relu} div={div}"
    if div:
        # The clamp brow >= bias_rows acts only in the padding rows, so ALL rows are compared: +-BIG in X hides any finite bias there, but
        # not the NaN behind the last bias row (at relu = 0: max(v, 0) turns NaN into 0).
        xa = br.unpack_panels(x1p, Mp, k1)[:, :k1l]
        ref, cond = fr.layer(xa, w, None, relu=bool(relu), bias_rows=bias_rows, div=div)
        ratio = br.assert_close(yl[:, :n_out], ref, cond, what)
        assert (yl[:M, n_out:] == 0).all()
    else:
        ref, cond = fr.layer(x1, w, b, x2, relu=bool(relu))
        ratio = br.assert_close(yl[:M, :n_out], ref, cond, what)
        assert (yl[:M, n_out:] == 0).all(), "a padding feature of a valid row is not 0"
    if relu:
        ym, bits = _twice(lambda: run(True))
        assert _same_bits(ym, y), "y differs when the mask is written"
        assert torch.equal(bits, br.mask_bits(y > 0)), "mask words differ from (y > 0)"
    return ratio


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("Mp", [256, 768])
@pytest.mark.parametrize("k1,k2,Np", fr.LAYER_CASES)
def test_layer_forward_every_tile_and_loop_form(k1, k2, Np, Mp, relu):
    """128- and 64-feature tiles x the pipelined loop (an even number >= 4 of panels) / the plain loop (48: odd, 32: fewer than 4) x one
    and two K sources x with and without the ReLU, at one and three row tiles; at relu = 1 also the mask-writing form."""
    _layer_case(k1, k2, Np, Mp, relu)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("div", fr.BIAS_DIVS)
@pytest.mark.parametrize("Np", [64, 128])
def test_layer_forward_per_ray_bias_rows(Np, div, relu):
    """The per-ray-bias instantiation (the view layer) at both tiles: 700 points in 768 rows, rays of 1, 33 (straddling the row tiles),
    64 and 300 samples, exactly ceil(700 / div) bias rows."""
    _layer_case(64, 0, Np, 768, relu, div=div)


# ---- b. mofa_layer0_forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", fr.LAYER0_RAYS)
@pytest.mark.parametrize("Np", [64, 128])
@pytest.mark.parametrize("nf", fr.LAYER0_FREQS)
def test_layer0_forward_against_fp64(nf, Np, R, S):
    """relu(PE(x) @ W.T + b) with the encoding generated in the prologue: 4 (up to 10 frequencies) and 8 (11, 16) operand panels, both
    tiles, 1 / 185 / 1170 points (all ragged).  Rays with their own z rows, rays sharing one z row, and explicit points agree bit for
    bit on the points br.points_from_rays forms.  The packed weight's padding columns hold BIG: a padding feature that is not exactly 0
    shows."""
    gen = _gen(nf + Np + R + S)
    st = lib.stream()
    n, Mp = R * S, br.round_up(R * S, 256)
    feats, kp, n_out = 3 + 6 * nf, L().mofa_pe_k_padded(nf), Np - 3
    assert kp == (64 if nf <= 10 else 128)
    o, d, z = _rays(gen, R, S)
    zs = S + 4                                                                     # z rows with a stride, BIG between them
    zfull = torch.full((R, zs), BIG, device=DEV)
    zfull[:, :S] = z
    z0 = z[R // 2:R // 2 + 1].contiguous()                                         # one row shared by every ray
    z0_rows = z0.expand(R, S).contiguous()
    pts_a, pts_b = br.points_from_rays(o, d, z).contiguous(), br.points_from_rays(o, d, z0_rows).contiguous()
    w, b = _randn(gen, n_out, feats + 5, scale=1 / 8), _randn(gen, n_out)
    wp = br.pack_panels(w[:, :feats].contiguous(), Np, k_padded=kp, col_fill=BIG)       # (rows >= n_out: zero in every column)
    bp = _then_nan(_padded(b, Np))

    def run(src, masked=False):
        y, bits = Guarded(Mp * Np), Guarded(Mp * Np // 64, dtype=torch.int64, fill=0x33)
        mb = bits.ptr() if masked else None
        if src == "rays":
            args = (lib.ptr(o), lib.ptr(d), lib.ptr(zfull), zs, None)
        elif src == "rays, full rows of the shared z":
            args = (lib.ptr(o), lib.ptr(d), lib.ptr(z0_rows), S, None)
        elif src == "shared z":
            args = (lib.ptr(o), lib.ptr(d), lib.ptr(z0), 0, None)
        else:
            args = (None, None, None, 0, lib.ptr(pts_a if src == "points a" else pts_b))
        lib.check(L().mofa_layer0_forward(*args, n, S, nf, lib.ptr(wp), lib.ptr(bp), y.ptr(), Mp, Np, mb, st), f"layer0_forward/{src}")
        torch.cuda.synchronize()
        return y.check(), bits.check()

    for group, pts in ((("rays", "points a"), pts_a), (("shared z", "rays, full rows of the shared z", "points b"), pts_b)):
        ys = [_twice(lambda: run(src))[0] for src in group]
        for src, y in zip(group[1:], ys[1:]):
            assert _same_bits(y, ys[0]), f"{src} differs from {group[0]}"
        yl = br.unpack_panels(ys[0], Mp, Np)
        ref, cond, trig = fr.layer0(pts, nf, w, b)
        br.assert_close(yl[:n, :n_out], ref, cond, f"layer0_forward nf={nf} Np={Np} {R}x{S} ({group[0]})", trig=trig)
        assert (yl[:n, n_out:] == 0).all()
        assert torch.isfinite(yl).all()                                            # padding rows: finite
    ym, bits = _twice(lambda: run("rays", True))
    y = run("rays")[0]
    assert _same_bits(ym, y) and torch.equal(bits, br.mask_bits(y > 0))


# ---- c. mofa_head_forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 700])
@pytest.mark.parametrize("kp", [64, 528])
@pytest.mark.parametrize("raw_off,n_out", [(0, 3), (3, 1), (0, 4), (1, 2)])
def test_head_forward_against_fp64(raw_off, n_out, kp, n):
    gen = _gen(raw_off + n_out + kp + n)
    Mp, kl = br.round_up(n, 256), kp - 5
    x = _randn(gen, n, kl)
    xp = br.pack_panels(x, Mp, k_padded=kp, row_fill=BIG, col_fill=0.5)
    w, b = _randn(gen, n_out, kl, scale=1 / 8), _randn(gen, n_out)
    wd, bd = _then_nan(_padded(w, kp)), _then_nan(b)                               # dense rows [n_out, k_padded], zero in the padding columns

    def run():
        raw = Guarded(Mp * 4, fill=SENT)
        lib.check(L().mofa_head_forward(lib.ptr(xp), kp, Mp, lib.ptr(wd), lib.ptr(bd), n_out, raw.ptr(), raw_off, n, lib.stream()), "head_forward")
        torch.cuda.synchronize()
        return (raw.check().reshape(Mp, 4),)

    (raw,) = _twice(run)
    ref, cond = fr.head(x, w, b)
    br.assert_close(raw[:n, raw_off:raw_off + n_out], ref, cond, f"head_forward off={raw_off} n_out={n_out} kp={kp} n={n}")
    rest = raw.clone()
    rest[:n, raw_off:raw_off + n_out] = SENT
    assert (rest == SENT).all(), "raw written outside rows < n_points, columns [raw_off, raw_off + n_out)"


# ---- d. mofa_view_bias --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 8, 50])
@pytest.mark.parametrize("nf", [0, 4, 16])
def test_view_bias_against_fp64(nf, R):
    gen = _gen(nf + R)
    feats, n_out, Np = 3 + 6 * nf, 96, 128
    ld = feats + 13                                                                # the view layer's weight: [encoding | W per-point columns]
    vd = _then_nan(torch.nn.functional.normalize(_randn(gen, R, 3), dim=-1))
    w, b = _randn(gen, n_out, ld, scale=1 / 5), _randn(gen, n_out)
    wb, bb = _then_nan(w), _then_nan(b)

    def run():
        out = Guarded(R * Np, guard=Np)
        lib.check(L().mofa_view_bias(lib.ptr(vd), R, nf, lib.ptr(wb), n_out, ld, lib.ptr(bb), out.ptr(), Np, lib.stream()), "view_bias")
        torch.cuda.synchronize()
        return (out.check().reshape(R, Np),)

    (out,) = _twice(run)
    ref, cond, trig = fr.view_bias(vd[:R * 3].reshape(R, 3), nf, w, b)
    br.assert_close(out[:, :n_out], ref, cond, f"view_bias nf={nf} R={R}", trig=trig)
    assert (out[:, n_out:] == 0).all()


# ---- e. mofa_positional_encode ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("nf", [0, 1, 10, 16])
def test_positional_encode_against_fp64(nf, n):
    """Identity features: the input's bits.  Sine / cosine features: within C_PE * 2^-24 of fp64 sin / cos of the exact argument 2^f x,
    for x up to +-50 (arguments up to 1.6e6 at 16 frequencies), +-0 and a denormal; NaN for a NaN or infinite coordinate."""
    gen = _gen(nf + n)
    feats = 3 + 6 * nf
    x = torch.rand(n, 3, generator=gen, device=DEV) * 100 - 50
    special = torch.tensor([[50.0, -0.0, 1e-40], [-50.0, 0.0, -1e-40], [NAN, float("inf"), -float("inf")]], device=DEV)
    x[:min(n, 2)] = special[:min(n, 2)]
    if n > 2:
        x[2] = special[2]
    xb = _then_nan(x)

    def run():
        out = Guarded(n * feats, guard=feats)
        lib.check(L().mofa_positional_encode(lib.ptr(xb), n, nf, out.ptr(), lib.stream()), "positional_encode")
        torch.cuda.synchronize()
        return (out.check().reshape(n, feats),)

    (out,) = _twice(run)
    ref, ident = fr.positional_encode(x, nf)
    assert _same_bits(out[:, ident].contiguous(), x)
    finite = torch.isfinite(x).all(1)
    assert torch.isnan(out[~finite][:, ~ident]).all()
    err = (out[finite][:, ~ident].double() - ref[finite][:, ~ident]).abs()
    worst = float(err.max() / br.U32) if err.numel() else 0.0
    print(f"positional_encode nf={nf} n={n}: worst sine / cosine |err| / 2^-24 = {worst:.3f}")
    assert not (~(err <= br.C_PE * br.U32)).any(), worst


# ---- f. mofa_net_fold ---------------------------------------------------------------------------------------------------------------------
def _network(gen, D, W, nf, ch_exp=30, ch_shape=50, ch_tex=256):
    """A NeRF with asymmetric random weights (He-scaled, so activations keep their size through 2D + 5 layers) and its HipNet"""
    from mofanerf_amd.hipnet import HipNet
    from mofanerf_amd.model import NeRF
    net = NeRF(D=D, W=W, input_ch=3 + 6 * nf + ch_exp, input_ch_views=27, input_ch_textureCodes=ch_tex, input_ch_shapeCodes=ch_shape,
               use_viewdirs=True).to(DEV)
    with torch.no_grad():
        for lin in net.ordered_linears():
            lin.weight.copy_(_randn(gen, *lin.weight.shape, scale=(2.0 / lin.in_features) ** 0.5))
            lin.bias.copy_(_randn(gen, *lin.bias.shape, scale=0.1))
    h = HipNet(net, point_freqs=nf)
    ws, bs = h._weights()
    return h, ws, bs


@pytest.mark.parametrize("ch_exp,ch_shape,ch_tex", [(30, 50, 256), (0, 7, 33), (6, 0, 0)])
def test_net_fold_against_fp64(ch_exp, ch_shape, ch_tex):
    """mofa_net_fold slice by slice at the offsets of fr.net_plan: the five conditioned layers are bias + W[:, code columns] @ code, every
    other slice is a bit-equal copy of its bias, entries at or beyond n_out are 0, and the slices tile the blob (no NaN is left)."""
    gen = _gen(ch_exp + ch_shape + ch_tex)
    D, W = 8, 64
    h, ws, bs = _network(gen, D, W, 10, ch_exp, ch_shape, ch_tex)
    plan = fr.net_plan(D, W, 10, 4, ch_exp, ch_shape, ch_tex)
    n = L().mofa_net_folded_floats(h.shape)
    assert n == plan["folded_floats"]
    codes = {k: (_then_nan(_randn(gen, c)) if c else None) for k, c in (("exp", ch_exp), ("shape", ch_shape), ("tex", ch_tex))}

    def run():
        folded = Guarded(n)
        lib.check(L().mofa_net_fold(h.shape, lib.ptr_array(ws), lib.ptr_array(bs), lib.ptr(codes["exp"]), lib.ptr(codes["shape"]),
                                    lib.ptr(codes["tex"]), folded.ptr(), lib.stream()), "net_fold")
        torch.cuda.synchronize()
        return (folded.check(),)

    (folded,) = _twice(run)
    assert not torch.isnan(folded).any()
    conditioned = 0
    for li, l in enumerate(plan["layers"]):
        if l["fold"] and l["fold"][0] == "view":
            continue
        got = folded[l["folded_off"]:l["folded_off"] + l["n_padded"]]
        assert (got[l["n_out"]:] == 0).all(), li
        kind, col0, ncols = l["fold"] or (None, 0, 0)
        if ncols:
            ref, cond = fr.fold_bias(ws[li], col0, ncols, codes[kind][:ncols], bs[li])
            br.assert_close(got[:l["n_out"]], ref, cond, f"net_fold ({ch_exp}, {ch_shape}, {ch_tex}) layer {li} ({kind}, {ncols} columns at {col0})")
            conditioned += 1
        else:
            assert _same_bits(got[:l["n_out"]].contiguous(), bs[li]), li
    assert conditioned == (ch_exp > 0) + 2 * (ch_shape > 0) + 2 * (ch_tex > 0)


# ---- g. the tape audit --------------------------------------------------------------------------------------------------------------------
FORMS = {   # form: (knobs, D, W, R, S, verdict word [1] advances)
    "per-layer 8x64": ({"MOFA_FUSED": "0", "MOFA_CHAIN": "0"}, 8, 64, 9, 33, False),
    "per-layer 10x512": ({"MOFA_FUSED": "0", "MOFA_CHAIN": "0"}, 10, 512, 5, 64, False),
    "persistent pipelined 8x256": ({"MOFA_FUSED": "1"}, 8, 256, 9, 64, False),
    "persistent generic 10x96": ({"MOFA_FUSED": "1"}, 10, 96, 9, 33, False),
    "chained 10x512": ({}, 10, 512, 9, 64, True),
}


def _tape_audit(form, nf, explicit_points, knob):
    knobs, D, W, R, S, chained = FORMS[form]
    gen = _gen(D + W + nf + R)
    h, ws, bs = _network(gen, D, W, nf)                                            # (HipNet initialises the device: census + self-check)
    for name, value in knobs.items():
        knob(name, value)
    Lb, st = L(), lib.stream()
    plan = fr.net_plan(D, W, nf, 4, 30, 50, 256)
    M = R * S
    Mp = br.round_up(M, 256)
    o, d, z = _rays(gen, R, S)
    pts = br.points_from_rays(o, d, z).contiguous()
    vd = torch.nn.functional.normalize(_randn(gen, R, 3), dim=-1).contiguous()
    folded = h.fold(_randn(gen, 30), _randn(gen, 50), _randn(gen, 256)).clone()
    view = plan["layers"][plan["view"]]
    view_rows = torch.full((R, plan["Hp"]), NAN, device=DEV)
    lib.check(Lb.mofa_view_bias(lib.ptr(vd), R, 4, lib.ptr(ws[plan["view"]]), view["n_out"], view["ld"], lib.ptr(bs[plan["view"]]),
                                lib.ptr(view_rows), plan["Hp"], st), "view_bias")
    vrows = _then_nan(view_rows)
    packed = h.packed()
    n_tape = Lb.mofa_net_tape_floats(h.shape, M)
    assert n_tape == Mp * plan["tape_cols"]
    verdict = torch.zeros(lib.VERDICT_WORDS, dtype=torch.int32, device=DEV)
    src = (None, None, None, 0, lib.ptr(pts)) if explicit_points else (lib.ptr(o), lib.ptr(d), lib.ptr(z), S, None)

    def run(with_tape=True):
        ws_ = torch.full((Lb.mofa_net_workspace_floats(h.shape, M, R),), NAN, device=DEV)
        raw, tape = Guarded(M * 4), Guarded(n_tape if with_tape else 64)
        lib.check(Lb.mofa_net_forward(h.shape, lib.ptr(packed), lib.ptr(folded), None, None, *src, None, R, S, lib.ptr(ws_), raw.ptr(),
                                      tape.ptr() if with_tape else None, None, lib.ptr(vrows), verdict.data_ptr(), st), "net_forward")
        torch.cuda.synchronize()
        return raw.check().reshape(M, 4), tape.check()

    raw, tape = _twice(run)
    what = f"{form} nf={nf}{' explicit points' if explicit_points else ''}"
    worst = fr.audit_tape(plan, ws, pts, S, folded, view_rows, tape, raw, what=what)
    print(f"tape audit {what}: worst err / sum|ab| over {len(plan['layers'])} layers = {worst:.3e}")
    raw_inf, _ = run(False)                                                        # inference: four recycled buffers, the same bits
    assert _same_bits(raw_inf, raw), "raw_out differs between tape mode and inference mode"
    v = verdict.tolist()
    assert v[0] == 0, v
    assert v[1] == (3 if chained else 0), (form, v)                                # the chained launch really ran (only) where it should


@pytest.mark.parametrize("nf", [10, 16])
@pytest.mark.parametrize("form", list(FORMS))
def test_tape_audit_every_layer_of_every_launch_form(form, nf, knob):
    """mofa_net_forward with the fp32 tape: EVERY layer recomputed on its own in fp64 from the tape slots that feed it, the source weights
    and the device's own folded biases, every element of its slot held to the bound; layer 0 from the fp32 points (4 operand panels at
    10 frequencies, 8 at 16: k_layer<L0>, both persistent kernels' prologue, mofa_pe_panels for the 512-wide forms); the heads from their
    slots.  A fault shared by the per-layer form and its twin cannot hide here: nothing is compared with another launch form."""
    _tape_audit(form, nf, False, knob)


def test_tape_audit_from_explicit_points(knob):
    _tape_audit("per-layer 8x64", 10, True, knob)

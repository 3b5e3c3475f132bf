"""The comparator of tests/test_gpu_fwd_kernels.py must be able to fail.  For every forward operation: the fp64 restatement
(tests/fwd_reference.py) at the smallest shapes the GPU file uses, an honest fp32 evaluation — summed as one matmul and summed 16 columns
at a time, a skip layer h-first and x-first — that stays inside the GPU test's bound on every element, and the faults such kernels
usually have, each of which must put at least one element outside it.  `net_plan` is checked against the library's host functions.
Runs on the CPU; prints the honest evaluations' worst err / sum |a b| and the number of elements every fault puts outside the bound."""
import ctypes as C

import pytest
import torch

import bwd_reference as br
import fwd_reference as fr

BIG = 3e30
SENT = -7.25e11


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _mm(x, w, panels=False, order=None):
    """fp32 x @ w.T: one matmul, or summed 16 columns at a time (`order`: the column blocks [(first, end)] in summation order)"""
    if not panels:
        return x @ w.T
    acc = torch.zeros(x.shape[0], w.shape[0])
    for first, end in (order or [(0, x.shape[1])]):
        for k in range(first, end, 16):
            acc = acc + x[:, k:min(k + 16, end)] @ w[:, k:min(k + 16, end)].T
    return acc


def _outside(got, ref, cond, trig=None):
    """elements of got outside the bound (NaN counts)"""
    return int((~((got.double() - ref).abs() <= fr.bound(cond, trig))).sum())


def _honest(name, got, ref, cond, trig=None):
    assert got.shape == ref.shape
    assert _outside(got, ref, cond, trig) == 0, name
    ratio = br.worst_ratio(got, ref, cond)
    print(f"honest fp32 {name}: worst err / sum|ab| = {ratio:.3e}")
    return ratio


def _fault(name, got, ref, cond, trig=None):
    assert got.shape == ref.shape
    n = _outside(got, ref, cond, trig)
    print(f"fault {name}: {n} of {ref.numel()} elements outside the bound")
    assert n >= 1, name
    return n


def _pe32(x, n_freqs, sin=torch.sin, cos=torch.cos, freq=lambda f: 2.0 ** f, major="frequency"):
    """fp32 features of fp32 points; the keyword arguments are the faults"""
    blocks = [(sin(x * freq(f)), cos(x * freq(f))) for f in range(n_freqs)]
    if major == "frequency":
        return torch.cat([x] + [t for b in blocks for t in b], -1)
    per_coord = [torch.stack([t[:, c] for b in blocks for t in b], -1) for c in range(3)]      # coordinate-major: all of x's, then y's, ...
    return torch.cat([x] + per_coord, -1)


# ---- mofa_layer_forward ---------------------------------------------------------------------------------------------------------------------
def _layer_inputs(gen, k1, k2, Np, M):
    k1l, k2l, n_out = fr.logical(k1, k2, Np)
    x1, x2 = _rand(gen, M, k1l), (_rand(gen, M, k2l) if k2 else None)
    w, b = _rand(gen, n_out, k1l + k2l, scale=(k1l + k2l) ** -0.5), _rand(gen, n_out)
    return x1, x2, w, b


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("k1,k2,Np", fr.LAYER_CASES)
def test_layer_honest_fp32_stays_inside_the_bound(k1, k2, Np, relu):
    gen = torch.Generator().manual_seed(k1 + k2 + Np + relu)
    M = 256 - 68
    x1, x2, w, b = _layer_inputs(gen, k1, k2, Np, M)
    ref, cond = fr.layer(x1, w, b, x2, relu=bool(relu))
    x = x1 if x2 is None else torch.cat([x1, x2], 1)
    k1l = x1.shape[1]
    orders = [None] if x2 is None else [[(0, k1l), (k1l, x.shape[1])], [(k1l, x.shape[1]), (0, k1l)]]       # h-first, x-first
    for panels, order in [(False, None)] + [(True, o) for o in orders]:
        y = _mm(x, w, panels, order) + b
        _honest(f"layer {k1}+{k2}->{Np} relu={relu} panels={panels} order={order}", torch.relu(y) if relu else y, ref, cond)


def test_layer_comparator_sees_every_fault():
    gen = torch.Generator().manual_seed(11)
    for k1, k2, Np in ((32, 0, 128), (64, 0, 64), (96, 64, 192)):                 # fewest panels, the 64-feature tile, its skip layer
        M = 256 - 68
        x1, x2, w, b = _layer_inputs(gen, k1, k2, Np, M)
        x = x1 if x2 is None else torch.cat([x1, x2], 1)
        K, k1l = x.shape[1], x1.shape[1]
        ref, cond = fr.layer(x1, w, b, x2)
        tag = f"[{k1}+{k2}->{Np}]"
        _fault(f"{tag} last K column dropped", fr.layer(x[:, :-1], w[:, :-1], b)[0], ref, cond)
        keep = [k for k in range(K) if not 16 <= k < 32]
        _fault(f"{tag} one 16-column panel dropped", fr.layer(x[:, keep], w[:, keep], b)[0], ref, cond)
        _fault(f"{tag} ReLU missing", fr.layer(x1, w, b, x2, relu=False)[0], ref, cond)
        lin, cond_lin = fr.layer(x1, w, b, x2, relu=False)
        _fault(f"{tag} ReLU applied at relu = 0", ref, lin, cond_lin)
        wide = _rand(gen, w.shape[0], K + 9, scale=K ** -0.5)                      # w is columns [5, 5 + K) of a wider matrix
        r5, c5 = fr.layer(x, wide[:, 5:5 + K], b)
        _fault(f"{tag} column offset shifted by one", fr.layer(x, wide[:, 6:6 + K], b)[0], r5, c5)
        _fault(f"{tag} bias forgotten", fr.layer(x1, w, torch.zeros_like(b), x2)[0], ref, cond)
        # one swizzled 4-float chunk of the input panels / of the output panels exchanged with its neighbour
        xs = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(x, 256), 256, 100, 21), 256, br.round_up(K, 16))[:M, :K]
        _fault(f"{tag} one chunk of X swapped", fr.layer(xs, w, b)[0], ref, cond)
        ys = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(ref, 256, k_padded=Np), 256, 100, 21), 256, Np)[:M, :w.shape[0]]
        _fault(f"{tag} one chunk of Y swapped", ys, ref, cond)
        if x2 is not None:
            swapped = torch.cat([w[:, k1l:], w[:, :k1l]], 1)                       # the x2 block of the weight meets x1
            _fault(f"{tag} x1 and x2 blocks of the weight exchanged", fr.layer(x, swapped, b)[0], ref, cond)


@pytest.mark.parametrize("div", fr.BIAS_DIVS)
def test_per_ray_bias_comparator_sees_a_shifted_row_and_a_missing_clamp(div):
    """700 points in 768 rows, ceil(700 / div) bias rows.  The clamp matters only in the padding rows (m // div of a valid row is a valid
    bias row), so the GPU test compares ALL 768 rows there: the padding rows of X hold +-BIG, which hides any finite bias, and the
    buffer holds NaN behind the last row, which nothing hides."""
    gen = torch.Generator().manual_seed(div)
    n, Mp, k1, Np = 700, 768, 64, 64
    k1l, _, n_out = fr.logical(k1, 0, Np)
    rows = -(-n // div)
    x, w = _rand(gen, Mp, k1l), _rand(gen, n_out, k1l, scale=k1l ** -0.5)
    x[n:] = BIG * torch.sign(x[n:])
    bias_rows = _rand(gen, rows, n_out)
    for relu in (False, True):
        ref, cond = fr.layer(x, w, None, relu=relu, bias_rows=bias_rows, div=div)
        row = (torch.arange(Mp) // div).clamp_max(rows - 1)
        y = _mm(x, w) + bias_rows[row]
        _honest(f"per-ray bias div={div} relu={relu}", torch.relu(y) if relu else y, ref, cond)
        nxt = ((torch.arange(Mp) + 1) // div).clamp_max(rows - 1)
        y = x.double() @ w.double().T + bias_rows.double()[nxt]
        _fault(f"bias row of (m + 1) // {div} relu={relu}", (torch.relu(y) if relu else y)[:n], ref[:n], cond[:n])
        if not relu:                                                               # (a ReLU computed as max(v, 0) turns NaN into 0)
            behind = torch.cat([bias_rows, torch.full((Mp, n_out), float("nan"))])
            y = x.double() @ w.double().T + behind.double()[torch.arange(Mp) // div]
            if (torch.arange(Mp) // div).max() >= rows:
                _fault(f"clamp missing div={div}: NaN behind the last row", y, ref, cond)
    # with ordinary values in the padding rows a finite sentinel row shows as well
    x[n:] = _rand(gen, Mp - n, k1l)
    ref, cond = fr.layer(x, w, None, relu=False, bias_rows=bias_rows, div=div)
    if (Mp - 1) // div >= rows:
        behind = torch.cat([bias_rows, torch.full((Mp, n_out), SENT)])
        _fault(f"clamp missing div={div}: sentinel row", x.double() @ w.double().T + behind.double()[torch.arange(Mp) // div], ref, cond)


# ---- layer 0, the view bias, the encoding itself ------------------------------------------------------------------------------------------
def _points(gen, R, S):
    o = torch.rand(R, 3, generator=gen) * 6 - 3
    d = _rand(gen, R, 3, scale=0.6)
    z = torch.sort(torch.rand(R, S, generator=gen) * 18 + 8, -1)[0]
    return br.points_from_rays(o, d, z)


@pytest.mark.parametrize("R,S", fr.LAYER0_RAYS)
@pytest.mark.parametrize("nf", fr.LAYER0_FREQS)
def test_layer0_honest_fp32_stays_inside_the_bound(nf, R, S):
    gen = torch.Generator().manual_seed(nf + R + S)
    feats, n_out = 3 + 6 * nf, 61
    pts = _points(gen, R, S)
    w, b = _rand(gen, n_out, feats, scale=1 / 8), _rand(gen, n_out)
    ref, cond, trig = fr.layer0(pts, nf, w, b)
    pe = _pe32(pts, nf)
    for panels in (False, True):
        _honest(f"layer0 nf={nf} {R}x{S} panels={panels}", torch.relu(_mm(pe, w, panels) + b), ref, cond, trig)
    err = (pe.double() - br.pe_features(pts, nf)).abs().max() / br.U32
    print(f"fp32 sin / cos of arguments up to 2^{max(nf - 1, 0)} x: worst |err| / 2^-24 = {float(err):.3f}")
    assert err <= br.C_PE


def test_encoding_comparators_see_every_fault():
    gen = torch.Generator().manual_seed(12)
    for nf in (4, 16):
        feats, n_out = 3 + 6 * nf, 61
        pts = _points(gen, 5, 37)
        w, b = _rand(gen, n_out, feats, scale=1 / 8), _rand(gen, n_out)
        ref, cond, trig = fr.layer0(pts, nf, w, b)
        vd = torch.nn.functional.normalize(_rand(gen, 8, 3), dim=-1)
        wv, bv = _rand(gen, 96, feats + 13, scale=1 / 5), _rand(gen, 96)
        vref, vcond, vtrig = fr.view_bias(vd, nf, wv, bv)
        _honest(f"view_bias nf={nf}", _pe32(vd, nf) @ wv[:, :feats].T + bv, vref, vcond, vtrig)
        pref, ident = fr.positional_encode(pts, nf)
        lim = torch.where(ident, torch.zeros(()), torch.full((), br.C_PE * br.U32)).double()[None, :].expand_as(pref)
        assert not br.exceeds(_pe32(pts, nf), pref, lim)
        for name, kw in (("sine and cosine exchanged", dict(sin=torch.cos, cos=torch.sin)), ("frequency 2^(f+1)", dict(freq=lambda f: 2.0 ** (f + 1))),
                         ("coordinate-major feature order", dict(major="coordinate"))):
            bad = _pe32(pts, nf, **kw).double()
            _fault(f"nf={nf} layer0: {name}", torch.relu(bad @ w.double().T + b.double()), ref, cond, trig)
            _fault(f"nf={nf} view_bias: {name}", _pe32(vd, nf, **kw).double() @ wv[:, :feats].double().T + bv.double(), vref, vcond, vtrig)
            assert br.exceeds(_pe32(pts, nf, **kw), pref, lim), name
        # the point not rounded to fp32 before it is encoded: 2^(nf-1) amplifies half an ulp of x
        _fault(f"nf={nf} layer0: point half an ulp off", fr.layer0(torch.nextafter(pts, torch.full_like(pts, 99.0)), nf, w, b)[0], ref, cond, trig)
        # a non-zero padding feature: invisible while the packed weight is zero there, so the GPU test fills the weight's padding columns
        kp = br.round_up(feats, 64)
        wj = torch.full((n_out, kp), 0.75, dtype=torch.float64)
        wj[:, :feats] = w.double()
        pan = br.pe_panels(pts, nf, 256, kp)[:pts.shape[0]]
        assert not br.exceeds(torch.relu(pan @ wj.T + b.double()), ref, fr.bound(cond, trig))
        pan[:, feats] = 1e-3
        _fault(f"nf={nf} layer0: a non-zero padding feature", torch.relu(pan @ wj.T + b.double()), ref, cond, trig)
        # ... and in the panels themselves the padding features are exactly 0
        full = br.pe_panels(pts, nf, 256, kp)
        bad = full.clone()
        bad[7, kp - 1] = 1e-30
        assert br.exceeds(bad, full, torch.full_like(full, 0.0)) and not br.exceeds(full, full, torch.full_like(full, 0.0))
        # one swizzled chunk of the output
        ys = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(ref, 256, k_padded=64), 256, 100, 21), 256, 64)[:ref.shape[0], :n_out]
        _fault(f"nf={nf} layer0: one chunk of Y swapped", ys, ref, cond, trig)


# ---- heads and folded biases ----------------------------------------------------------------------------------------------------------------
def test_head_comparator_sees_every_fault():
    gen = torch.Generator().manual_seed(13)
    for n, kp in ((1, 64), (700, 64), (700, 528)):
        kl = kp - 5
        x = _rand(gen, n, kl)
        for raw_off, n_out in ((0, 3), (3, 1), (0, 4), (1, 2)):
            w, b = _rand(gen, n_out, kl, scale=1 / 8), _rand(gen, n_out)
            ref, cond = fr.head(x, w, b)
            _honest(f"head off={raw_off} n_out={n_out} kp={kp} n={n}", x @ w.T + b, ref, cond)
            _honest(f"head off={raw_off} n_out={n_out} kp={kp} n={n} panels", _mm(x, w, True) + b, ref, cond)

            def place(off):                                                        # raw [n, 4] pre-filled with the sentinel
                raw = torch.full((n, 5), SENT, dtype=torch.float64)
                raw[:, off:off + n_out] = ref
                return raw[:, :4]
            lim = torch.full((n, 4), br.TINY, dtype=torch.float64)
            lim[:, raw_off:raw_off + n_out] = fr.bound(cond)
            assert not br.exceeds(place(raw_off), place(raw_off), lim)
            moved = int((~((place(raw_off + 1) - place(raw_off)).abs() <= lim)).sum())
            print(f"fault head: written at raw_off + 1: {moved} of {lim.numel()} elements outside the bound")
            assert moved >= 1
            _fault("head: last K column dropped", fr.head(x[:, :-1], w[:, :-1], b)[0], ref, cond)
            _fault("head: bias forgotten", fr.head(x, w, torch.zeros_like(b))[0], ref, cond)
            if n > 1:
                xs = br.unpack_panels(br.swap_chunk_with_neighbour(br.pack_panels(x, 768, k_padded=kp), 768, 333, 21), 768, kp)[:n, :kl]
                _fault("head: one chunk of X swapped", fr.head(xs, w, b)[0], ref, cond)


def test_fold_comparator_sees_every_fault():
    gen = torch.Generator().manual_seed(14)
    for n_out, col0, ncols, ld in ((64, 63, 30, 93), (64, 0, 50, 114), (64, 0, 7, 135), (64, 0, 256, 320), (64, 0, 33, 97), (64, 63, 6, 69)):
        w, code, bias = _rand(gen, n_out, ld + 1, scale=ld ** -0.5), _rand(gen, ncols), _rand(gen, n_out)
        ref, cond = fr.fold_bias(w, col0, ncols, code, bias)
        acc = torch.zeros(n_out)
        for c in range(ncols):                                                     # k_fold_bias's order: the columns one by one, then the bias
            acc = acc + w[:, col0 + c] * code[c]
        _honest(f"fold {ncols} columns at {col0}", acc + bias, ref, cond)
        _honest(f"fold {ncols} columns at {col0} (one matmul)", w[:, col0:col0 + ncols] @ code + bias, ref, cond)
        _fault("fold: code columns read from col0 + 1", fr.fold_bias(w, col0 + 1, ncols, code, bias)[0], ref, cond)
        _fault("fold: bias forgotten", fr.fold_bias(w, col0, ncols, code, torch.zeros_like(bias))[0], ref, cond)
        _fault("fold: last code column dropped", fr.fold_bias(w, col0, ncols - 1, code[:-1], bias)[0], ref, cond)
    ref, cond = fr.fold_bias(w, 0, 0, None, bias)                                  # a code of width 0: the bias itself, exactly
    assert torch.equal(ref, bias.double()) and br.exceeds(bias + 1e-7, ref, fr.bound(cond))


# ---- net_plan against the library's host functions -----------------------------------------------------------------------------------------
SHAPES = [(8, 64, 10, 4, 30, 50, 256), (10, 512, 10, 4, 30, 50, 256), (10, 512, 16, 4, 30, 50, 256), (8, 256, 16, 4, 30, 50, 256),
          (10, 96, 10, 4, 30, 50, 256), (8, 64, 10, 4, 0, 7, 33), (8, 64, 10, 4, 6, 0, 0), (8, 256, 16, 16, 0, 0, 0), (10, 1024, 0, 0, 30, 50, 64)]


@pytest.mark.parametrize("shape", SHAPES)
def test_net_plan_matches_the_library(shape):
    from mofanerf_amd import lib, schema
    L = lib.load()
    D, W, mr, mv, ce, cs, ct = shape
    s = lib.NetShape(*shape)
    p = fr.net_plan(*shape)
    assert L.mofa_net_num_layers(s) == len(p["layers"]) == 2 * D + 7
    no, ni = C.c_int32(), C.c_int32()
    want = list(schema.nerf_layers(D, W, ch_pts=3 + 6 * mr + ce, ch_shape=cs, ch_tex=ct, ch_views=3 + 6 * mv).values())
    for li, l in enumerate(p["layers"]):
        assert L.mofa_net_layer_dims(s, li, C.byref(no), C.byref(ni)) == 0
        assert (no.value, ni.value) == (l["n_out"], l["ld"]) == tuple(want[li]), li
        for c0, nc, kp in l["parts"]:
            assert 0 <= c0 and c0 + nc <= l["ld"] and nc <= kp and kp % 16 == 0
        covered = [c for c0, nc, _ in l["parts"] for c in range(c0, c0 + nc)]      # per-point columns + constant columns = every column, once
        covered += list(range(l["fold"][1], l["fold"][1] + l["fold"][2])) if l["fold"] else []
        assert sorted(covered) == list(range(l["ld"])), li
    assert sum(not l["head"] for l in p["layers"]) == 2 * D + 5
    for n in (1, 700, 4096):
        assert L.mofa_net_tape_floats(s, n) == br.round_up(n, 256) * p["tape_cols"]
    assert L.mofa_net_folded_floats(s) == p["folded_floats"]
    assert L.mofa_pe_k_padded(mr) == p["pe_k"]
    sk = p["layers"][p["bim_skip"]]                                                 # the skip layer: h columns first, then x
    assert sk["parts"] == [(cs + W, W, p["Wp"]), (cs, W, p["Wp"])] and sk["inputs"] == [p["bim_skip"] - 1, p["bim0"] - 1]
    assert p["layers"][p["uv_skip"]]["inputs"] == [p["uv_skip"] - 1, p["sigma"]] and p["layers"][p["alpha"]]["inputs"] == [p["sigma"]]
    assert p["layers"][p["view"]]["folded_off"] == p["layers"][p["alpha"]]["folded_off"]       # the view layer takes no slice


# ---- the tape audit -------------------------------------------------------------------------------------------------------------------------
def _fp32_network(plan, gen, R, S, panels):
    """An honest fp32 evaluation of mofa_net_fold + mofa_view_bias + mofa_net_forward with the fp32 tape, in torch: what the audit is given."""
    L, M = plan["layers"], R * S
    Mp = br.round_up(M, 256)
    weights = [_rand(gen, l["n_out"], l["ld"], scale=(2.0 / l["ld"]) ** 0.5) for l in L]
    biases = [_rand(gen, l["n_out"], scale=0.1) for l in L]
    codes = {k: _rand(gen, n) for k, n in (("exp", L[0]["fold"][2]), ("shape", L[plan["bim0"]]["fold"][2]), ("tex", L[plan["uv0"]]["fold"][2]))}
    pts = _points(gen, R, S)
    vd = torch.nn.functional.normalize(_rand(gen, R, 3), dim=-1)
    folded = torch.zeros(plan["folded_floats"])
    outs, tape = {}, torch.zeros(Mp * plan["tape_cols"])
    raw = torch.zeros(M, 4)
    view_rows = torch.zeros(R, plan["Hp"])
    for li, l in enumerate(L):
        w, n_out = weights[li], l["n_out"]
        if l["fold"] and l["fold"][0] == "view":
            view_rows[:, :n_out] = _pe32(vd, plan["pe_view_freqs"]) @ w[:, :l["fold"][2]].T + biases[li]
            b = view_rows[torch.arange(M) // S, :n_out]
        else:
            b = biases[li]
            if l["fold"] and l["fold"][2]:
                b = b + w[:, l["fold"][1]:l["fold"][1] + l["fold"][2]] @ codes[l["fold"][0]]
            folded[l["folded_off"]:l["folded_off"] + n_out] = b
        xs = [(_pe32(pts, plan["pe_point_freqs"]) if i == "pe" else outs[i])[:, :nc] for i, (_, nc, _) in zip(l["inputs"], l["parts"])]
        y = sum(_mm(x, w[:, c0:c0 + nc], panels) for x, (c0, nc, _) in zip(xs, l["parts"])) + b
        if l["head"]:
            off = 3 if li == plan["alpha"] else 0
            raw[:, off:off + n_out] = y
        else:
            outs[li] = torch.relu(y)
            t0 = Mp * l["tape_cols"]
            tape[t0:t0 + Mp * l["n_padded"]] = br.pack_panels(outs[li], Mp, k_padded=l["n_padded"])
    return weights, pts, folded, view_rows, tape, raw


@pytest.mark.parametrize("panels", [False, True])
@pytest.mark.parametrize("D,W,nf,R,S", [(8, 64, 10, 9, 33), (8, 64, 16, 9, 33), (10, 96, 16, 9, 33)])
def test_tape_audit_passes_an_honest_network_and_sees_every_fault(D, W, nf, R, S, panels):
    gen = torch.Generator().manual_seed(D + W + nf)
    plan = fr.net_plan(D, W, nf, 4, 30, 50, 256)
    weights, pts, folded, view_rows, tape, raw = _fp32_network(plan, gen, R, S, panels)
    worst = fr.audit_tape(plan, weights, pts, S, folded, view_rows, tape, raw, what=f"honest fp32 network {D}x{W} nf={nf} panels={panels}")
    assert worst < br.C_CONTRACTION
    if panels:
        return

    def outside(plan_, weights_=weights, pts_=pts, S_=S, folded_=folded, view_rows_=view_rows, tape_=tape, raw_=raw):
        return {name: _outside(got, ref, cond, trig) + (0 if pad is None else int((pad != 0).sum()))
                for name, got, ref, cond, trig, pad in fr.audit_items(plan_, weights_, pts_, S_, folded_, view_rows_, tape_, raw_)}

    def report(name, res, must):
        hit = {k: v for k, v in res.items() if v}
        print(f"fault {name}: layers outside the bound {hit}")
        for m in must:
            assert res[m] >= 1, (name, m)

    Mp = br.round_up(R * S, 256)
    for li in (plan["xyz0"] + 1, plan["bim_skip"], plan["view"]):                  # a tape slot offset by one layer
        bad = dict(plan, layers=[dict(l) for l in plan["layers"]])
        bad["layers"][li]["tape_cols"] = plan["layers"][li + 1 if li != plan["view"] else li - 1]["tape_cols"]
        report(f"tape slot of layer {li} offset by one layer", outside(bad), [f"layer {li}"])
    sk = plan["bim_skip"]                                                          # the skip layer's two K sources exchanged
    bad = dict(plan, layers=[dict(l) for l in plan["layers"]])
    bad["layers"][sk]["inputs"] = plan["layers"][sk]["inputs"][::-1]
    report("skip layer: h and x sources exchanged", outside(bad), [f"layer {sk}"])
    t = tape.clone()                                                               # one swizzled chunk of one slot: the layer itself and its consumer
    l = plan["layers"][plan["uv0"]]
    t0 = Mp * l["tape_cols"]
    t[t0:t0 + Mp * l["n_padded"]] = br.swap_chunk_with_neighbour(tape[t0:t0 + Mp * l["n_padded"]], Mp, 100, 21)
    report("one chunk of a tape slot swapped", outside(plan, tape_=t), [f"layer {plan['uv0']}", f"layer {plan['uv0'] + 1}"])
    report("per-ray bias rows of ray r + 1", outside(plan, view_rows_=view_rows.roll(-1, 0)), [f"layer {plan['view']}"])
    report("sigma head written to column 2", outside(plan, raw_=raw[:, [0, 1, 3, 2]]), [f"layer {plan['alpha']} (head)", f"layer {plan['rgb']} (head)"])
    f2 = folded.clone()                                                            # a folded slice read one float off
    off = plan["layers"][plan["bim0"]]["folded_off"]
    f2[off:off + W] = folded[off + 1:off + W + 1]
    report("folded bias read from offset + 1", outside(plan, folded_=f2), [f"layer {plan['bim0']}"])
    report("points of the neighbouring sample", outside(plan, pts_=pts.roll(1, 0)), [f"layer {plan['xyz0']}"])

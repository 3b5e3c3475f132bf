"""Plain fp64 restatements of the forward kernels' arithmetic (tests only): one function per operation of the forward C ABI, each returning
(value, cond) — cond is sum |a b| of the same contraction plus |bias|, what the rounding-level bound of tests/test_gpu_fwd_kernels.py is
stated in — and, where sines and cosines enter, a third tensor `trig` = sum |w| over the sine / cosine features (the device's sinf / cosf
err by a few 2^-24 per feature, whatever the feature's own size).  Plus `net_plan`, a restatement of make_plan (csrc/mofa_net.hip): which
columns every layer contracts, which earlier outputs feed it, where its tape slot and its folded bias lie.  torch only (any device), no
call into the library; panel layout, bound and comparison come from tests/bwd_reference.py.  tests/test_fwd_reference_cpu.py shows that
every fault these comparisons are meant to see does break the bound."""
import torch

import bwd_reference as br


def bound(cond, trig=None):
    """|got - ref64| <= C_CONTRACTION * cond + TINY (+ C_PE * 2^-24 * trig): bwd_reference's constants, unchanged"""
    return br.bound(cond, trig)


# ---- the operations: (value, cond[, trig]) in fp64 ----------------------------------------------------------------------------------------
def layer(x1, w, bias, x2=None, relu=True, bias_rows=None, div=0):
    """act([x1 | x2] @ w.T + b): x1 [M, k1], x2 [M, k2] or None, w [N, k1 + k2]; b = bias [N], or bias_rows[min(m // div, rows - 1)]."""
    x = (x1 if x2 is None else torch.cat([x1, x2], 1)).double()
    w = w.double()
    if bias_rows is None:
        b = bias.double()[None, :]
    else:
        row = (torch.arange(x.shape[0], device=x.device) // div).clamp_max(bias_rows.shape[0] - 1)
        b = bias_rows.double()[row]
    val, cond = x @ w.T + b, x.abs() @ w.abs().T + b.abs()
    return (torch.relu(val) if relu else val), cond


def layer0(points, n_freqs, w, bias):
    """relu(PE(x) @ w[:, :3 + 6 f].T + b) at the fp32 points x [M, 3] (2^f x is exact in fp32: fp64 sin / cos of it is the true value)."""
    feats = 3 + 6 * n_freqs
    pe, w, b = br.pe_features(points, n_freqs), w.double()[:, :feats], bias.double()[None, :]
    trig = w[:, 3:].abs().sum(1)[None, :].expand(pe.shape[0], -1)
    return torch.relu(pe @ w.T + b), pe.abs() @ w.abs().T + b.abs(), trig


def head(x, w, b):
    """x @ w.T + b, no activation: x [M, K], w [n_out, K], b [n_out]."""
    x, w, b = x.double(), w.double(), b.double()[None, :]
    return x @ w.T + b, x.abs() @ w.abs().T + b.abs()


def view_bias(viewdirs, n_freqs, w, bias):
    """bias + w[:, :3 + 6 f] @ PE(viewdir) per ray: viewdirs [R, 3] fp32, w [n_out, ld >= 3 + 6 f]."""
    feats = 3 + 6 * n_freqs
    pe, w, b = br.pe_features(viewdirs, n_freqs), w.double()[:, :feats], bias.double()[None, :]
    trig = w[:, 3:].abs().sum(1)[None, :].expand(pe.shape[0], -1)
    return pe @ w.T + b, pe.abs() @ w.abs().T + b.abs(), trig


def fold_bias(w, col0, ncols, code, bias):
    """bias + w[:, col0:col0 + ncols] @ code (ncols = 0 or code = None: the bias itself, exactly)."""
    b = bias.double()
    if code is None or ncols == 0:
        return b.clone(), b.abs()
    wc, c = w.double()[:, col0:col0 + ncols], code.double().reshape(-1)
    return b + wc @ c, b.abs() + wc.abs() @ c.abs()


def positional_encode(x, n_freqs):
    """[x, sin(2^0 x), cos(2^0 x), ...] in fp64 and a bool per feature: is it one of the three identity features?"""
    ident = torch.zeros(3 + 6 * n_freqs, dtype=torch.bool, device=x.device)
    ident[:3] = True
    return br.pe_features(x, n_freqs), ident


# ---- the network's plan (make_plan, csrc/mofa_net.hip) ------------------------------------------------------------------------------------
def net_plan(D, W, pe_point_freqs=10, pe_view_freqs=4, ch_exp=30, ch_shape=50, ch_tex=256):
    """The 2D + 7 Linear layers in state-dict order.  Per layer: n_out, ld (PyTorch weight [n_out, ld]), n_padded, head,
    parts = [(col0, ncols, k_padded)] — the per-point column ranges in contraction order (a skip layer: part 0 the h columns
    [cin + W, cin + 2W), part 1 the x columns [cin, cin + W)) —, inputs = the layer whose output feeds each part ("pe": the encoded point),
    fold = (which code, col0, ncols) of the per-call-constant columns, tape_cols = sum of n_padded of the MFMA layers before it,
    folded_off = its slice of the folded-bias blob (n_padded floats; heads 4; the view layer none: its bias is per ray)."""
    Wp, Hp = br.round_up(W, 64), br.round_up(W // 2, 64)
    PE, PV = 3 + 6 * pe_point_freqs, 3 + 6 * pe_view_freqs
    pe_k = br.round_up(PE, 64)
    L = []

    def add(n_out, ld, parts, inputs, fold=None, n_padded=None, head=False):
        L.append(dict(n_out=n_out, ld=ld, parts=parts, inputs=inputs, fold=fold, head=head,
                      n_padded=br.round_up(n_out, 64) if n_padded is None else n_padded))
        return len(L) - 1

    def plain():
        return add(W, W, [(0, W, Wp)], [len(L) - 1])

    xyz0 = add(W, PE + ch_exp, [(0, PE, pe_k)], ["pe"], fold=("exp", PE, ch_exp))
    for _ in range(3):
        plain()

    def stack(cin, code):
        x = len(L) - 1                                                     # the stack's input: the previous stack's last layer
        first = add(W, cin + W, [(cin, W, Wp)], [x], fold=(code, 0, cin))
        for _ in range(4):
            plain()
        skip = add(W, cin + 2 * W, [(cin + W, W, Wp), (cin, W, Wp)], [len(L) - 1, x], fold=(code, 0, cin))
        for _ in range(D - 6):
            plain()
        return first, skip

    bim0, bim_skip = stack(ch_shape, "shape")
    sigma = len(L) - 1
    uv0, uv_skip = stack(ch_tex, "tex")
    view = add(W // 2, PV + W, [(PV, W, Wp)], [len(L) - 1], fold=("view", 0, PV), n_padded=Hp)
    alpha = add(1, W, [(0, W, Wp)], [sigma], n_padded=4, head=True)
    rgb = add(3, W // 2, [(0, W // 2, Hp)], [view], n_padded=4, head=True)
    tape_cols = folded = 0
    for l in L:
        l["tape_cols"], l["folded_off"] = tape_cols, folded
        if not l["head"]:
            tape_cols += l["n_padded"]
        if not (l["fold"] and l["fold"][0] == "view"):
            folded += l["n_padded"]
    return dict(D=D, W=W, Wp=Wp, Hp=Hp, pe_k=pe_k, pe_point_freqs=pe_point_freqs, pe_view_freqs=pe_view_freqs, layers=L, tape_cols=tape_cols, folded_floats=folded, xyz0=xyz0, bim0=bim0,
                bim_skip=bim_skip, sigma=sigma, uv0=uv0, uv_skip=uv_skip, view=view, alpha=alpha, rgb=rgb)


def tape_slot(tape, plan, li, m_padded):
    """Layer li's output in the fp32 tape (every MFMA layer's panels back to back) as a logical matrix [m_padded, n_padded]."""
    l = plan["layers"][li]
    off = m_padded * l["tape_cols"]
    return br.unpack_panels(tape[off:off + m_padded * l["n_padded"]], m_padded, l["n_padded"])


def layer_from_tape(plan, li, slots, weights, bias, n_points, bias_rows=None, div=0):
    """Layer li (not layer 0, not a head) recomputed in fp64 from the outputs `slots[input]` [>= n_points, >= ncols] of the layers that
    feed it, the source weight tensors and the bias the device used (its folded slice, or the per-ray rows of the view layer)."""
    l = plan["layers"][li]
    xs = [slots[i][:n_points, :nc] for i, (_, nc, _) in zip(l["inputs"], l["parts"])]
    ws = [weights[li][:, c0:c0 + nc] for c0, nc, _ in l["parts"]]
    return layer(xs[0], torch.cat(ws, 1), None if bias is None else bias[:l["n_out"]], xs[1] if len(xs) > 1 else None,
                 relu=True, bias_rows=None if bias_rows is None else bias_rows[:, :l["n_out"]], div=div)


def audit_items(plan, weights, points, S, folded, view_rows, tape, raw):
    """The tape audit: every layer of one mofa_net_forward call recomputed on its own in fp64 FROM WHAT THE CALL ITSELF WROTE — its inputs
    are the fp32 tape slots of the layers that feed it, its bias the folded blob (the view layer: the per-ray rows) — so an error does not
    travel: a layer is judged on its own rounding.  (ReLU is 1-Lipschitz: the bound of the pre-activation holds behind it.)
    points [M, 3] fp32; folded [folded_floats]; view_rows [n_rays, Hp]; tape [m_padded * tape_cols]; raw [M, 4].
    Yields (name, got [M, n_out], ref, cond, trig or None, padding columns of got [M, n_padded - n_out] or None) per layer."""
    M = points.shape[0]
    Mp = br.round_up(M, br.ROW_TILE)
    L = plan["layers"]
    slots = {li: tape_slot(tape, plan, li, Mp) for li, l in enumerate(L) if not l["head"]}
    for li, l in enumerate(L):
        n_out, bias = l["n_out"], folded[l["folded_off"]:l["folded_off"] + l["n_out"]]
        if l["head"]:
            nc = l["parts"][0][1]
            ref, cond = head(slots[l["inputs"][0]][:M, :nc], weights[li], bias)
            got = raw[:, 3:4] if li == plan["alpha"] else raw[:, 0:3]
            yield f"layer {li} (head)", got, ref, cond, None, None
            continue
        trig = None
        if li == plan["xyz0"]:
            ref, cond, trig = layer0(points, plan["pe_point_freqs"], weights[li], bias)
        elif li == plan["view"]:
            ref, cond = layer_from_tape(plan, li, slots, weights, None, M, bias_rows=view_rows, div=S)
        else:
            ref, cond = layer_from_tape(plan, li, slots, weights, bias, M)
        yield f"layer {li}", slots[li][:M, :n_out], ref, cond, trig, slots[li][:M, n_out:]


def audit_tape(plan, weights, points, S, folded, view_rows, tape, raw, what=""):
    """Assert every element of every layer (valid rows) inside its bound and the padding features exactly 0; returns the worst
    err / sum |a b| over the layers."""
    worst = 0.0
    for name, got, ref, cond, trig, pad in audit_items(plan, weights, points, S, folded, view_rows, tape, raw):
        worst = max(worst, br.assert_close(got, ref, cond, f"{what} {name}", trig=trig))
        assert pad is None or (pad == 0).all(), f"{what} {name}: a padding feature is not 0"
    return worst


# ---- the shapes tests/test_gpu_fwd_kernels.py runs (tests/test_fwd_reference_cpu.py injects its faults at the smallest of them) -------------
LAYER_CASES = [(64, 0, 128), (48, 0, 128), (32, 0, 128), (1024, 0, 128), (128, 128, 256), (64, 0, 64), (96, 64, 192)]   # (k1, k2, Np)
BIAS_DIVS = [1, 33, 64, 300]
LAYER0_FREQS = [0, 4, 10, 11, 16]
LAYER0_RAYS = [(1, 1), (5, 37), (9, 130)]


def logical(k1, k2, n_padded):
    """The un-padded widths a (k1, k2, Np) case runs at: no multiple of anything, so every padding column and feature is exercised."""
    return k1 - 1, (k2 - 3 if k2 else 0), n_padded - 3

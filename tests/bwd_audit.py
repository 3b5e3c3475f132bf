"""The one-hot audit of mofa_net_backward (tests only): torch, no call into the library; serves a GPU call and a CPU emulation alike.

The backward keeps no tape of its gradients, but the training form returns every one of them as a sum: d_folded[layer l] = sum_m G_l[m, :]
(G_l: the masked gradient at layer l's output), d_view_bias_rows the same per ray for the view layer.  With d_raw zero except at one point
m*, every G_l is zero off row m*, every such sum has ONE non-zero term, and x + 0 is exact in any order: d_folded then holds the device's
own G_l[m*, :], layer by layer.  As in the forward tape audit (fwd_reference.audit_tape) an error does not travel: every layer is judged
on its own rounding, G_{l-1}[m*] = mask_{l-1}[m*] (G_l[m*] W_l) recomputed in fp64 FROM THE VALUES THE DEVICE ITSELF REPORTED one layer
downstream, every weight gradient is one outer product G_l[m*]^T X_{l-1}[m*] of two things the test can read.  The bound is
bwd_reference.bound with its constants unchanged.  tests/test_bwd_audit_cpu.py shows that an honest fp32 evaluation passes and that every
fault the host function could have breaks it."""
import torch

import bwd_reference as br
import fwd_reference as fr
from mofanerf_amd import schema
from oracle import mofa_oracle as orc

SENT = -7.25e11          # what the constant columns of d_weights hold before the call (tests/test_gpu_bwd_kernels.py's sentinel)
PATTERNS = ("all four", "only sigma", "only rgb")      # d_raw at the hot row: every channel / only channel 3 / only channels 0..2
HOT_ROWS = (0, 240, 255, 256, 299)                     # of M = 300 points: first, last of row tile 0, first of the ragged tile, M - 1; and 240,
M_POINTS, RAYS, SAMPLES = 300, 5, 60                   # the first sample of the last ray (where per-ray sums over S + 1 samples would show)
NETS = {"8x64": (8, 64, 10, 82), "8x96": (8, 96, 10, 114), "10x128": (10, 128, 10, 148), "8x256": (8, 256, 10, 274),   # name: (D, W, point
        "10x512": (10, 512, 10, 532), "8x64 nf16": (8, 64, 16, 88)}                                                     # frequencies, seed)


# ---- inputs: made on the CPU from a seed, so that the GPU test and the CPU emulation see the same network and points ----------------------
def make_case(D, W, nf, seed, R=RAYS, S=SAMPLES, shared_z=False):
    """A network with asymmetric random weights (He-scaled: activations and gradients keep their size through 2D + 5 layers), codes,
    rays (o in +-3, |d| about 0.6, z in [8, 26]: coordinates up to about 20) and unit view directions, all fp32 CPU tensors."""
    gen = torch.Generator().manual_seed(seed)
    plan = fr.net_plan(D, W, nf, 4, 30, 50, 256)
    names = list(schema.nerf_layers(D, W, ch_pts=3 + 6 * nf + 30))
    assert len(names) == len(plan["layers"])
    weights = [torch.randn(l["n_out"], l["ld"], generator=gen) * (2.0 / l["ld"]) ** 0.5 for l in plan["layers"]]
    biases = [torch.randn(l["n_out"], generator=gen) * 0.1 for l in plan["layers"]]
    codes = {k: torch.randn(n, generator=gen) for k, n in (("exp", 30), ("shape", 50), ("tex", 256))}
    o = torch.rand(R, 3, generator=gen) * 6 - 3
    d = torch.randn(R, 3, generator=gen) * 0.6
    z = torch.sort(torch.rand(R, S, generator=gen) * 18 + 8, -1)[0].contiguous()
    if shared_z:
        z = z[R // 2:R // 2 + 1].expand(R, S).contiguous()
    vd = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    return dict(D=D, W=W, nf=nf, R=R, S=S, plan=plan, names=names, weights=weights, biases=biases, codes=codes, o=o, d=d, z=z, vd=vd,
                pts=br.points_from_rays(o, d, z).contiguous(), seed=seed)


def one_hot_d_raw(M, hot_row, pattern, seed=0, device="cpu"):
    """d_raw [M, 4]: zero except at hot_row, where the pattern's channels hold asymmetric random values of order 1"""
    gen = torch.Generator().manual_seed(1000 + 7 * hot_row + seed)
    v = torch.randn(4, generator=gen) + 0.25
    v = v * {"all four": torch.tensor([1.0, 1, 1, 1]), "only sigma": torch.tensor([0.0, 0, 0, 1]), "only rgb": torch.tensor([1.0, 1, 1, 0])}[pattern]
    out = torch.zeros(M, 4)
    out[hot_row] = v
    return out.to(device)


# ---- an honest fp32 evaluation of mofa_net_forward (fp32 tape) + mofa_net_backward, in torch -----------------------------------------------
def emulate(case, d_raw, form="points", fitting=False):
    """The oracle network under torch autograd in fp32, with a hook on every Linear's output that keeps the activation and its gradient
    (the masked output gradient G_l), laid out as mofa_net_backward lays its outputs out by fr.net_plan.  form: "points" (d_pts) or
    "rays" (d_rays_o / d_rays_d).  Returns (tape, outputs, G) — G[li] is the emulation's own [M, n_out] gradient of layer li."""
    plan, S, R = case["plan"], case["S"], case["R"]
    L, M = plan["layers"], case["R"] * case["S"]
    Mp = br.round_up(M, br.ROW_TILE)
    st = {}
    for name, w, b in zip(case["names"], case["weights"], case["biases"]):
        st[name + ".weight"], st[name + ".bias"] = w.clone().requires_grad_(True), b.clone()
    if form == "points":
        pts = case["pts"].clone().requires_grad_(True)
        leaves = [pts]
    else:
        o, d = case["o"].clone().requires_grad_(True), case["d"].clone().requires_grad_(True)
        pts = (o[:, None, :] + d[:, None, :] * case["z"][:, :, None]).reshape(-1, 3)
        leaves = [o, d]
    kept, lin = {}, orc._lin

    def hooked(st_, key, x):
        y = lin(st_, key, x)
        y.retain_grad()
        kept[key] = y
        return y

    orc._lin = hooked
    try:
        x93 = torch.cat([orc.positional_encode(pts, case["nf"]), case["codes"]["exp"].expand(M, -1)], -1)
        v27 = orc.positional_encode(case["vd"][:, None].expand(R, S, 3).reshape(-1, 3), 4)
        raw = orc.nerf_forward(st, x93, case["codes"]["shape"].expand(M, -1), v27, case["codes"]["tex"].expand(M, -1))
    finally:
        orc._lin = lin
    (raw * d_raw).sum().backward()
    tape = torch.zeros(Mp * plan["tape_cols"])
    d_folded = torch.zeros(plan["folded_floats"])
    view_rows = torch.zeros(R, plan["Hp"])
    d_weights, G = [], {}
    conditioned = conditioned_layers(plan)
    for li, (l, name) in enumerate(zip(L, case["names"])):
        y = kept[name]
        G[li] = y.grad
        n_out = l["n_out"]
        if not l["head"]:
            t0 = Mp * l["tape_cols"]
            tape[t0:t0 + Mp * l["n_padded"]] = br.pack_panels(torch.relu(y.detach()), Mp, k_padded=l["n_padded"])
        if li == plan["view"]:
            view_rows[:, :n_out] = y.grad.reshape(R, S, n_out).sum(1)
        elif l["head"] or not fitting or li in conditioned:
            d_folded[l["folded_off"]:l["folded_off"] + n_out] = y.grad.sum(0)
        dw = torch.full((n_out, l["ld"]), SENT)
        for c0, nc, _ in l["parts"]:
            dw[:, c0:c0 + nc] = st[name + ".weight"].grad[:, c0:c0 + nc]
        d_weights.append(dw)
    outputs = dict(d_folded=d_folded, d_view_bias_rows=view_rows, d_weights=None if fitting else d_weights)
    if form == "points":
        outputs["d_pts"] = leaves[0].grad
    else:
        outputs["d_rays_o"], outputs["d_rays_d"] = leaves[0].grad, leaves[1].grad
    return tape, outputs, G


# ---- the audit ----------------------------------------------------------------------------------------------------------------------------
def conditioned_layers(plan):
    """The five layers with per-call-constant code columns: the only MFMA layers whose d_folded slice the fitting form fills"""
    return {plan["xyz0"], plan["bim0"], plan["bim_skip"], plan["uv0"], plan["uv_skip"]}


def tape_row(tape, plan, li, m_padded, m):
    """Row m of layer li's tape slot: [n_padded]"""
    l = plan["layers"][li]
    k = torch.arange(l["n_padded"], device=tape.device)
    return tape[m_padded * l["tape_cols"] + br.panel_offset(m_padded, m, k)]


def relation_of(plan, i):
    """Which of the issue's relations produces the gradient at layer i's output"""
    if i == plan["view"]:
        return "rgb head -> view layer"
    if i == plan["view"] - 1:
        return "view layer -> last uv layer"
    if i == plan["sigma"]:
        return "d sigmaCodes (uv skip x + uv0 + alpha head, then mask)"
    if i == plan["xyz0"] + 3:
        return "d xyz_code (bim skip x + bim0, then mask)"
    if i in (plan["bim_skip"] - 1, plan["uv_skip"] - 1):
        return "skip layer h part"
    if i < plan["xyz0"] + 3:
        return "xyzEncode 3..1"
    return "plain layer"


class Report:
    def __init__(self, what):
        self.what, self.ratios, self.failures, self.G, self.live = what, {}, [], {}, {}

    def hold(self, relation, name, got, ref, cond, trig=None, extra=None):
        """every element of got within bound(cond, trig) (+ extra) of ref; keeps the worst err / sum |a b| per relation"""
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        lim = br.bound(cond, trig)
        if extra is not None:
            lim = lim + extra
        err = (got.double() - ref).abs()
        self.ratios[relation] = max(self.ratios.get(relation, 0.0), br.worst_ratio(got, ref, cond))
        bad = ~(err <= lim)
        if bad.any():
            self.failures.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements over the bound, worst err / bound = "
                                 f"{float((err / lim)[bad].nan_to_num(float('inf')).max()):.3e}")

    def exact(self, name, ok):
        if not bool(ok):
            self.failures.append(name)

    def finish(self, collect):
        assert collect or not self.failures, f"{self.what}: " + "; ".join(self.failures)
        return self


def audit_backward(plan, weights, tape, d_raw, hot_row, outputs, S, points=None, rays=None, sentinel=SENT, upstream=None, what="",
                   collect=False):
    """Audit one mofa_net_backward call (or its emulation) whose d_raw is zero off row hot_row.

    weights: the 2D + 7 source tensors [n_out, ld]; tape: the call's fp32 tape; outputs: plain tensors d_folded, d_view_bias_rows,
    d_pts (with points [M, 3]) or d_rays_o / d_rays_d (with rays = (o, d, z [R, S])), d_weights (a list, or None: the fitting form).
    upstream: the G of another call on the same inputs (the training form's report.G) — the fitting form fills only five layers'
    slices, so its relations are recomputed from those.  Returns a Report (ratios per relation, G per layer); raises unless collect."""
    L, M = plan["layers"], d_raw.shape[0]
    Mp, m, r = br.round_up(M, br.ROW_TILE), hot_row, hot_row // S
    rep = Report(f"{what} hot row {m}")
    fitting = outputs.get("d_weights") is None
    assert not fitting or upstream is not None, "the fitting form is audited against the training call's gradients"
    others = torch.ones(M, dtype=torch.bool, device=d_raw.device)
    others[m] = False
    assert (d_raw[others] == 0).all() and torch.isfinite(d_raw[m]).all(), "d_raw is not one-hot"
    dr = d_raw[m].double()
    df, vr = outputs["d_folded"], outputs["d_view_bias_rows"]
    mfma = [li for li, l in enumerate(L) if not l["head"]]
    conditioned = conditioned_layers(plan)
    X = {li: tape_row(tape, plan, li, Mp, m)[:L[li]["n_out"]] for li in mfma}
    # ---- reading the gradients ------------------------------------------------------------------------------------------------------------
    G, read = {plan["alpha"]: dr[3:4], plan["rgb"]: dr[0:3]}, set()
    for li in mfma:
        l = L[li]
        if li == plan["view"]:
            G[li] = vr[r, :l["n_out"]].double()
        elif fitting and li not in conditioned:
            G[li] = upstream[li]
            continue
        else:
            G[li] = df[l["folded_off"]:l["folded_off"] + l["n_out"]].double()
        read.add(li)
    rep.G = G
    src = G if upstream is None else upstream                 # the downstream values every relation is recomputed from
    colour_dead = bool((dr[0:3] == 0).all())                   # only channel 3: the uv stack's and the view layer's gradients are exactly zero
    # ---- per-layer relations: the gradient at producer i's output = mask_i (sum over its consumers of G_consumer W_consumer[:, part]) ----------
    consumers = {}
    for li, l in enumerate(L):
        for (c0, nc, _), i in zip(l["parts"], l["inputs"]):
            consumers.setdefault(i, []).append((li, c0, nc))

    def product(i):
        val = cond = 0.0
        for li, c0, nc in consumers[i]:
            w = weights[li][:, c0:c0 + nc].double()
            val, cond = val + src[li] @ w, cond + src[li].abs() @ w.abs()
        return val, cond

    for i in mfma:
        val, cond = product(i)
        ref = torch.where(X[i] > 0, val, torch.zeros_like(val))
        name = f"layer {i}: {relation_of(plan, i)}"
        dead = colour_dead and plan["uv0"] <= i <= plan["view"]
        if dead:
            assert (ref == 0).all()
        else:                                                  # the guard against a vacuous audit: a condition on the REFERENCE side
            rep.live[i] = int((ref != 0).sum())
            assert torch.isfinite(ref).all() and rep.live[i] >= L[i]["n_out"] / 8, \
                f"{rep.what}: {name} has {rep.live[i]} non-zero of {L[i]['n_out']} gradients at the hot row — a dead point audits nothing"
        if i not in read:
            continue
        if dead:
            rep.exact(f"{name}: not exactly zero although d_raw[:, 0:3] is", (G[i] == 0).all())
        rep.hold(relation_of(plan, i), name, G[i], ref, cond)
    # ---- geometry -------------------------------------------------------------------------------------------------------------------------
    nf, PE = plan["pe_point_freqs"], 3 + 6 * plan["pe_point_freqs"]
    w0 = weights[plan["xyz0"]][:, :PE].double()
    dpe = src[plan["xyz0"]] @ w0
    E = br.bound(src[plan["xyz0"]].abs() @ w0.abs())           # what the device's fp32 d(encoding) may be off by, feature by feature
    if points is not None:
        x, zm = points[m:m + 1], None
    else:
        o, d, z = rays
        x, zm = br.points_from_rays(o, d, z)[m:m + 1], z.reshape(-1)[m].double()
    gx, cond, trig = br.pe_point_backward(dpe[None], x, nf)
    _, _, e_trig = br.pe_point_backward(E[None], x, nf)
    carried = E[None, 0:3] + e_trig                            # E_id + sum_f 2^f (E_sin + E_cos): |cos|, |sin| <= 1
    if points is not None:
        rep.hold("d_pts", "d_pts[hot row]", outputs["d_pts"][m:m + 1], gx, cond, trig, carried)
        rep.exact("d_pts: a row other than the hot row is not zero", (outputs["d_pts"][others] == 0).all())
    else:
        R = o.shape[0]
        cold = torch.ones(R, dtype=torch.bool, device=d_raw.device)
        cold[r] = False
        rep.hold("d_rays_o", "d_rays_o[hot ray]", outputs["d_rays_o"][r:r + 1], gx, cond, trig, carried)
        az = zm.abs()                                          # one more rounding (the product with z): C * |gx z| is part of cond * |z|
        rep.hold("d_rays_d", "d_rays_d[hot ray]", outputs["d_rays_d"][r:r + 1], gx * zm, cond * az, trig * az, carried * az)
        rep.exact("d_rays_o: a ray other than the hot ray is not zero", (outputs["d_rays_o"][cold] == 0).all())
        rep.exact("d_rays_d: a ray other than the hot ray is not zero", (outputs["d_rays_d"][cold] == 0).all())
    # ---- weight gradients: one outer product each ---------------------------------------------------------------------------------------------
    if not fitting:
        feats = br.pe_features(x, nf)[0]
        for li, l in enumerate(L):
            dw = outputs["d_weights"][li]
            assert dw.shape == (l["n_out"], l["ld"])
            for (c0, nc, _), i in zip(l["parts"], l["inputs"]):
                xin = feats if i == "pe" else X[i][:nc].double()
                ref = G[li][:, None] * xin[None, :]
                trig_w = None
                if i == "pe":                                  # the device's sincosf: absolute error of a few 2^-24 per sine / cosine feature
                    trig_w = G[li].abs()[:, None].expand(-1, nc).clone()
                    trig_w[:, :3] = 0
                kind = "d_weights heads" if l["head"] else ("d_weights layer 0 (encoding)" if i == "pe" else "d_weights")
                rep.hold(kind, f"d_weights[{li}][:, {c0}:{c0 + nc}]", dw[:, c0:c0 + nc], ref, ref.abs(), trig_w)
            if l["fold"] and l["fold"][2]:
                _, c0, nc = l["fold"]
                rep.exact(f"d_weights[{li}]: a per-call-constant column [{c0}, {c0 + nc}) lost the sentinel", (dw[:, c0:c0 + nc] == sentinel).all())
    # ---- exact zeros and the head slices ----------------------------------------------------------------------------------------------------
    vcold = torch.ones(vr.shape[0], dtype=torch.bool, device=vr.device)
    vcold[r] = False
    rep.exact("d_view_bias_rows: a row other than the hot ray's is not zero", (vr[vcold] == 0).all())
    rep.exact("d_view_bias_rows: a padding column is not zero", (vr[:, L[plan["view"]]["n_out"]:] == 0).all())
    for li, l in enumerate(L):
        if li == plan["view"]:
            continue
        sl = df[l["folded_off"]:l["folded_off"] + l["n_padded"]]
        if l["head"]:                                          # k_raw_colsum_combine: rgb slice [sum d0, sum d1, sum d2, 0], alpha slice [sum d3, 0, 0, 0]
            want = torch.zeros(4, dtype=d_raw.dtype, device=d_raw.device)
            want[:l["n_out"]] = d_raw[m, 3:4] if li == plan["alpha"] else d_raw[m, 0:3]
            rep.exact(f"d_folded head slice of layer {li} is not d_raw[hot row] and zeros", (sl == want).all())
        elif fitting and li not in conditioned:
            rep.exact(f"d_folded[layer {li}] is not zero in the fitting form", (sl == 0).all())
        else:
            rep.exact(f"d_folded[layer {li}]: a padding entry is not zero", (sl[l["n_out"]:] == 0).all())
    return rep.finish(collect)

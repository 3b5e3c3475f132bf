"""The one-hot audit of tests/test_gpu_bwd_audit.py must be able to fail — and must pass an honest evaluation.  An fp32 emulation of
mofa_net_backward's outputs (the oracle network under torch autograd, a hook on every Linear's output; tests/bwd_audit.py) passes
audit_backward at every network, hot row, d_raw pattern and geometry form the GPU test uses, with bwd_reference's constants unchanged;
every fault the host function of csrc/mofa_net.hip could have — a wrong mask slot, a wrong accumulate / mask order, a dropped
contribution, exchanged weight blocks, a shifted d_folded slice, a recycled gradient buffer, ... — breaks it.  The guard against a
vacuous audit (at least n_out / 8 live gradients per layer at the hot row) is checked here for the inputs of the GPU test, which are made
on the CPU from the same seeds.  Runs on the CPU; prints the honest evaluation's worst err / sum |a b| per relation."""
import ctypes as C

import pytest
import torch

import bwd_audit as ba
import bwd_reference as br
import fwd_reference as fr

SMALL = ["8x64", "8x96", "10x128"]


def _honest(net, form, shared_z=False, fitting=False):
    """every hot row and pattern of one network: {relation: worst ratio}"""
    case = ba.make_case(*ba.NETS[net], shared_z=shared_z)
    plan, M, worst = case["plan"], case["R"] * case["S"], {}
    geo = dict(points=case["pts"]) if form == "points" else dict(rays=(case["o"], case["d"], case["z"]))
    for m in ba.HOT_ROWS:
        for pattern in ba.PATTERNS:
            d_raw = ba.one_hot_d_raw(M, m, pattern)
            tape, out, _ = ba.emulate(case, d_raw, form)
            rep = ba.audit_backward(plan, case["weights"], tape, d_raw, m, out, case["S"], what=f"honest fp32 {net} {form} {pattern}", **geo)
            reps = [rep]
            if fitting:
                _, fit, _ = ba.emulate(case, d_raw, form, fitting=True)
                reps.append(ba.audit_backward(plan, case["weights"], tape, d_raw, m, fit, case["S"], upstream=rep.G,
                                              what=f"honest fp32 fitting {net} {form} {pattern}", **geo))
            for rp in reps:
                for k, v in rp.ratios.items():
                    worst[k] = max(worst.get(k, 0.0), v)
            assert min(rep.live.values()) >= 1
    for k, v in sorted(worst.items()):
        print(f"honest fp32 {net} {form}: {k}: worst err / sum|ab| = {v:.3e}")
    return worst


@pytest.mark.parametrize("form", ["points", "rays"])
@pytest.mark.parametrize("net", SMALL)
def test_honest_fp32_emulation_passes_the_audit(net, form):
    """8x64, 8x96 (n_out != n_padded) and 10x128, explicit points and rays, the training and the fitting form, every hot row x pattern"""
    _honest(net, form, fitting=True)


def test_honest_fp32_emulation_passes_with_a_shared_z_row():
    _honest("8x96", "rays", shared_z=True)


@pytest.mark.parametrize("net", [n for n in ba.NETS if n not in SMALL])
def test_the_gpu_tests_wide_networks_are_alive_at_every_hot_row(net):
    """The guard (audit_backward asserts it): the inputs tests/test_gpu_bwd_audit.py runs at 8x256, 10x512 and 16 frequencies have at
    least n_out / 8 live gradients in every layer at every hot row, for every pattern"""
    _honest(net, "points")


# ---- the faults ---------------------------------------------------------------------------------------------------------------------------
class _Faulty:
    """One honest emulated call and what is needed to restate single steps of the host function wrongly, in fp32"""

    def __init__(self, net, m, form="points", pattern="all four"):
        self.case = case = ba.make_case(*ba.NETS[net])
        self.plan, self.m, self.S, self.form = case["plan"], m, case["S"], form
        self.M = case["R"] * case["S"]
        self.Mp = br.round_up(self.M, 256)
        self.d_raw = ba.one_hot_d_raw(self.M, m, pattern)
        self.tape, self.out, _ = ba.emulate(case, self.d_raw, form)
        self.geo = dict(points=case["pts"]) if form == "points" else dict(rays=(case["o"], case["d"], case["z"]))
        self.rep = self.audit(self.out)                                            # honest: passes
        self.G = {li: g.float() for li, g in self.rep.G.items()}

    def audit(self, out, collect=False, upstream=None):
        return ba.audit_backward(self.plan, self.case["weights"], self.tape, self.d_raw, self.m, out, self.S, collect=collect,
                                 upstream=upstream, **self.geo)

    def sl(self, li, padded=False):
        l = self.plan["layers"][li]
        return slice(l["folded_off"], l["folded_off"] + (l["n_padded"] if padded else l["n_out"]))

    def mask(self, li):
        return ba.tape_row(self.tape, self.plan, li, self.Mp, self.m)[:self.plan["layers"][li]["n_out"]] > 0

    def contrib(self, li, part=0, weights_of=None, cols=None):
        c0, nc, _ = self.plan["layers"][li]["parts"][part] if cols is None else cols
        return self.G[li] @ self.case["weights"][li if weights_of is None else weights_of][:, c0:c0 + nc]

    def with_G(self, li, g):
        out = dict(self.out, d_folded=self.out["d_folded"].clone())
        out["d_folded"][self.sl(li)] = g
        return out

    def breaks(self, name, out, must, upstream=None):
        try:
            failures = self.audit(out, collect=True, upstream=upstream).failures
        except AssertionError as e:                                                # the guard: a gradient read as all zero is a failure too
            failures = [str(e)]
        print(f"fault {name}: {failures}")
        assert failures, f"the audit did not see: {name}"
        assert any(must in f for f in failures), (name, must, failures)


@pytest.mark.parametrize("net,m", [("8x64", 0), ("8x96", 255), ("10x128", 256), ("8x96", 299)])
def test_the_audit_sees_every_fault_of_the_layer_chain(net, m):
    f = _Faulty(net, m)
    p, where = f.plan, torch.where
    zero = torch.zeros(p["W"])
    # a mask taken from the neighbouring tape slot
    i = p["xyz0"] + 1
    f.breaks("mask of the neighbouring tape slot", f.with_G(i, where(f.mask(i + 1), f.contrib(i + 1), zero)), f"layer {i}:")
    i = p["uv_skip"] - 1
    f.breaks("skip h part masked by the neighbouring slot", f.with_G(i, where(f.mask(i - 1), f.contrib(i + 1), zero)), f"layer {i}:")
    # the two stack inputs: accumulate first, then mask
    for i, skip, first, head in ((p["sigma"], p["uv_skip"], p["uv0"], p["alpha"]), (p["xyz0"] + 3, p["bim_skip"], p["bim0"], None)):
        a, b = f.contrib(skip, 1), f.contrib(first)
        c = f.contrib(head) if head is not None else zero
        mk, last = f.mask(i), (c if head is not None else b)
        f.breaks(f"layer {i}: mask before the accumulate", f.with_G(i, (a + b + c - last) + where(mk, last, zero)), f"layer {i}:")
        f.breaks(f"layer {i}: the final mask left out", f.with_G(i, a + b + c), f"layer {i}:")
        f.breaks(f"layer {i}: the skip x part masked", f.with_G(i, where(mk, where(f.mask(skip - 1), a, zero) + b + c, zero)), f"layer {i}:")
        if head is not None:
            f.breaks("the alpha head's contribution left out", f.with_G(i, where(mk, a + b, zero)), f"layer {i}:")
        # the skip layer's two column parts exchanged: h meets the x columns, x the h columns
        parts = p["layers"][skip]["parts"]
        out = f.with_G(skip - 1, where(f.mask(skip - 1), f.contrib(skip, cols=parts[1]), zero))
        f.breaks(f"skip layer {skip}: h part from the x columns", out, f"layer {skip - 1}:")
        out = f.with_G(i, where(mk, f.contrib(skip, cols=parts[0]) + b + c, zero))
        f.breaks(f"skip layer {skip}: x part from the h columns", out, f"layer {i}:")
    # a weight block of the neighbouring layer
    i = p["bim0"] + 2
    f.breaks("weight block of the neighbouring layer", f.with_G(i, where(f.mask(i), f.contrib(i + 1, weights_of=i + 2), zero)), f"layer {i}:")
    i = p["view"] - 1
    wrong = (0, p["W"], 0)                                                         # the view layer's block read from column 0, not 27
    f.breaks("view layer's block at column 0", f.with_G(i, where(f.mask(i), f.contrib(p["view"], cols=wrong), zero)), f"layer {i}:")
    # one layer's d_folded slice shifted by 64 floats
    li = p["bim0"] + 1
    out = f.with_G(li, 0.0)
    out["d_folded"][f.sl(li, True)] = f.out["d_folded"][f.sl(li, True).start + 64:f.sl(li, True).stop + 64]
    f.breaks("d_folded slice shifted by 64 floats", out, f"layer {li}")
    # a gradient buffer recycled one step early: layer l's G replaced by layer l + 2's
    for li in (p["xyz0"] + 1, p["bim_skip"] + 1, p["uv0"] + 2):
        f.breaks(f"layer {li}: the buffer holds layer {li + 2}'s gradient", f.with_G(li, f.G[li + 2]), f"layer {li}")
    # the head slices
    out = f.with_G(p["rgb"], f.G[p["rgb"]].flip(0))
    f.breaks("rgb head slice in another order", out, "head slice")
    out = dict(f.out, d_folded=f.out["d_folded"].clone())
    out["d_folded"][f.sl(p["alpha"], True).start + 1] = f.d_raw[m, 3]
    f.breaks("alpha head slice padded with the value", out, "head slice")
    out = dict(f.out, d_folded=f.out["d_folded"].clone())
    out["d_folded"][f.sl(p["uv0"], True).stop - 1] += 1e-20 if p["W"] % 64 else 0.0
    if p["W"] % 64:
        f.breaks("a padding entry of d_folded written", out, "padding entry")


@pytest.mark.parametrize("m", ba.HOT_ROWS)
def test_the_audit_sees_every_fault_of_the_view_rows(m):
    f = _Faulty("8x96", m, form="rays")
    p, R, S = f.plan, f.case["R"], f.S
    n_out = p["layers"][p["view"]]["n_out"]
    g = f.out["d_view_bias_rows"][m // S].clone()
    seen = 0
    for s_wrong in (S - 1, S + 1):                                                 # the per-ray sums taken over S -+ 1 samples
        rows = torch.zeros_like(f.out["d_view_bias_rows"])
        if m // s_wrong < R:
            rows[m // s_wrong] = g
        if m // s_wrong != m // S:
            f.breaks(f"view rows summed with S = {s_wrong}", dict(f.out, d_view_bias_rows=rows), "view")
            seen += 1
    assert seen >= (1 if m in (240, 299) else 0)                                   # row 240 sees S + 1, row 299 sees S - 1
    rows = f.out["d_view_bias_rows"].clone()
    rows[(m // S + 1) % R, 3] = 1e-20
    f.breaks("a value leaked into another ray's view row", dict(f.out, d_view_bias_rows=rows), "row other than")
    rows = f.out["d_view_bias_rows"].clone()
    rows[m // S, n_out] = 1e-20
    f.breaks("a padding column of the view rows written", dict(f.out, d_view_bias_rows=rows), "padding column")
    d_o = f.out["d_rays_o"].clone()
    d_o[(m // S + 1) % R, 1] = 1e-20
    f.breaks("a value leaked into another ray's d_rays_o", dict(f.out, d_rays_o=d_o), "d_rays_o: a ray other")
    f.breaks("d_rays_d without z", dict(f.out, d_rays_d=f.out["d_rays_o"].clone()), "d_rays_d[hot ray]")
    f.breaks("d_rays_o with z", dict(f.out, d_rays_o=f.out["d_rays_d"].clone()), "d_rays_o[hot ray]")
    z_next = f.case["z"].reshape(-1)[m - 1 if m else 1]
    f.breaks("d_rays_d with the neighbouring sample's z", dict(f.out, d_rays_d=f.out["d_rays_o"] * z_next), "d_rays_d[hot ray]")


@pytest.mark.parametrize("net,m", [("8x64", 256), ("8x96", 0), ("8x64 nf16", 299)])
def test_the_audit_sees_every_fault_of_the_geometry_and_the_weight_gradients(net, m):
    f = _Faulty(net, m)
    p = f.plan
    d_pts = f.out["d_pts"].clone()
    d_pts[m - 1 if m else 1] = d_pts[m]
    f.breaks("d_pts written to the neighbouring row too", dict(f.out, d_pts=d_pts), "d_pts: a row other")
    nf, PE = p["pe_point_freqs"], 3 + 6 * p["pe_point_freqs"]
    dpe = f.G[p["xyz0"]] @ f.case["weights"][p["xyz0"]][:, :PE]
    for name, bad in (("last frequency dropped", torch.cat([dpe[:-6], torch.zeros(6)])), ("sine and cosine exchanged", dpe[[0, 1, 2] + [
            3 + 6 * k + (j + 3) % 6 for k in range(nf) for j in range(6)]])):
        gx = br.pe_point_backward(bad[None], f.case["pts"][m:m + 1], nf)[0].float()
        d_pts = f.out["d_pts"].clone()
        d_pts[m] = gx[0]
        f.breaks(f"d_pts: {name}", dict(f.out, d_pts=d_pts), "d_pts[hot row]")

    def with_dw(li, dw):
        ws = list(f.out["d_weights"])
        ws[li] = dw
        return dict(f.out, d_weights=ws)

    dw = f.out["d_weights"][p["bim0"]].clone()
    dw[5, 3] = 0.0
    f.breaks("a constant column overwritten", with_dw(p["bim0"], dw), "lost the sentinel")
    for li in (p["uv0"], p["bim_skip"], p["xyz0"]):                                # a block written at col0 + 1
        c0, nc, _ = p["layers"][li]["parts"][-1]
        dw = f.out["d_weights"][li].clone()
        dw[:, c0 + 1:c0 + nc] = f.out["d_weights"][li][:, c0:c0 + nc - 1]
        f.breaks(f"d_weights[{li}] block at col0 + 1", with_dw(li, dw), f"d_weights[{li}]")
    sk = p["uv_skip"]                                                              # the skip layer's parts meet each other's input
    (h0, nc, _), (x0, _, _) = p["layers"][sk]["parts"]
    dw = f.out["d_weights"][sk].clone()
    dw[:, h0:h0 + nc], dw[:, x0:x0 + nc] = f.out["d_weights"][sk][:, x0:x0 + nc], f.out["d_weights"][sk][:, h0:h0 + nc]
    f.breaks("skip layer's weight-gradient parts exchanged", with_dw(sk, dw), f"d_weights[{sk}]")
    li = p["bim0"] + 2                                                             # the input of the neighbouring layer
    x = ba.tape_row(f.tape, p, li, f.Mp, m)[:p["W"]]
    f.breaks("weight gradient from the layer's own output", with_dw(li, f.G[li][:, None] * x[None, :]), f"d_weights[{li}]")
    x = ba.tape_row(f.tape, p, p["view"] - 1, f.Mp, m)[:p["W"]]                    # the alpha head reads sigmaCodes, not rgbCodes
    f.breaks("alpha head's weight gradient from the last uv layer", with_dw(p["alpha"], f.G[p["alpha"]][:, None] * x[None, :]),
             f"d_weights[{p['alpha']}]")
    f.breaks("rgb head's weight gradient in another order", with_dw(p["rgb"], f.out["d_weights"][p["rgb"]].flip(0)), f"d_weights[{p['rgb']}]")


def test_the_audit_sees_every_fault_of_the_fitting_form():
    f = _Faulty("8x96", 255)
    p = f.plan
    _, fit, _ = ba.emulate(f.case, f.d_raw, "points", fitting=True)
    f.audit(fit, upstream=f.rep.G)                                                 # honest: passes
    li = p["bim0"] + 1
    out = dict(fit, d_folded=fit["d_folded"].clone())
    out["d_folded"][f.sl(li).start + 7] = 1e-20
    f.breaks("fitting: a non-conditioned layer's slice is not zero", out, "not zero in the fitting form", upstream=f.rep.G)
    out = dict(fit, d_folded=fit["d_folded"].clone())
    out["d_folded"][f.sl(p["uv_skip"])] = f.out["d_folded"][f.sl(p["uv_skip"] + 1)]
    f.breaks("fitting: the deferred bias gradient read a recycled buffer", out, f"layer {p['uv_skip']}", upstream=f.rep.G)
    out = dict(fit, d_folded=fit["d_folded"].clone())
    out["d_folded"][f.sl(p["bim0"])] = 0.0
    f.breaks("fitting: a conditioned layer's bias gradient missing", out, f"layer {p['bim0']}", upstream=f.rep.G)
    with pytest.raises(AssertionError):
        f.audit(fit)                                                               # the fitting form cannot be audited from its own five slices


def test_a_dead_point_cannot_pass_silently():
    """the guard: a hot row whose gradients are all masked away must raise, whatever the outputs say"""
    f = _Faulty("8x64", 0)
    tape = torch.zeros_like(f.tape)
    with pytest.raises(AssertionError, match="dead point"):
        ba.audit_backward(f.plan, f.case["weights"], tape, f.d_raw, f.m, f.out, f.S, points=f.case["pts"])
    with pytest.raises(AssertionError, match="one-hot"):
        ba.audit_backward(f.plan, f.case["weights"], f.tape, f.d_raw + 1e-3, f.m, f.out, f.S, points=f.case["pts"])


# ---- the backward workspace against what the weight gradients' partial sums need -------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 64, 16), (8, 64, 11), (6, 32, 16), (8, 64, 10), (8, 96, 16), (10, 128, 16), (8, 256, 16), (10, 512, 10)])
@pytest.mark.parametrize("n", [1, 300, 5000])
def test_backward_workspace_holds_every_weight_gradients_partial_sums(shape, n):
    """mofa_net_backward lays its workspace out as four gradient buffers, the encoding gradient, 64 floats, then the weight gradients'
    scratch: the query must leave room there for the LARGEST product's partial sums — layer 0 contracts pe_k columns, which is wider than
    Wp for a network of width <= 64 behind more than ten frequencies (found by the GPU audit at 8x64, 16 frequencies: the partials ran
    7,360 floats past the end of the workspace)."""
    from mofanerf_amd import lib
    D, W, nf = shape
    L, s, p = lib.load(), lib.NetShape(D, W, nf, 4, 30, 50, 256), fr.net_plan(D, W, nf)
    Mp = br.round_up(n, 256)
    scratch_at = Mp * (4 * p["Wp"] + p["pe_k"]) + 64
    need = max(L.mofa_weight_grad_workspace_floats(n, l["n_padded"], kp) for l in p["layers"] if not l["head"] for _, _, kp in l["parts"])
    assert need >= br.wg_plan(n, p["Wp"], p["pe_k"])["total"] * p["Wp"] * (p["pe_k"] + 1)
    assert L.mofa_net_backward_workspace_floats(s, n, 1) >= scratch_at + need + 64


# ---- net_plan's d_folded slices against the library's host functions ----------------------------------------------------------------------
@pytest.mark.parametrize("net", list(ba.NETS))
def test_net_plan_places_every_d_folded_slice_where_the_library_does(net):
    from mofanerf_amd import lib
    D, W, nf, _ = ba.NETS[net]
    L, s, p = lib.load(), lib.NetShape(D, W, nf, 4, 30, 50, 256), ba.make_case(*ba.NETS[net])["plan"]
    off, no, ni = 0, C.c_int32(), C.c_int32()
    for li, l in enumerate(p["layers"]):
        assert L.mofa_net_layer_dims(s, li, C.byref(no), C.byref(ni)) == 0
        assert (no.value, ni.value) == (l["n_out"], l["ld"]) and l["folded_off"] == off, li
        off += 0 if li == p["view"] else (4 if li > p["view"] else br.round_up(no.value, 64))
    assert off == L.mofa_net_folded_floats(s) == p["folded_floats"]

"""mofa_net_backward as a whole, layer by layer, against fp64 — with one-hot gradients (tests/bwd_audit.py).

The host function of csrc/mofa_net.hip strings about sixty launches together: which transposed weight block meets which gradient buffer,
which tape slot masks it, where the contributions to d sigmaCodes and d xyz_code accumulate, which buffer may be recycled, where every
layer's slice of d_folded lies.  With d_raw zero except at ONE point m*, every sum the call returns has one non-zero term, so d_folded
holds the device's own G_l[m*, :] of every layer, and every layer is recomputed in fp64 from what the device reported one layer
downstream and held to the rounding-level bound of bwd_reference (constants unchanged), element by element; every weight gradient is
one outer product.  Direct C-ABI calls: outputs between guard regions, pre-filled with NaN (d_weights: with a sentinel the per-call
constant columns must keep), the workspace full of NaN before every call, every call twice with the same bytes.  M = 300 points (two row
tiles, the second ragged), hot rows 0 / 240 / 255 / 256 / 299, three d_raw patterns; explicit points and rays (once with a shared z row);
8x64, 8x96 and 10x128 per layer, 8x256 and 10x512 per layer and chained (fitting: the default; training: MOFA_CHAIN_TRAIN=1).
The fitting form (mask tape, no weight gradients) must be zero outside the five conditioned layers and the heads, is held to the same
bounds with the training call's gradients upstream, and must compare EQUAL to the training form.  tests/test_bwd_audit_cpu.py shows on
the CPU that an honest fp32 evaluation passes and that every fault of the host function breaks the audit; the inputs are made on the
CPU from the same seeds, so its guard against dead points covers these runs.  Each test prints its worst err / sum |a b| per relation."""
import functools

import pytest
import torch

import bwd_audit as ba
import bwd_reference as br
import fwd_reference as fr
from mofanerf_amd import lib
from test_gpu_bwd_kernels import Guarded, _same_bits, _twice

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
KNOBS = ("MOFA_PIPE", "MOFA_CHAIN", "MOFA_FUSED", "MOFA_CHAIN_TRAIN")
LAUNCH = {"per-layer": {"MOFA_CHAIN": "0"}, "chained": {"MOFA_CHAIN_TRAIN": "1"}}


@pytest.fixture(autouse=True)
def _shipped_launch_forms(monkeypatch):
    """Whatever MOFA_* knob the surrounding run exports, these tests start from the shipped forms and set what they vary themselves."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    lib.reload_env()
    yield
    monkeypatch.undo()
    lib.reload_env()


def L():
    return lib.load()


class Net:
    """One network on the device, one forward per geometry form: the fp32 tape, and — from a second call — the mask tape."""

    def __init__(self, name, shared_z=False):
        from mofanerf_amd.hipnet import HipNet
        from mofanerf_amd.model import NeRF
        D, W, nf, seed = ba.NETS[name]
        self.name, self.case = name, ba.make_case(D, W, nf, seed, shared_z=shared_z)
        c = self.case
        self.plan, self.R, self.S, self.M = c["plan"], c["R"], c["S"], c["R"] * c["S"]
        self.Mp = br.round_up(self.M, 256)
        net = NeRF(D=D, W=W, input_ch=3 + 6 * nf + 30, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True).to(DEV)
        with torch.no_grad():
            for lin, w, b in zip(net.ordered_linears(), c["weights"], c["biases"]):
                lin.weight.copy_(w)
                lin.bias.copy_(b)
        self.h = HipNet(net, point_freqs=nf)                                       # (initialises the device: census + self-check)
        self.ws, self.bs = self.h._weights()
        self.o, self.d, self.z, self.vd, self.pts = (c[k].to(DEV).contiguous() for k in ("o", "d", "z", "vd", "pts"))
        self.z_arg = (self.z[:1].contiguous(), 0) if shared_z else (self.z, self.S)
        self.codes = {k: v.to(DEV) for k, v in c["codes"].items()}
        self.folded = self.h.fold(self.codes["exp"], self.codes["shape"], self.codes["tex"]).clone()
        view = self.plan["layers"][self.plan["view"]]
        self.view_rows = torch.full((self.R, self.plan["Hp"]), NAN, device=DEV)
        lib.check(L().mofa_view_bias(lib.ptr(self.vd), self.R, 4, lib.ptr(self.ws[self.plan["view"]]), view["n_out"], view["ld"],
                                     lib.ptr(self.bs[self.plan["view"]]), lib.ptr(self.view_rows), self.plan["Hp"], lib.stream()), "view_bias")
        self.packed, self.packed_t = self.h.packed(), self.h.packed_t()
        self.verdict = torch.zeros(lib.VERDICT_WORDS, dtype=torch.int32, device=DEV)
        self.tapes = {}

    def geometry(self, form):
        """(rays_o, rays_d, z, z_row_stride, pts) of the C ABI"""
        if form == "points":
            return None, None, None, 0, lib.ptr(self.pts)
        return lib.ptr(self.o), lib.ptr(self.d), lib.ptr(self.z_arg[0]), self.z_arg[1], None

    def forward(self, form):
        """the fp32 tape and the mask tape of this geometry form (kept: one forward per net and form)"""
        if form not in self.tapes:
            Lb, sh = L(), self.h.shape
            n_tape, n_mask = Lb.mofa_net_tape_floats(sh, self.M), Lb.mofa_net_mask_tape_words(sh, self.M)
            assert n_tape == self.Mp * self.plan["tape_cols"] and n_mask * 64 == n_tape
            res = []
            for kind in ("tape", "mask"):
                ws = torch.full((Lb.mofa_net_workspace_floats(sh, self.M, self.R),), NAN, device=DEV)
                raw = Guarded(self.M * 4)
                tape = Guarded(n_tape) if kind == "tape" else None
                mask = Guarded(n_mask, dtype=torch.int64, fill=0x33) if kind == "mask" else None
                lib.check(Lb.mofa_net_forward(sh, lib.ptr(self.packed), lib.ptr(self.folded), None, None, *self.geometry(form), None, self.R, self.S,
                                              lib.ptr(ws), raw.ptr(), tape.ptr() if tape else None, mask.ptr() if mask else None,
                                              lib.ptr(self.view_rows), self.verdict.data_ptr(), lib.stream()), "net_forward")
                torch.cuda.synchronize()
                res.append((raw.check().clone(), (tape or mask).check().clone()))
            (raw_t, tape), (raw_m, words) = res
            assert _same_bits(raw_t, raw_m) and torch.isfinite(raw_t).all()
            # the mask tape's bits are (tape > 0) at the offsets of br.mask_bit_position — the valid rows of every slot
            o = torch.arange(n_tape, device=DEV)
            word, bit = br.mask_bit_position(o)
            flags = ((words[word] >> bit) & 1).float()
            for li, l in enumerate(self.plan["layers"]):
                if not l["head"]:
                    t0 = self.Mp * l["tape_cols"]
                    got = br.unpack_panels(flags[t0:t0 + self.Mp * l["n_padded"]], self.Mp, l["n_padded"])[:self.M]
                    assert torch.equal(got > 0, fr.tape_slot(tape, self.plan, li, self.Mp)[:self.M] > 0), f"mask tape of layer {li}"
            assert self.verdict.tolist()[0] == 0
            self.tapes[form] = (tape, words)
        return self.tapes[form]

    def backward(self, form, d_raw, training):
        """one mofa_net_backward call, twice; -> outputs as plain tensors"""
        Lb, sh, p = L(), self.h.shape, self.plan
        tape, words = self.forward(form)
        n_ws = Lb.mofa_net_backward_workspace_floats(sh, self.M, int(training))

        def run():
            ws = torch.full((n_ws,), NAN, device=DEV)
            outs = dict(d_folded=Guarded(p["folded_floats"]), d_view_bias_rows=Guarded(self.R * p["Hp"]))
            if form == "points":
                outs["d_pts"] = Guarded(self.M * 3)
            else:
                outs["d_rays_o"], outs["d_rays_d"] = Guarded(self.R * 3), Guarded(self.R * 3)
            dws = [Guarded(l["n_out"] * l["ld"], fill=ba.SENT) for l in p["layers"]] if training else None
            ptrs = lib.ptr_array([g.out for g in dws]) if training else None
            g = lambda k: outs[k].ptr() if k in outs else None
            lib.check(Lb.mofa_net_backward(sh, lib.ptr(self.packed), lib.ptr(self.packed_t), lib.ptr(tape) if training else None,
                                           None if training else words.data_ptr(), lib.ptr(d_raw), *self.geometry(form), self.R, self.S,
                                           lib.ptr(ws), g("d_folded"), g("d_view_bias_rows"), g("d_rays_o"), g("d_rays_d"), g("d_pts"), ptrs,
                                           self.verdict.data_ptr(), lib.stream()), "net_backward")
            torch.cuda.synchronize()
            return tuple(v.check() for v in outs.values()) + tuple(w.check() for w in (dws or []))

        flat = _twice(run)
        keys = ["d_folded", "d_view_bias_rows"] + (["d_pts"] if form == "points" else ["d_rays_o", "d_rays_d"])
        out = dict(zip(keys, flat))
        out["d_view_bias_rows"] = out["d_view_bias_rows"].reshape(self.R, p["Hp"])
        for k in keys[2:]:
            out[k] = out[k].reshape(-1, 3)
        out["d_weights"] = [w.reshape(l["n_out"], l["ld"]) for w, l in zip(flat[len(keys):], p["layers"])] if training else None
        return out

    def geo(self, form):
        return dict(points=self.pts) if form == "points" else dict(rays=(self.o, self.d, self.z))


@functools.lru_cache(maxsize=2)
def _net(name, shared_z=False):
    return Net(name, shared_z)


def _chained_launches(net):
    v = net.verdict.tolist()
    assert v[0] == 0, v
    return v[1]


def _audit(name, form, launch, knob, shared_z=False):
    net = _net(name, shared_z)
    net.forward(form)                                                              # (under the shipped knobs: the forward is not what varies here)
    for k, v in LAUNCH[launch].items():
        knob(k, v)
    chained = launch == "chained"
    worst, equal = {}, True
    for m in ba.HOT_ROWS:
        for pattern in ba.PATTERNS:
            what = f"{name} {form}{' shared z' if shared_z else ''} {launch} [{pattern}]"
            d_raw = ba.one_hot_d_raw(net.M, m, pattern, device=DEV)
            before = _chained_launches(net)
            train = net.backward(form, d_raw, True)
            mid = _chained_launches(net)
            fit = net.backward(form, d_raw, False)
            after = _chained_launches(net)
            # two chained launches per call, each call twice: the chained form really ran (only) where it should
            assert (mid - before, after - mid) == ((4, 4) if chained else (0, 0)), (what, before, mid, after)
            rep = ba.audit_backward(net.plan, net.ws, net.forward(form)[0], d_raw, m, train, net.S, what="training " + what, **net.geo(form))
            rfit = ba.audit_backward(net.plan, net.ws, net.forward(form)[0], d_raw, m, fit, net.S, upstream=rep.G, what="fitting " + what, **net.geo(form))
            for tag, rp in (("", rep), ("fitting: ", rfit)):
                for k, v in rp.ratios.items():
                    worst[tag + k] = max(worst.get(tag + k, 0.0), v)
            # fitting == training (==: +-0 are equal) on everything the fitting form fills: one non-zero term per sum, so the orders cannot matter
            cond = ba.conditioned_layers(net.plan)
            for li, l in enumerate(net.plan["layers"]):
                if li != net.plan["view"] and (l["head"] or li in cond):
                    sl = slice(l["folded_off"], l["folded_off"] + l["n_padded"])
                    same = bool((fit["d_folded"][sl] == train["d_folded"][sl]).all())
                    equal &= same
                    assert same, f"{what} hot row {m}: d_folded of layer {li} differs between the fitting and the training form"
            for k in fit:
                if k not in ("d_folded", "d_weights"):
                    same = bool((fit[k] == train[k]).all())
                    equal &= same
                    assert same, f"{what} hot row {m}: {k} differs between the fitting and the training form"
            if form == "rays":                                                     # the same points, o + d z rounded separately: the point form's row
                net.forward("points")
                pt = net.backward("points", d_raw, True)
                assert _same_bits(net.tapes["points"][0], net.tapes["rays"][0])
                assert (train["d_rays_o"][m // net.S] == pt["d_pts"][m]).all(), f"{what} hot row {m}: d_rays_o[r*] != d_pts[m*] of the point form"
                assert (train["d_folded"] == pt["d_folded"]).all() and (train["d_view_bias_rows"] == pt["d_view_bias_rows"]).all()
    for k, v in sorted(worst.items()):
        print(f"audit {name} {form}{' shared z' if shared_z else ''} {launch}: {k}: worst err / sum|ab| = {v:.3e}")
    print(f"audit {name} {form} {launch}: fitting == training on every compared element: {equal}")


@pytest.mark.parametrize("form", ["points", "rays"])
@pytest.mark.parametrize("name", ["8x64", "8x96", "10x128", "8x64 nf16"])
def test_backward_audit_per_layer_launches(name, form, knob):
    """8x64, 8x96 (padding columns: n_out != n_padded), 10x128, and 8x64 at 16 frequencies (8 operand panels of the encoding)"""
    _audit(name, form, "per-layer", knob)


def test_backward_audit_rays_sharing_one_z_row(knob):
    _audit("8x96", "rays", "per-layer", knob, shared_z=True)


@pytest.mark.parametrize("launch", ["per-layer", "chained"])
@pytest.mark.parametrize("form", ["points", "rays"])
@pytest.mark.parametrize("name", ["8x256", "10x512"])
def test_backward_audit_wide_networks_per_layer_and_chained(name, form, launch, knob):
    """8x256 and 10x512 under MOFA_CHAIN=0 and chained: the fitting backward's two chained launches (the default) with their deferred
    bias gradients and kept buffers, the training backward's (MOFA_CHAIN_TRAIN=1) with the weight gradients as queue entries — verdict
    word [1] must advance by two per call where, and only where, the chain is asked for."""
    _audit(name, form, launch, knob)


def test_backward_audit_through_the_host_layer(knob):
    """NetFn + fold_torch + view_bias_torch in training mode at 8x96 with the same one-hot gradient: what torch autograd adds around the
    HIP backward — the constant weight columns, the biases, the three codes, the view layer's encoding columns."""
    from mofanerf_amd.autograd import NetFn, fold_torch, view_bias_torch
    knob("MOFA_CHAIN", "0")
    net = Net("8x96")
    p, h, S, m = net.plan, net.h, net.S, 256
    Lp = p["layers"]
    # the direct call's forward gets the biases the host layer's forward gets (torch's fold and view rows round differently from the
    # library's kernels; a ReLU input near zero carries that into the tape): the same inputs, so the same tape, bit for bit
    with torch.no_grad():
        net.folded = fold_torch(h, net.codes["exp"], net.codes["shape"], net.codes["tex"]).contiguous()
        net.view_rows = view_bias_torch(h, net.vd).contiguous()
    d_raw = ba.one_hot_d_raw(net.M, m, "all four", device=DEV)
    direct = net.backward("rays", d_raw, True)
    tape = net.forward("rays")[0]
    rep = ba.audit_backward(p, net.ws, tape, d_raw, m, direct, S, what="direct call", **net.geo("rays"))
    G = rep.G
    lins = h._linears
    for lin in lins:
        lin.weight.grad = lin.bias.grad = None
    codes = {k: v.clone().requires_grad_(True) for k, v in net.codes.items()}
    og, dg, vdg = net.o.clone().requires_grad_(True), net.d.clone().requires_grad_(True), net.vd.clone().requires_grad_(True)
    raw = NetFn.apply(h, og, dg, net.z, S, S, fold_torch(h, codes["exp"], codes["shape"], codes["tex"]), view_bias_torch(h, vdg), None,
                      *[l.weight for l in lins])
    (raw.reshape(-1, 4) * d_raw).sum().backward()
    torch.cuda.synchronize()
    h.check_verdict(block=True)
    assert (og.grad == direct["d_rays_o"]).all() and (dg.grad == direct["d_rays_d"]).all()
    X = {li: ba.tape_row(tape, p, li, net.Mp, m)[:l["n_out"]].double() for li, l in enumerate(Lp) if not l["head"]}
    feats = {"pe": br.pe_features(net.pts[m:m + 1], p["pe_point_freqs"])[0], "view": br.pe_features(net.vd[m // S:m // S + 1], 4)[0]}
    code_ref = {k: [0.0, 0.0] for k in codes}
    worst = {}

    def hold(kind, name, got, ref, cond, trig=None):
        worst[kind] = max(worst.get(kind, 0.0), br.assert_close(got, ref, cond, name, trig=trig))

    for li, (l, lin) in enumerate(zip(Lp, lins)):
        g = G[li]
        assert (lin.bias.grad.double() == g).all(), f"bias.grad of layer {li} is not the G the direct call reported"
        ref, trig = torch.zeros(l["n_out"], l["ld"], dtype=torch.float64, device=DEV), None
        for (c0, nc, _), i in zip(l["parts"], l["inputs"]):
            ref[:, c0:c0 + nc] = g[:, None] * (feats["pe"] if i == "pe" else X[i][:nc])[None, :]
        if l["fold"] and l["fold"][2]:
            kind, c0, nc = l["fold"]
            const = feats["view"] if kind == "view" else net.codes[kind].double()
            ref[:, c0:c0 + nc] = g[:, None] * const[None, :]
            if kind != "view":
                w = net.ws[li][:, c0:c0 + nc].double()
                code_ref[kind][0] = code_ref[kind][0] + g @ w
                code_ref[kind][1] = code_ref[kind][1] + g.abs() @ w.abs()
        if li in (p["xyz0"], p["view"]):                                           # sine / cosine features: a few 2^-24 each, whatever their size
            trig = torch.zeros_like(ref)
            c0, nc = (0, 3 + 6 * p["pe_point_freqs"]) if li == p["xyz0"] else (0, 27)
            trig[:, c0 + 3:c0 + nc] = g.abs()[:, None]
        hold("weight.grad", f"host layer: weight.grad of layer {li}", lin.weight.grad, ref, ref.abs(), trig)
    for k, (ref, cond) in code_ref.items():                                        # exp: layer 0; shape, tex: the stack's first and skip layers
        hold("code gradients", f"host layer: d {k} code", codes[k].grad, ref, cond)
    for k, v in sorted(worst.items()):
        print(f"audit host layer 8x96: {k}: worst err / sum|ab| = {v:.3e}")
    for lin in lins:
        lin.weight.grad = lin.bias.grad = None

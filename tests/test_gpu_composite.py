"""Compositing and its backward through the C ABI (``mofa_composite_forward``, ``mofa_composite_sigma``, ``mofa_composite_backward``:
k_composite<1|2|4>, k_composite_long, k_composite_sigma*, k_composite_backward<1|2|4>, k_composite_backward_long) against the fp64
restatement of tests/comp_reference.py, element by element:  |got - ref| <= C * E + TINY  on EVERY element of every output, E being the
restatement's first-order bound for an fp32 evaluation, NaN exactly where the reference is NaN.

Explicit rays, no network, no camera.  One batch per sample count on both sides of every lane width and of the 256-sample pass
(comp_reference.make_batch): thin, moderate, empty and all-zero rays, hard surfaces of one to three opaque samples on each side of every
lane and pass boundary, nearly opaque samples, a ray whose only density is the last sample's, eight opaque samples in a row; an odd ray
count; white background off and on, noise absent and present, a shared z row (stride 0) and per-ray rows.  Every output lies between two
guard regions and is pre-filled with a sentinel, every call runs twice and must repeat bit for bit.  tests/test_comp_reference_cpu.py
shows on the CPU that the reference's own fp32 arithmetic passes this comparison and that eleven faults each miss it a hundredfold.
Each test prints its worst |err| / (E + TINY) per output (recorded in DESIGN.md, "Compositing, element by element")."""
import numpy as np
import pytest
import torch

import comp_reference as cr
from mofanerf_amd import lib
from test_comp_reference_cpu import oracle_autograd, split

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.25e11          # guard regions and never-written outputs
CASES = [(S, noise, shared) for S in cr.SAMPLE_COUNTS for noise in (False, True) for shared in (False, True)]
OPTIONAL = ("g_disp", "g_acc", "g_depth", "g_weights")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Outs:
    """Named fp32 outputs, each between two guard regions of at least four rays' worth of its elements, everything filled with SENT."""

    def __init__(self, S, **shapes):
        self.g = 16 * S + 64                                          # four rays of d_raw; a multiple of 4 floats (16-byte stores)
        self.shapes = shapes
        self.buf = {k: torch.full((int(np.prod(sh)) + 2 * self.g,), SENT, dtype=torch.float32, device=DEV) for k, sh in shapes.items()}

    def ptr(self, k):
        return self.buf[k][self.g:].data_ptr() if k in self.buf else None

    def done(self, written=None):
        """the outputs (guards checked, no element left unwritten), as device tensors"""
        torch.cuda.synchronize()
        out = {}
        guard = torch.full((self.g,), SENT, dtype=torch.float32, device=DEV)
        for k, sh in self.shapes.items():
            n = int(np.prod(sh))
            assert _same_bits(self.buf[k][:self.g], guard) and _same_bits(self.buf[k][self.g + n:], guard), f"{k}: a guard region was written"
            out[k] = self.buf[k][self.g:self.g + n].reshape(sh).clone()
            assert not (out[k] == SENT).any(), f"{k}: an element was never written"
        return out


def _device(b):
    d = {k: torch.from_numpy(v).to(DEV).contiguous() for k, v in b.items() if isinstance(v, np.ndarray) and v.dtype == np.float32}
    d["noise"] = d.get("noise") if b["noise"] is not None else None
    d["z_stride"] = 0 if b["z"].ndim == 1 else b["S"]
    d["sigma"] = d["raw"][..., 3].contiguous()
    return d


def _forward(b, d, white):
    o = Outs(b["S"], rgb=(b["R"], 3), disp=(b["R"],), acc=(b["R"],), depth=(b["R"],), weights=(b["R"], b["S"]))
    lib.check(lib.load().mofa_composite_forward(lib.ptr(d["raw"]), lib.ptr(d["z"]), d["z_stride"], lib.ptr(d["rays_d"]), lib.ptr(d["noise"]),
                                                b["R"], b["S"], int(white), o.ptr("rgb"), o.ptr("disp"), o.ptr("acc"), o.ptr("depth"),
                                                o.ptr("weights"), lib.stream()), "mofa_composite_forward")
    return o.done()


def _sigma(b, d):
    o = Outs(b["S"], disp=(b["R"],), acc=(b["R"],), depth=(b["R"],), weights=(b["R"], b["S"]))
    lib.check(lib.load().mofa_composite_sigma(lib.ptr(d["sigma"]), lib.ptr(d["z"]), d["z_stride"], lib.ptr(d["rays_d"]), lib.ptr(d["noise"]),
                                              b["R"], b["S"], o.ptr("disp"), o.ptr("acc"), o.ptr("depth"), o.ptr("weights"), lib.stream()),
              "mofa_composite_sigma")
    return o.done()


def _backward(b, d, white, g, with_rays_d=True):
    """g: the upstream gradients on the device, None for a NULL pointer"""
    shapes = {"d_raw": (b["R"], b["S"], 4)}
    if with_rays_d:
        shapes["d_rays_d"] = (b["R"], 3)
    o = Outs(b["S"], **shapes)
    lib.check(lib.load().mofa_composite_backward(lib.ptr(d["raw"]), lib.ptr(d["z"]), d["z_stride"], lib.ptr(d["rays_d"]), lib.ptr(d["noise"]),
                                                 b["R"], b["S"], int(white), lib.ptr(g["g_rgb"]), lib.ptr(g["g_disp"]), lib.ptr(g["g_acc"]),
                                                 lib.ptr(g["g_depth"]), lib.ptr(g["g_weights"]), o.ptr("d_raw"), o.ptr("d_rays_d"),
                                                 lib.stream()), "mofa_composite_backward")
    return o.done()


def _twice(run):
    a, b = run(), run()
    for k in a:
        assert _same_bits(a[k], b[k]), f"{k}: two runs differ"
    return a


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _report(what, worst):
    print(f"{what}: worst |err| / (E + TINY): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _behind_run_is_nothing(b, *arrays):
    """behind eight opaque samples (transmittance 1e-80): finite, and nothing"""
    m = b["behind_run"]
    for a in arrays:
        v = a[m]
        assert np.isfinite(v).all() and (np.abs(v) < 1e-30).all(), "something behind the long opaque run"


@pytest.mark.parametrize("S,noise,shared", CASES)
def test_composite_forward_every_element(S, noise, shared):
    """weights, rgb, acc, depth inside their bounds, disp NaN exactly on the rays without opacity and inside the quotient's bound on the
    others; mofa_composite_sigma on channel 3 gives mofa_composite_forward's bits."""
    b = cr.make_batch(S, noise, shared)
    d = _device(b)
    worst = {}
    for white in (False, True):
        got = _twice(lambda: _forward(b, d, white))
        F = cr.Forward(b["raw"], b["z"], b["rays_d"], b["noise"], white)
        dead = np.array([f in ("empty", "zero") for f in b["family"]])
        assert (np.isnan(F.disp) == dead).all() and dead.sum() == 3
        for name, ref, E in (("weights", F.w, F.EW), ("rgb", F.rgb, F.Ergb), ("acc", F.acc, F.Eacc), ("depth", F.depth, F.Edepth),
                             ("disp", F.disp, F.Edisp)):
            r = cr.assert_inside(_np(got[name]), ref, E, f"S={S} noise={noise} shared={shared} white={white} {name}")
            worst[name] = max(worst.get(name, 0.0), r)
        _behind_run_is_nothing(b, _np(got["weights"]))
        if not white:
            twin = _twice(lambda: _sigma(b, d))
            for k in ("disp", "acc", "depth", "weights"):
                assert _same_bits(twin[k], got[k]), f"mofa_composite_sigma: {k} is not mofa_composite_forward's"
    _report(f"forward S={S} noise={noise} shared_z={shared}", worst)


@pytest.mark.parametrize("S,noise,shared", CASES)
def test_composite_backward_every_element(S, noise, shared):
    """d_raw and d_rays_d inside their bounds with all five upstream gradients, and with each optional one NULL (NULL is zeros, bit for
    bit); d_rays_d = NULL leaves d_raw's bits alone.  A ray without opacity: with g_disp != 0 the NaN pattern is the one the fp32 oracle's
    autograd gives on the CPU (d_rays_d NaN, d_raw finite: every sigma there is gated off); with g_disp == 0 the kernel returns the finite
    0 that test_composite_backward_vs_autograd documents."""
    b = cr.make_batch(S, noise, shared)
    d = _device(b)
    full = {k: d[k] for k in ("g_rgb",) + OPTIONAL}
    dead = np.array([f in ("empty", "zero") for f in b["family"]])
    worst = {}

    def check(got, g, white, what):
        F = cr.Forward(b["raw"], b["z"], b["rays_d"], b["noise"], white)
        d_raw, E_raw, d_rd, E_rd = cr.backward(F, *[None if g[k] is None else _np(g[k]) for k in ("g_rgb",) + OPTIONAL])
        what = f"S={S} noise={noise} shared={shared} white={white} {what}"
        raw_got = _np(got["d_raw"])
        for name, a, ref, E in (("d_raw rgb", raw_got[..., :3], d_raw[..., :3], E_raw[..., :3]),
                                ("d_raw sigma", raw_got[..., 3], d_raw[..., 3], E_raw[..., 3]), ("d_rays_d", _np(got["d_rays_d"]), d_rd, E_rd)):
            worst[name] = max(worst.get(name, 0.0), cr.assert_inside(a, ref, E, f"{what} {name}"))
        _behind_run_is_nothing(b, raw_got[..., 0], raw_got[..., 1], raw_got[..., 2], raw_got[..., 3])
        return d_raw, d_rd

    for white in (False, True):
        # all five, g_disp != 0 on every ray: the rays without opacity are NaN where the fp32 oracle's autograd is
        got = _twice(lambda: _backward(b, d, white, full))
        ref_raw, ref_rd = check(got, full, white, "all five")
        o32 = split(oracle_autograd(b, white, torch.float32))
        assert np.isnan(o32["d_rays_d"][dead]).all() and not np.isnan(o32["d_rays_d"][~dead]).any() and not np.isnan(o32["d_raw sigma"]).any()
        assert (np.isnan(_np(got["d_rays_d"])) == np.isnan(o32["d_rays_d"])).all(), "d_rays_d: NaN pattern is not the fp32 oracle's"
        assert (np.isnan(_np(got["d_raw"])) == np.isnan(np.concatenate([o32["d_raw rgb"], o32["d_raw sigma"][..., None]], -1))).all()
        assert (np.isnan(ref_rd) == np.isnan(o32["d_rays_d"])).all() and not np.isnan(ref_raw).any()
        # d_rays_d = NULL: the same d_raw
        alone = _twice(lambda: _backward(b, d, white, full, with_rays_d=False))
        assert _same_bits(alone["d_raw"], got["d_raw"]), "d_rays_d = NULL changed d_raw"
        # g_disp == 0 on the rays without opacity: finite everywhere
        g0 = dict(full, g_disp=torch.where(torch.from_numpy(dead).to(DEV), torch.zeros_like(full["g_disp"]), full["g_disp"]).contiguous())
        fin = _twice(lambda: _backward(b, d, white, g0))
        assert torch.isfinite(fin["d_raw"]).all() and torch.isfinite(fin["d_rays_d"]).all()
        assert (fin["d_rays_d"][torch.from_numpy(dead).to(DEV)] == 0).all()
        check(fin, g0, white, "g_disp = 0 without opacity")
        # each optional gradient NULL in turn == zeros in its place, bit for bit, and inside the bound
        for k in OPTIONAL:
            gn, gz = dict(full, **{k: None}), dict(full, **{k: torch.zeros_like(full[k])})
            a, z = _twice(lambda: _backward(b, d, white, gn)), _backward(b, d, white, gz)
            assert _same_bits(a["d_raw"], z["d_raw"]) and _same_bits(a["d_rays_d"], z["d_rays_d"]), f"{k} = NULL is not {k} = 0"
            check(a, gn, white, f"{k} = NULL")
    _report(f"backward S={S} noise={noise} shared_z={shared}", worst)

"""The comparator of tests/test_gpu_composite.py must be right, must let an honest fp32 evaluation through, and must be able to fail.
On the inputs of the GPU test (comp_reference.make_batch, every sample count, noise / white background / shared z on and off):
the fp64 restatement (tests/comp_reference.py) agrees with fp64 autograd through the oracle's raw2outputs — two independent
derivations; the oracle's own fp32 arithmetic with torch autograd stays inside  C * E + TINY  on every element (this is the
measurement C comes from, kept as a test); and each fault such kernels usually have, injected into a copy of the restatement,
exceeds that bound by at least 100x on at least one element.  Runs on the CPU."""
import itertools

import numpy as np
import pytest
import torch

import comp_reference as cr
from oracle import mofa_oracle as orc

CONFIGS = list(itertools.product((False, True), repeat=3))            # noise, shared z, white background
OUTPUTS = ("weights", "rgb", "acc", "depth", "disp", "d_raw rgb", "d_raw sigma", "d_rays_d")


def oracle_autograd(b, white, dtype):
    """oracle.raw2outputs and torch autograd in `dtype` on a batch: the forward results and the two gradients, as NumPy arrays"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    raw, d = t(b["raw"]).requires_grad_(True), t(b["rays_d"]).requires_grad_(True)
    z = t(b["z"])
    z = z[None, :].expand(b["R"], b["S"]) if z.dim() == 1 else z
    rgb, disp, acc, w, depth = orc.raw2outputs(raw, z, d, None if b["noise"] is None else t(b["noise"]), white)
    loss = (rgb * t(b["g_rgb"])).sum() + (disp * t(b["g_disp"])).sum() + (acc * t(b["g_acc"])).sum() + \
        (depth * t(b["g_depth"])).sum() + (w * t(b["g_weights"])).sum()
    loss.backward()
    n = lambda a: a.detach().double().numpy()
    return dict(weights=n(w), rgb=n(rgb), acc=n(acc), depth=n(depth), disp=n(disp), d_raw=n(raw.grad), d_rays_d=n(d.grad))


def restated(b, white):
    """the restatement on a batch: {output: (value, bound)}"""
    F = cr.Forward(b["raw"], b["z"], b["rays_d"], b["noise"], white)
    d_raw, E_raw, d_rd, E_rd = cr.backward(F, b["g_rgb"], b["g_disp"], b["g_acc"], b["g_depth"], b["g_weights"])
    return {"weights": (F.w, F.EW), "rgb": (F.rgb, F.Ergb), "acc": (F.acc, F.Eacc), "depth": (F.depth, F.Edepth), "disp": (F.disp, F.Edisp),
            "d_raw rgb": (d_raw[..., :3], E_raw[..., :3]), "d_raw sigma": (d_raw[..., 3], E_raw[..., 3]), "d_rays_d": (d_rd, E_rd)}


def split(o):
    """the oracle's / a kernel's results under the names of `restated`"""
    return {"weights": o["weights"], "rgb": o["rgb"], "acc": o["acc"], "depth": o["depth"], "disp": o["disp"],
            "d_raw rgb": o["d_raw"][..., :3], "d_raw sigma": o["d_raw"][..., 3], "d_rays_d": o["d_rays_d"]}


@pytest.fixture(scope="module")
def cases():
    """every (S, noise, shared z, white): the batch and the restatement, computed once"""
    out = {}
    for S in cr.SAMPLE_COUNTS:
        for noise, shared, white in CONFIGS:
            b = cr.make_batch(S, noise, shared)
            out[S, noise, shared, white] = (b, restated(b, white))
    return out


def test_batches_are_what_the_families_say():
    for S in cr.SAMPLE_COUNTS:
        b0 = cr.make_batch(S)
        assert b0["R"] % 2 == 1 and len(b0["family"]) == b0["R"]
        assert all(np.array_equal(v, cr.make_batch(S)[k]) for k, v in b0.items() if isinstance(v, np.ndarray))     # the same rays every time
        for noise, shared in itertools.product((False, True), repeat=2):
            b = cr.make_batch(S, noise, shared)
            F = cr.Forward(b["raw"], b["z"], b["rays_d"], b["noise"])
            assert (F.dlt > 0).all()
            for r, fam in enumerate(b["family"]):
                if fam == "thin":
                    assert (F.x[r] > 2.0 ** -25).all() and (F.x[r] < 1.1e-3).all()
                elif fam in ("empty", "zero"):
                    assert F.acc[r] == 0.0 and ((F.sg[r] == 0).all() if fam == "zero" else (F.sg[r] < 0).all())
                elif fam.startswith("surface"):
                    p, k = (int(t.split("=")[1]) for t in fam.split()[1:])
                    assert np.allclose(F.x[r, p:p + k], cr.X_OPAQUE, rtol=1e-5) and (F.x[r, :p] < 0.11).all()
                    assert p == 0 or F.sg[r, p - 1] > 0
                elif fam == "last only":
                    assert (F.sg[r, :-1] < 0).all() and F.sg[r, -1] == np.float32(1e-9)
                elif fam == "long opaque run":
                    assert b["behind_run"][r].any() and np.allclose(F.x[r, S // 3:S // 3 + 8], cr.X_OPAQUE, rtol=1e-5)
                    assert np.abs(F.w[r][b["behind_run"][r]]).max() < 1e-70
        places = {int(f.split()[1][2:]) for f in b0["family"] if f.startswith("surface")}
        assert places >= {p for p in (0, 1, S // 2, 63, 64, 127, 128, 255, 256, S - 2, S - 1) if p < S}


def test_restatement_agrees_with_fp64_autograd(cases):
    worst = 0.0
    for key, (b, ref) in cases.items():
        got = split(oracle_autograd(b, key[3], torch.float64))
        for name in OUTPUTS:
            val = ref[name][0]
            nan = np.isnan(val)
            assert (np.isnan(got[name]) == nan).all(), (key, name)
            scale = np.abs(np.where(nan, 0.0, val)).max()
            err = np.abs(np.where(nan, 0.0, got[name] - val)).max()
            worst = max(worst, err / max(scale, 1e-300))
            assert err <= 1e-12 * scale, (key, name, err, scale)
    print(f"restatement vs fp64 autograd: worst error / tensor scale = {worst:.2e}")


def test_fp32_oracle_stays_inside_the_bound(cases):
    """The reference's own fp32 arithmetic (sequential cumprod, torch's sums, its autograd): the worst |err| / (E + TINY) per output is
    what C is four times of."""
    worst = {name: 0.0 for name in OUTPUTS}
    for key, (b, ref) in cases.items():
        got = split(oracle_autograd(b, key[3], torch.float32))
        for name in OUTPUTS:
            worst[name] = max(worst[name], cr.assert_inside(got[name], *ref[name], f"fp32 oracle {key} {name}"))
    print("fp32 oracle, worst |err| / (E + TINY): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) <= cr.C / 4.0 + 1e-9, "C is four times the measured ratio: re-measure"


# ---- the faults ---------------------------------------------------------------------------------------------------------------------------
def faulty(b, white, fault):
    """A copy of the restatement's values (no bounds) with one fault injected; lanes and passes as the kernels lay them out: SPL = 1, 2, 4
    samples per lane up to 64, 128, 256 samples, passes of 256 samples (SPL = 4) beyond."""
    raw, d = b["raw"].astype(np.float64), b["rays_d"].astype(np.float64)
    R, S = raw.shape[:2]
    z = np.broadcast_to(b["z"].astype(np.float64), (R, S))
    if fault == "shared z read with stride S":                      # ray r reads S floats further on: somebody else's positions
        z = b["z_rows"].astype(np.float64)
    nz = 0.0 if b["noise"] is None else b["noise"].astype(np.float64)
    dnorm = np.sqrt((d * d).sum(-1))
    dlt = np.concatenate([z[:, 1:] - z[:, :-1], np.full((R, 1), 1e10)], -1)
    dist = dlt * dnorm[:, None]
    if fault == "last distance without |d|":
        dist[:, -1] = 1e10
    sg = raw[..., 3] + nz
    rs = np.maximum(sg, 0.0)
    if fault == "noise after the ReLU":
        rs = np.maximum(raw[..., 3], 0.0) + nz
    x = rs * dist
    e = np.exp(-x)
    a = 1.0 - e
    m = e + (0.0 if fault == "1e-10 dropped" else 1e-10)
    T = np.cumprod(m, -1) if fault == "inclusive product" else cr._excl_prefix(m, np.cumprod)
    spl = 1 if S <= 64 else 2 if S <= 128 else 4
    idx = np.arange(S)
    if fault == "carry one pass late" and S > 256:
        total = np.cumprod(m, -1)                                   # pass p gets the carry that belongs in front of pass p - 1
        for p in range(1, (S + 255) // 256):
            late = total[:, 256 * (p - 1) - 1] if p >= 2 else np.ones(R)
            T[:, 256 * p:256 * (p + 1)] *= (late / total[:, 256 * p - 1])[:, None]
    w = a * T
    c = 1.0 / (1.0 + np.exp(-raw[..., :3]))
    acc, depth = w.sum(-1), (w * z).sum(-1)
    rgb = (w[..., None] * c).sum(1) + ((1.0 - acc)[:, None] if white else 0.0)
    g_rgb, g_disp = b["g_rgb"].astype(np.float64), b["g_disp"].astype(np.float64)
    live = acc > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        disp = np.where(live, 1.0 / np.maximum(1e-10, depth / acc), np.nan)
        poison = np.where(~live & (g_disp != 0), np.nan, 0.0)
        gdep = b["g_depth"] + g_disp * np.where(live, -acc / depth ** 2, 0.0) + poison
        gacc = b["g_acc"] + g_disp * np.where(live, 1.0 / depth, 0.0) + poison
    if white and fault != "g_acc without the white term":
        gacc = gacc - g_rgb.sum(-1)
    G = b["g_weights"] + (g_rgb[:, None, :] * c).sum(-1) + gdep[:, None] * z + gacc[:, None]
    Gw = G * w
    A = cr._excl_suffix_sum(Gw)
    if fault == "suffix sum includes j":
        A = A + Gw
    if fault in ("suffix sum misses lane l+1's first sample", "suffix sum misses the next pass's first sample"):
        nxt = (idx // spl + 1) * spl                                # the first sample of the next lane
        at_pass = nxt % 256 == 0
        hit = (nxt < S) & (at_pass if fault.endswith("pass's first sample") else ~at_pass)
        A[:, hit] -= Gw[:, nxt[hit]]
    dalpha = G * T - A / m
    keep = 1.0 if fault == "keep taken as 1" else e
    d_raw = np.zeros((R, S, 4))
    gate = (raw[..., 3] > 0) if fault == "noise after the ReLU" else (sg > 0)
    d_raw[..., 3] = np.where(gate, dalpha * dist * keep, 0.0)
    d_raw[..., :3] = w[..., None] * g_rgb[:, None, :] * c * (1.0 - c)
    dn = (dalpha * rs * keep * dlt).sum(-1)
    return split(dict(weights=w, rgb=rgb, acc=acc, depth=depth, disp=disp, d_raw=d_raw, d_rays_d=dn[:, None] * (d / dnorm[:, None])))


def over(got, ref, E):
    """worst |got - ref| / (C * E + TINY) over the elements that are numbers on both sides (a fault is to show there, not only by a NaN)"""
    ok = np.isfinite(ref) & np.isfinite(got)
    if not ok.any():
        return 0.0
    return float((np.abs(np.where(ok, got - ref, 0.0)) / (cr.C * np.where(ok, E, 0.0) + cr.TINY)).max())


FAULTS = {                                                           # fault -> the sample counts at which it must show
    "1e-10 dropped": cr.SAMPLE_COUNTS,
    "inclusive product": cr.SAMPLE_COUNTS,
    "suffix sum includes j": cr.SAMPLE_COUNTS,
    "suffix sum misses lane l+1's first sample": (64, 128, 256, 65, 129, 257, 513),     # SPL = 1, 2, 4, and inside a pass
    "suffix sum misses the next pass's first sample": (257, 513),
    "carry one pass late": (257, 513),
    "last distance without |d|": cr.SAMPLE_COUNTS,
    "g_acc without the white term": cr.SAMPLE_COUNTS,
    "noise after the ReLU": cr.SAMPLE_COUNTS,
    "keep taken as 1": cr.SAMPLE_COUNTS,
    "shared z read with stride S": cr.SAMPLE_COUNTS,
}


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.filterwarnings("ignore::RuntimeWarning")              # a fault may overflow or divide by zero: that is one way of being wrong
def test_every_fault_exceeds_the_bound_a_hundredfold(cases, fault):
    for S in FAULTS[fault]:
        worst, where = 0.0, None
        for (s, noise, shared, white), (b, ref) in cases.items():
            if s != S or (fault == "g_acc without the white term" and not white) or (fault == "noise after the ReLU" and not noise) or \
                    (fault == "shared z read with stride S" and not shared):
                continue
            got = faulty(b, white, fault)
            for name in OUTPUTS:
                r = over(got[name], *ref[name])
                if r > worst:
                    worst, where = r, (name, noise, shared, white)
        print(f"{fault}, S = {S}: worst |err| / bound = {worst:.2e} at {where}")
        assert worst >= 100.0, (fault, S, worst, where)


def test_the_copy_without_a_fault_is_the_restatement(cases):
    for (S, noise, shared, white), (b, ref) in cases.items():
        got = faulty(b, white, None)
        for name in OUTPUTS:
            assert np.array_equal(got[name], ref[name][0], equal_nan=True), (S, name)

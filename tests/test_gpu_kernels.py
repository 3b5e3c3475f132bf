"""GPU parity tests of the individual HIP kernels, called through the C ABI (ctypes), against the CPU oracle on
the same seeded inputs and against the committed golden fixtures.  Floating-point path: tolerances are stated
per test (fp32; north-star budget is 1e-4 max-abs on RGB)."""
import numpy as np
import pytest
import torch

from conftest import nan_equal_close
from mofanerf_amd import lib, schema, synth
from oracle import mofa_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = torch.from_numpy


def L():
    return lib.load()


def dev(x):
    return (T(x) if isinstance(x, np.ndarray) else x).float().contiguous().to(DEV)


def test_library_loaded_from_tree():
    assert lib.LIB_PATH.endswith("mofanerf_amd/libmofanerf_hip.so")
    assert L().mofa_abi_version() == 5


def test_positional_encode_golden(golden):
    g = golden("kat.npz")
    x = dev(g["embed_x"])
    for nf, key in ((10, "embed_L10"), (4, "embed_L4")):
        out = torch.empty(x.shape[0], 3 + 6 * nf, device=DEV)
        lib.check(L().mofa_positional_encode(lib.ptr(x), x.shape[0], nf, lib.ptr(out), lib.stream()), "pe")
        # arguments reach 6e3 rad; OCML sinf/cosf vs torch CPU (SLEEF): <= 2 ulp of a value in [-1,1]
        nan_equal_close(out.cpu().numpy(), g[key], 3e-7)


def test_panels_roundtrip():
    rng = np.random.default_rng(0)
    for rows, k in ((300, 63), (512, 128), (1000, 40)):
        x = dev(rng.normal(size=(rows, k)).astype(np.float32))
        rp = (rows + 255) // 256 * 256
        p = torch.full((L().mofa_panel_floats(rp, k),), float("nan"), device=DEV)
        lib.check(L().mofa_to_panels(lib.ptr(x), rows, k, lib.ptr(p), rp, lib.stream()), "to_panels")
        y = torch.empty_like(x)
        lib.check(L().mofa_from_panels(lib.ptr(p), rp, rows, k, lib.ptr(y), lib.stream()), "from_panels")
        assert torch.equal(x, y)
        kp = (k + 15) // 16 * 16
        pn = p.cpu().numpy().reshape(kp // 16, rp, 16)
        xn = x.cpu().numpy()
        for (r, kk) in ((0, 0), (5, 7), (rows - 1, k - 1), (17, 33 % k)):     # documented address formula
            assert pn[kk // 16, r, (((kk % 16) // 4) ^ ((r // 4) % 4)) * 4 + kk % 4] == xn[r, kk]
        assert not np.isnan(pn).any()


def _layer(x1, w, b, x2=None, relu=True, bias_rows=None, div=0):
    """y = act([x1|x2] @ w.T + b) through mofa_to_panels / mofa_pack_panels / mofa_layer_forward."""
    M, k1 = x1.shape
    n_out = w.shape[0]
    Mp, Np = (M + 255) // 256 * 256, (n_out + 63) // 64 * 64
    k1p = (k1 + 15) // 16 * 16
    k2 = 0 if x2 is None else x2.shape[1]
    k2p = (k2 + 15) // 16 * 16
    st = lib.stream()
    p1 = torch.empty(L().mofa_panel_floats(Mp, k1), device=DEV)
    lib.check(L().mofa_to_panels(lib.ptr(x1), M, k1, lib.ptr(p1), Mp, st), "to_panels")
    p2 = None
    if x2 is not None:
        p2 = torch.empty(L().mofa_panel_floats(Mp, k2), device=DEV)
        lib.check(L().mofa_to_panels(lib.ptr(x2), M, k2, lib.ptr(p2), Mp, st), "to_panels")
    wp = torch.empty(Np * (k1p + k2p), device=DEV)
    lib.check(L().mofa_pack_panels(lib.ptr(w), n_out, w.shape[1], 0, k1, lib.ptr(wp), Np, 0, k1p, st), "pack")
    if x2 is not None:
        lib.check(L().mofa_pack_panels(lib.ptr(w), n_out, w.shape[1], k1, k2, lib.ptr(wp), Np, k1p // 16, k2p, st), "pack")
    if bias_rows is None:
        bp = torch.zeros(Np, device=DEV)
        bp[:n_out] = b
        nb = 1
    else:
        bp = torch.zeros(bias_rows.shape[0], Np, device=DEV)
        bp[:, :n_out] = bias_rows
        nb = bias_rows.shape[0]
    yp = torch.full((Mp * Np,), float("nan"), device=DEV)
    lib.check(L().mofa_layer_forward(lib.ptr(p1), k1p, lib.ptr(p2), k2p, lib.ptr(wp), lib.ptr(bp), div, nb,
                                     lib.ptr(yp), Mp, Np, int(relu), st), "layer")
    y = torch.empty(M, n_out, device=DEV)
    lib.check(L().mofa_from_panels(lib.ptr(yp), Mp, M, n_out, lib.ptr(y), st), "from_panels")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("M,K,N", [(256, 64, 64), (700, 128, 128), (1024, 256, 256), (513, 96, 192), (2048, 1024, 128)])
def test_layer_forward(M, K, N):
    """One Linear+bias+ReLU.  Weights are ASYMMETRIC random (catches transposed operands / C layout)."""
    rng = np.random.default_rng(M + K + N)
    x = dev(rng.normal(size=(M, K)).astype(np.float32))
    w = dev((rng.normal(size=(N, K)) / np.sqrt(K)).astype(np.float32))
    b = dev(rng.normal(size=(N,)).astype(np.float32))
    ref = torch.relu(x.double().cpu() @ w.double().cpu().T + b.double().cpu()).float().numpy()
    y = _layer(x, w, b).cpu().numpy()
    # fp32 fmaf chain vs fp64: ~1.5e-7 * sum|a*b| (cdna_hip_programming.md §3)
    nan_equal_close(y, ref, 2e-5 if K >= 1024 else 5e-6)


def test_layer_forward_identity_weight():
    """A = I against an asymmetric X: y must equal relu(x) exactly (layout check, no rounding involved)."""
    rng = np.random.default_rng(3)
    x = dev(rng.normal(size=(512, 128)).astype(np.float32))
    w = torch.eye(128, device=DEV)
    y = _layer(x, w, torch.zeros(128, device=DEV))
    assert torch.equal(y, torch.relu(x))
    y = _layer(x, w, torch.zeros(128, device=DEV), relu=False)
    assert torch.equal(y, x)


def test_layer_forward_skip_concat_and_per_ray_bias():
    rng = np.random.default_rng(11)
    M, K1, K2, N, S = 640, 64, 128, 128, 64
    x1, x2 = dev(rng.normal(size=(M, K1)).astype(np.float32)), dev(rng.normal(size=(M, K2)).astype(np.float32))
    w = dev((rng.normal(size=(N, K1 + K2)) / 12).astype(np.float32))
    b = dev(rng.normal(size=(N,)).astype(np.float32))
    ref = torch.relu(torch.cat([x1, x2], 1).double() @ w.double().T + b.double()).float().cpu().numpy()
    nan_equal_close(_layer(x1, w, b, x2=x2).cpu().numpy(), ref, 5e-6)
    rows = dev(rng.normal(size=(M // S, N)).astype(np.float32))
    ref = torch.relu(x1.double() @ w[:, :K1].double().T + rows.double().repeat_interleave(S, 0)).float().cpu().numpy()
    nan_equal_close(_layer(x1, w[:, :K1].contiguous(), None, bias_rows=rows, div=S).cpu().numpy(), ref, 5e-6)


def test_pipelined_k_loop_is_bit_identical(knob):
    """The shipped K loop (kloop_pipelined: fragment reads and LDS-DMA requests interleaved with the MFMAs, requests a full panel
    ahead) against the plain loop it replaced (MOFA_PIPE=0): forward (plain, skip layer with two K sources, per-ray bias, ragged
    point count, the smallest eligible K = 64) and backward-data (mask + accumulate) must agree bit for bit; K = 48 (odd panel
    count) silently takes the plain loop."""
    rng = np.random.default_rng(22)
    M, K, N, S = 256 * 67, 256, 1024, 64
    x = dev(rng.normal(size=(M, K)).astype(np.float32))
    x2 = dev(rng.normal(size=(M, 128)).astype(np.float32))
    w = dev((rng.normal(size=(N, K + 128)) / 16).astype(np.float32))
    b = dev(rng.normal(size=(N,)).astype(np.float32))
    rows = dev(rng.normal(size=(M // S, 128)).astype(np.float32))
    st = lib.stream()
    gk, ko = 256, 384                             # backward data: dX[M, ko] = G[M, gk] @ Wt, raw panel buffers
    g_p = dev(rng.normal(size=(M * gk,)).astype(np.float32))
    wt_p = dev((rng.normal(size=(ko * gk,)) / 16).astype(np.float32))
    mask_p = dev(rng.normal(size=(M * ko,)).astype(np.float32))
    dx0 = dev(rng.normal(size=(M * ko,)).astype(np.float32))

    def bwd(accumulate=1, masked=True):
        dx = dx0.clone()
        lib.check(L().mofa_layer_backward_data(lib.ptr(g_p), gk, lib.ptr(wt_p), lib.ptr(mask_p) if masked else None, accumulate,
                                               lib.ptr(dx), M, ko, st), "bwd")
        return dx

    cases = [lambda: _layer(x, w[:, :K].contiguous(), b), lambda: _layer(x, w, b, x2=x2),
             lambda: _layer(x, w[:128, :K].contiguous(), None, bias_rows=rows, div=S),
             lambda: _layer(x[:700], w[:128, :K].contiguous(), b[:128]),
             lambda: _layer(x[:, :64].contiguous(), w[:256, :64].contiguous(), b[:256]),
             lambda: _layer(x[:, :48].contiguous(), w[:256, :48].contiguous(), b[:256]),
             lambda: _layer(x, w[:192, :K].contiguous(), b[:192]),                      # 64-feature tile (width not a multiple of 128)
             lambda: _layer(x, w[:64], b[:64], x2=x2), bwd, lambda: bwd(0, True), lambda: bwd(1, False), lambda: bwd(0, False)]
    knob("MOFA_PIPE", "0")
    base = [c() for c in cases]
    knob("MOFA_PIPE", "1")
    for c, ref in zip(cases, base):
        for _ in range(2):
            assert torch.equal(c(), ref)


def test_pipelined_weight_gradient_loop_is_bit_identical(knob):
    """k_wgrad<128,256>'s software-pipelined chunk loop (default) against its plain loop (MOFA_PIPE=0): dW and the bias sums
    that ride along must agree bit for bit — even chunk counts take the pipelined loop, a ragged point count (last chunk
    partly empty) and an odd chunk count silently take the plain one."""
    rng = np.random.default_rng(23)
    Np, Kp, Mp = 256, 512, 256 * 40
    g_p = dev(rng.normal(size=(Mp * Np,)).astype(np.float32))
    x_p = dev(rng.normal(size=(Mp * Kp,)).astype(np.float32))
    st = lib.stream()

    def run(n_points):
        ws = torch.empty(L().mofa_weight_grad_workspace_floats(n_points, Np, Kp), device=DEV)
        dw, db = torch.zeros(Np, Kp, device=DEV), torch.zeros(Np, device=DEV)
        lib.check(L().mofa_weight_grad(lib.ptr(g_p), Np, lib.ptr(x_p), Kp, Mp, n_points, Np, Kp, lib.ptr(dw), Kp, 0, lib.ptr(db),
                                       lib.ptr(ws), st), "weight_grad")
        return dw, db

    sizes = [Mp, Mp - 256 * 3, 16 * 250, 16 * 250 - 5, 16 * 7]
    knob("MOFA_PIPE", "0")
    base = [run(n) for n in sizes]
    knob("MOFA_PIPE", "1")
    for n, (dw0, db0) in zip(sizes, base):
        dw, db = run(n)
        assert torch.equal(dw, dw0) and torch.equal(db, db0), n
    dw, db = base[0]                                   # and the numbers themselves: every element of dW and db against fp64
    import bwd_reference as br
    ref_dw, cond_dw, ref_db, cond_db = br.weight_grad(_unswizzle(g_p, Mp, Np), _unswizzle(x_p, Mp, Kp), Mp)
    br.assert_close(dw, ref_dw, cond_dw, "weight_grad 256x512 n=10240 dW")
    br.assert_close(db, ref_db, cond_db, "weight_grad 256x512 n=10240 db")


def _unswizzle(panels, Mp, K):
    """[K/16][Mp][16] swizzled panels -> [Mp, K] (inverse of mofa_to_panels, through the library)."""
    out = torch.empty(Mp, K, device=DEV)
    lib.check(L().mofa_from_panels(lib.ptr(panels), Mp, Mp, K, lib.ptr(out), lib.stream()), "from_panels")
    return out


@pytest.mark.parametrize("n_points", [1, 700, 4096, 4 * 1024 * 3 + 517, 131072])
def test_bias_gradient_column_sums(n_points):
    """`mofa_bias_grad` (k_colsum): column sums of a gradient panel buffer over the first n_points rows — full unrolled rounds,
    the ragged remainder and fewer rows than threads — against fp64 sums, and run-to-run identical (fixed summation order)."""
    rng = np.random.default_rng(31 + n_points % 7)
    N = 128
    Mp = (n_points + 255) // 256 * 256
    g = dev(rng.normal(size=(Mp, N)).astype(np.float32))
    gp = torch.empty(L().mofa_panel_floats(Mp, N), device=DEV)
    lib.check(L().mofa_to_panels(lib.ptr(g), Mp, N, lib.ptr(gp), Mp, lib.stream()), "to_panels")
    outs = []
    for _ in range(2):
        out = torch.empty(N, device=DEV)
        lib.check(L().mofa_bias_grad(lib.ptr(gp), Mp, n_points, N, lib.ptr(out), lib.stream()), "bias_grad")
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    ref = g[:n_points].double().sum(0)
    assert torch.allclose(outs[0].double(), ref, rtol=0, atol=2e-6 * max(1.0, float(n_points) ** 0.5) * 4)


def test_layer0_positional_encoding_fused():
    """layer 0 = PE(o + d*z) @ W[:, :63].T + b, ReLU; compared with the oracle's PE + a torch fp64 matmul."""
    rng = np.random.default_rng(5)
    R, S, N = 37, 64, 128
    o = dev(rng.uniform(-3, 3, (R, 3)).astype(np.float32))
    d = dev(rng.normal(0, 0.6, (R, 3)).astype(np.float32))
    z = dev(np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1))
    w = dev((rng.normal(size=(N, 63)) / 8).astype(np.float32))
    b = dev(rng.normal(size=(N,)).astype(np.float32))
    M = R * S
    Mp = (M + 255) // 256 * 256
    st = lib.stream()
    wp = torch.empty(N * 64, device=DEV)
    lib.check(L().mofa_pack_panels(lib.ptr(w), N, 63, 0, 63, lib.ptr(wp), N, 0, 64, st), "pack")
    yp = torch.empty(Mp * N, device=DEV)
    y, y2 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    lib.check(L().mofa_layer0_forward(lib.ptr(o), lib.ptr(d), lib.ptr(z), S, None, M, S, 10, lib.ptr(wp), lib.ptr(b),
                                      lib.ptr(yp), Mp, N, None, st), "layer0")
    lib.check(L().mofa_from_panels(lib.ptr(yp), Mp, M, N, lib.ptr(y), st), "from_panels")
    pts = (o.cpu()[:, None, :] + d.cpu()[:, None, :] * z.cpu()[:, :, None]).reshape(-1, 3)
    lib.check(L().mofa_layer0_forward(None, None, None, 0, lib.ptr(dev(pts)), M, S, 10, lib.ptr(wp), lib.ptr(b), lib.ptr(yp),
                                      Mp, N, None, st), "layer0/pts")
    lib.check(L().mofa_from_panels(lib.ptr(yp), Mp, M, N, lib.ptr(y2), st), "from_panels")
    pe = orc.positional_encode(pts, 10).double()
    ref = torch.relu(pe @ w.double().cpu().T + b.double().cpu()).float().numpy()
    # fp32 fmaf-chain: sqrt(K)*2^-24*|partial sums| ~ 1e-6 * sum_k |a_k b_k| (raw x features reach |x| ~ 50 here)
    bound = (1e-6 * (pe.abs() @ w.double().cpu().abs().T + b.double().cpu().abs()) + 1e-6).numpy()
    err = np.abs(y2.cpu().numpy() - ref)
    assert (err <= bound).all(), float((err - bound).max())
    assert torch.equal(y, y2)      # in-kernel o + d*z is bit-identical to the separately rounded torch ops


def test_head_and_view_bias():
    rng = np.random.default_rng(9)
    M, K = 777, 128
    x = dev(rng.normal(size=(M, K)).astype(np.float32))
    w = dev((rng.normal(size=(3, K)) / 11).astype(np.float32))
    b = dev(rng.normal(size=(3,)).astype(np.float32))
    Mp = (M + 255) // 256 * 256
    st = lib.stream()
    xp = torch.empty(L().mofa_panel_floats(Mp, K), device=DEV)
    lib.check(L().mofa_to_panels(lib.ptr(x), M, K, lib.ptr(xp), Mp, st), "to_panels")
    raw = torch.zeros(M, 4, device=DEV)
    lib.check(L().mofa_head_forward(lib.ptr(xp), K, Mp, lib.ptr(w), lib.ptr(b), 3, lib.ptr(raw), 0, M, st), "head")
    lib.check(L().mofa_head_forward(lib.ptr(xp), K, Mp, lib.ptr(w[1:2].contiguous()), lib.ptr(b[1:2].contiguous()), 1,
                                    lib.ptr(raw), 3, M, st), "head")
    ref = (x.double() @ w.double().T + b.double()).float().cpu().numpy()
    nan_equal_close(raw[:, :3].cpu().numpy(), ref, 3e-6)
    nan_equal_close(raw[:, 3].cpu().numpy(), ref[:, 1], 3e-6)
    R, n_out, ld = 50, 96, 27 + 192
    vd = torch.nn.functional.normalize(dev(rng.normal(size=(R, 3)).astype(np.float32)), dim=-1).contiguous()
    wv = dev((rng.normal(size=(n_out, ld)) / 5).astype(np.float32))
    bv = dev(rng.normal(size=(n_out,)).astype(np.float32))
    out = torch.full((R, 128), float("nan"), device=DEV)
    lib.check(L().mofa_view_bias(lib.ptr(vd), R, 4, lib.ptr(wv), n_out, ld, lib.ptr(bv), lib.ptr(out), 128, st), "view_bias")
    ref = (orc.positional_encode(vd.cpu(), 4).double() @ wv[:, :27].double().cpu().T + bv.double().cpu()).float().numpy()
    nan_equal_close(out[:, :n_out].cpu().numpy(), ref, 2e-6)
    assert (out[:, n_out:] == 0).all()


@pytest.mark.parametrize("D,W", [(8, 64), (10, 64), (8, 96)])
def test_net_forward_golden(golden, D, W):
    """`NeRF.forward(input_pts, input_bmCodes, input_views, input_uvCodes)` (models/model.py:121-137) in the reference module's OWN
    call form — per-point, already-embedded inputs — against the reference's outputs `nerf{D}x{W}_out` of the KAT fixture, and the
    fused path (`mofa_net_pack` + `mofa_net_fold` + `mofa_net_forward` from explicit points) against the oracle."""
    from mofanerf_amd.hipnet import HipNet
    from mofanerf_amd.model import NeRF
    g = golden("kat.npz")
    rng = np.random.default_rng(D * W)
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50,
               use_viewdirs=True)
    st = synth.nerf_state(D, W)
    net.load_state_dict(st)
    net = net.to(DEV)
    t = f"nerf{D}x{W}"
    n = g[t + "_pts"].shape[0]
    with torch.no_grad():
        out = net(dev(g[t + "_pts"]), dev(g[t + "_bm"]).expand(n, -1), dev(g[t + "_views"]), dev(g[t + "_tex"]).expand(n, -1))
    torch.cuda.synchronize()
    err = nan_equal_close(out.cpu().numpy(), g[t + "_out"], 2e-5, 1e-5)
    print(t, f"NeRF.forward on embedded inputs vs the reference: {err:.2e}")
    with pytest.raises(RuntimeError):                # gradients through this entry are refused, not silently dropped
        net(dev(g[t + "_pts"]), dev(g[t + "_bm"]).expand(n, -1), dev(g[t + "_views"]), dev(g[t + "_tex"]).expand(n, -1))
    R, S = 23, 64
    pts = T(rng.uniform(-9, 9, (R, S, 3)).astype(np.float32))
    vd = torch.nn.functional.normalize(T(rng.normal(size=(R, 3)).astype(np.float32)), dim=-1)
    bm, tex, exp = synth.codes(1)
    e = T(rng.uniform(-1, 1, (1, 30)).astype(np.float32))
    h = HipNet(net)
    folded = h.fold(e.to(DEV), bm.to(DEV), tex.to(DEV))
    raw = torch.empty(R, S, 4, device=DEV)
    h.forward_points(dev(pts.reshape(-1, 3)), dev(vd), S, raw, folded)
    torch.cuda.synchronize()
    n = R * S
    x93 = torch.cat([orc.positional_encode(pts.reshape(-1, 3), 10), e.expand(n, -1)], -1)
    v27 = orc.positional_encode(vd[:, None].expand(R, S, 3).reshape(-1, 3), 4)
    ref = orc.nerf_forward(st, x93, bm.expand(n, -1), v27, tex[None].expand(n, -1)).reshape(R, S, 4)
    nan_equal_close(raw.cpu().numpy(), ref.numpy(), 2e-5, 1e-5)
    # the nominal (unfolded, embedded-input) entry and the fused entry agree with each other on the same points
    with torch.no_grad():
        emb = net(dev(x93), dev(bm).expand(n, -1), dev(v27), dev(tex[None]).expand(n, -1)).reshape(R, S, 4)
    nan_equal_close(emb.cpu().numpy(), raw.cpu().numpy(), 2e-5, 1e-5)


def test_reference_eager_run_network_body_runs_on_these_classes(golden):
    """The body of the reference's eager `run_network` (models/render_class.py:69-94: embed, expand the codes, `batchify(fn, netchunk)`)
    written against THESE classes — `get_embedder`, `Renderer.batchify`, `NeRF.forward` — reproduces the reference's KAT output and
    the fused `run_network`."""
    from mofanerf_amd.embedder import get_embedder
    from mofanerf_amd.model import NeRF
    from mofanerf_amd.renderer import Renderer
    g = golden("kat_run_network.npz")
    D, W = 10, 64
    t = f"rn{D}x{W}"
    _, _, netchunk, wseed, exp_type = [int(v) for v in g[t + "_meta"]]
    embed_fn, _ = get_embedder(10, 0)
    embeddirs_fn, _ = get_embedder(4, 0)
    render = Renderer(embed_fn=embed_fn, embeddirs_fn=embeddirs_fn, netchunk=netchunk, expCodesLen=30)
    render.idSpecificMod.load_state_dict(synth.style_state(0))
    for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(0)):
        dst.data[:] = src
    render = render.to(DEV).eval()
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, wseed, "kat"))
    net = net.to(DEV)
    inputs, viewdirs = dev(g[t + "_pts"]), dev(g[t + "_vd"])
    render.shapeCodes, render.expType, render.decoding_texCodes = dev(g[t + "_bm"]), exp_type, dev(g[t + "_tex"])
    with torch.no_grad():
        inputs_flat = torch.reshape(inputs, [-1, inputs.shape[-1]])
        shapeCodes = render.shapeCodes[0, :].expand([inputs_flat.shape[0], render.shapeCodes.shape[-1]])
        exp_scale, exp_bias = render.idSpecificMod(render.shapeCodes[0, :].reshape(1, -1))
        embedded = render.embed_fn(inputs_flat)
        code = (exp_scale * render.expCodes_Sigma[render.expType] + exp_bias).expand([inputs_flat.shape[0], -1])
        embedded = [torch.cat([embedded, code], -1), shapeCodes]
        input_dirs_flat = torch.reshape(viewdirs[:, None].expand(inputs.shape), [-1, 3])
        embedded.append(render.embeddirs_fn(input_dirs_flat))
        outputs = torch.reshape(render.batchify(net, render.netchunk)(embedded), list(inputs.shape[:-1]) + [4])
        fused = render.run_network(inputs, viewdirs, net)
    nan_equal_close(outputs.cpu().numpy(), g[t + "_raw"], 2e-5, 1e-5)
    nan_equal_close(outputs.cpu().numpy(), fused.cpu().numpy(), 2e-5, 1e-5)


def test_get_rays_golden(golden):
    g = golden("kat.npz")
    K = np.array([[600., 0, 128], [0, 600., 128], [0, 0, 1]])
    for ang in (-60, 0, 60):
        c2w = dev(g[f"rays{ang}_c2w"][:3, :4])
        n = 256 * 256
        o, d, v = (torch.empty(n, 3, device=DEV) for _ in range(3))
        lib.check(L().mofa_get_rays(256, 256, 600., 600., 128., 128., lib.ptr(c2w), 0, n, lib.ptr(o), lib.ptr(d),
                                    lib.ptr(v), lib.stream()), "get_rays")
        d_img = d.reshape(256, 256, 3).cpu().numpy()
        assert np.array_equal(o[0].cpu().numpy(), g[f"rays{ang}_o"])
        assert np.array_equal(d_img[::37, ::41], g[f"rays{ang}_d_sub"])          # bit-exact ray directions
        ro, rd = orc.get_rays(256, 256, K, T(g[f"rays{ang}_c2w"])[:3, :4])
        vref = (rd / torch.norm(rd, dim=-1, keepdim=True)).reshape(-1, 3).numpy()
        nan_equal_close(v.cpu().numpy(), vref, 1.2e-7)


def _composite(raw, z, d, noise, white):
    R, S = z.shape
    o = {k: torch.empty(R, *sh, device=DEV) for k, sh in (("rgb", (3,)), ("disp", ()), ("acc", ()), ("depth", ()),
                                                          ("weights", (S,)))}
    lib.check(L().mofa_composite_forward(lib.ptr(raw), lib.ptr(z), S, lib.ptr(d), lib.ptr(noise), R, S, int(white),
                                         lib.ptr(o["rgb"]), lib.ptr(o["disp"]), lib.ptr(o["acc"]), lib.ptr(o["depth"]),
                                         lib.ptr(o["weights"]), lib.stream()), "composite")
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_composite_golden(golden):
    g = golden("kat.npz")
    for S in (64, 128):
        raw, z, d = dev(g[f"r2o{S}_raw"]), dev(g[f"r2o{S}_z"]), dev(g[f"r2o{S}_d"])
        for wb in (0, 1):
            o = _composite(raw, z, d, None, wb)
            for n in ("rgb", "disp", "acc", "weights", "depth"):       # SURVEY §8d gate: composite <= 2e-6
                nan_equal_close(o[n], g[f"r2o{S}_{wb}_{n}"], 2e-6, 2e-6)
        assert np.isnan(_composite(raw, z, d, None, 0)["disp"][0])
        np.random.seed(0)
        noise = dev((np.random.rand(*raw.shape[:2]) * 0.7).astype(np.float32))
        o = _composite(raw, z, d, noise, 0)
        for n in ("rgb", "disp", "acc", "weights", "depth"):
            nan_equal_close(o[n], g[f"r2o{S}_noise_{n}"], 2e-6, 2e-6)


def test_composite_ragged_sample_counts():
    rng = np.random.default_rng(2)
    for S in (2, 7, 63, 65, 100, 129, 200, 256):
        R = 9
        raw = T(rng.normal(0, 1.5, (R, S, 4)).astype(np.float32))
        z = T(np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1))
        d = T(rng.normal(size=(R, 3)).astype(np.float32))
        ref = orc.raw2outputs(raw, z, d, None, False)
        o = _composite(dev(raw), dev(z), dev(d), None, 0)
        for n, v in zip(("rgb", "disp", "acc", "weights", "depth"), ref):
            nan_equal_close(o[n], v.numpy(), 3e-6, 3e-6)


def _sample(z, w, u, ustride):
    R, S = z.shape
    Ni = u.shape[-1]
    zs, zf, sd = torch.empty(R, Ni, device=DEV), torch.empty(R, S + Ni, device=DEV), torch.empty(R, device=DEV)
    lib.check(L().mofa_sample_pdf_merge(lib.ptr(z), S, lib.ptr(w), lib.ptr(u), ustride, R, S, Ni, lib.ptr(zs),
                                        lib.ptr(zf), lib.ptr(sd), lib.stream()), "sample_pdf_merge")
    return zs.cpu(), zf.cpu(), sd.cpu()


def test_sample_pdf_merge_vs_oracle():
    """sample_pdf + sort + std.  The inverse CDF is ill-conditioned where a bin holds < ~1e-4 of the mass (t is divided
    by cdf[i+1]-cdf[i]), so the comparison is scaled by the bin's conditioning; well-conditioned samples must agree to
    a few ulp of z."""
    rng = np.random.default_rng(4)
    R, S, Ni = 64, 64, 64
    z = T(np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1))
    w = T((rng.uniform(0, 1, (R, S)) ** 5).astype(np.float32))
    w[0] = 0.0
    w[1] = 0.0; w[1, 30] = 1.0
    w[2, :31] = 0.0
    for u, ustride in ((torch.linspace(0., 1., Ni), 0), (T(rng.uniform(0, 1, (R, Ni)).astype(np.float32)), Ni)):
        zs, zf, sd = _sample(dev(z), dev(w), dev(u), ustride)
        zmid = .5 * (z[:, 1:] + z[:, :-1])
        ref = orc.sample_pdf(zmid, w[:, 1:-1], u)
        from harness import classify_samples
        agree, expl = classify_samples(z, w, u, zs, ref)
        assert (agree | expl).all(), int((~(agree | expl)).sum())
        assert float(agree.float().mean()) > 0.9 and float((zs - ref).abs().median()) <= 2e-6
        zref, _ = torch.sort(torch.cat([z, zs], -1), -1)
        assert torch.equal(zf, zref)                                   # merge is an exact sort of what we sampled
        nan_equal_close(sd.numpy(), torch.std(zs, dim=-1, unbiased=False).numpy(), 2e-6, 2e-6)


@pytest.mark.parametrize("seed", range(6))
def test_sample_pdf_merge_random_shapes(seed):
    """Seeded sweep over (rays, coarse samples, importance samples) incl. counts beyond one 256-sample wavefront pass and the
    4 / 2 / 1 rays-per-block layouts of the dynamic-LDS resampler: every sample agrees with the oracle's `sample_pdf` or is explained
    by its conditioning, the merged row is the exact sort, z_std matches."""
    from harness import classify_samples
    rng = np.random.default_rng(100 + seed)
    R = int(rng.integers(1, 300))
    S = int(rng.choice([4, 17, 64, 129, 256, 300, 700, 1500][seed % 8:] + [64]))
    Ni = int(rng.choice([1, 16, 64, 200, 257, 600, 2000]))
    while 3 * S + Ni > 16384:
        Ni //= 2
    z = T(np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1))
    w = T((rng.uniform(0, 1, (R, S)) ** 4).astype(np.float32))
    if R > 2:
        w[0] = 0.0
        w[1] = 0.0; w[1, S // 2] = 1.0
    for u, ustride in ((torch.linspace(0., 1., Ni), 0), (T(rng.uniform(0, 1, (R, Ni)).astype(np.float32)), Ni)):
        zs, zf, sd = _sample(dev(z), dev(w), dev(u), ustride)
        ref = orc.sample_pdf(.5 * (z[:, 1:] + z[:, :-1]), w[:, 1:-1], u)
        agree, expl = classify_samples(z, w, u, zs, ref)
        assert (agree | expl).all(), (R, S, Ni, int((~(agree | expl)).sum()))
        assert float(agree.float().mean()) > 0.85, (R, S, Ni)
        assert torch.equal(zf, torch.sort(torch.cat([z, zs], -1), -1)[0]), (R, S, Ni)
        nan_equal_close(sd.numpy(), torch.std(zs, dim=-1, unbiased=False).numpy(), 3e-6, 3e-6)


def test_sample_pdf_golden(golden):
    """`sample_pdf(bins, weights, 64, det / pytest)` (run_nerf_helpers.py:203-247) through the bins-input entry point
    `mofa_sample_pdf`, against the REFERENCE's own outputs `spdf_det` / `spdf_rand` (40 rays incl. all-zero weights, a single
    spike and leading empty bins): identical inputs, and the kernel accumulates the cdf like torch's CPU cumsum, so almost
    every sample must be within an ulp or two and the few that are not must sit on the reference's 1e-5 threshold."""
    from harness import classify_samples
    g = golden("kat.npz")
    bins, w = dev(g["spdf_bins"]), dev(g["spdf_w"])
    R, B = bins.shape
    np.random.seed(0)
    u_rand = torch.Tensor(np.random.rand(R, 64))
    for u, us, key in ((torch.linspace(0., 1., 64), 0, "spdf_det"), (u_rand, 64, "spdf_rand")):
        out, u_dev = torch.empty(R, 64, device=DEV), dev(u)
        lib.check(L().mofa_sample_pdf(lib.ptr(bins), B, lib.ptr(w), lib.ptr(u_dev), us, R, B, 64, lib.ptr(out), lib.stream()),
                  "mofa_sample_pdf")
        got, ref = out.cpu(), T(g[key])
        agree, expl = classify_samples(None, None, u, got, ref, bins=g["spdf_bins"], bin_weights=g["spdf_w"])
        assert (agree | expl).all(), (key, int((~(agree | expl)).sum()))
        frac_ulp = float(((got - ref).abs() <= 2e-6).float().mean())
        print(key, "within 2e-6:", round(frac_ulp, 4), "bit-identical:", round(float((got == ref).float().mean()), 4))
        assert frac_ulp > 0.97, (key, frac_ulp)
        assert torch.equal(got[0], ref[0])                               # all-zero weights: uniform pdf, exact
    anchor = torch.empty(1, 8, device=DEV)
    a_bins, a_w, a_u = dev(torch.linspace(8, 26, 7)[None]), dev(torch.tensor([[0, .1, .6, .2, .05, 0]])), dev(torch.linspace(0., 1., 8))
    lib.check(L().mofa_sample_pdf(lib.ptr(a_bins), 7, lib.ptr(a_w), lib.ptr(a_u), 0, 1, 7, 8, lib.ptr(anchor), lib.stream()),
              "mofa_sample_pdf")
    torch.cuda.synchronize()
    nan_equal_close(anchor.cpu().numpy(), g["spdf_anchor"], 2e-6)        # SURVEY.md section 8c sanity anchor


@pytest.mark.parametrize("D,W", [(8, 64), (10, 64), (8, 96), (10, 128)])
def test_run_network_kat_golden(golden, D, W):
    """`run_network(inputs, viewdirs, fn)` (render_class.py:69-94) on the REFERENCE's KAT: explicit points / view directions /
    codes in, raw [R,S,4] out — Embedder, expression modulation, code expansion, netchunk batching and NeRF.forward in one
    comparison against the reference's own output (fixture g9)."""
    from mofanerf_amd.model import NeRF
    from mofanerf_amd.renderer import Renderer
    g = golden("kat_run_network.npz")
    t = f"rn{D}x{W}"
    _, _, netchunk, wseed, exp_type = [int(v) for v in g[t + "_meta"]]
    render = Renderer(netchunk=netchunk, expCodesLen=30)
    render.idSpecificMod.load_state_dict(synth.style_state(0))
    for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(0)):
        dst.data[:] = src
    render = render.to(DEV).eval()
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, wseed, "kat"))
    net = net.to(DEV)
    render.shapeCodes, render.expType, render.decoding_texCodes = dev(g[t + "_bm"]), exp_type, dev(g[t + "_tex"])
    with torch.no_grad():
        raw = render.run_network(dev(g[t + "_pts"]), dev(g[t + "_vd"]), net)
    torch.cuda.synchronize()
    err = nan_equal_close(raw.cpu().numpy(), g[t + "_raw"], 2e-5, 1e-5)
    print(t, f"max abs err vs reference {err:.2e}")


def test_layer_pipeline_race_screen_full_size():
    """The LDS-DMA double buffer relies on `vmcnt(0)` + `s_barrier` ordering: run the shipped fine-net layer shape
    (196,608 points x 1024 x 1024, 6,144 workgroups) repeatedly — also with a second stream hammering HBM — and require
    bit-identical outputs every time, plus agreement with a float64 reference on sampled rows."""
    M, K, N = 196608, 1024, 1024
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(M * K, device=DEV, generator=g)           # any values: interpreted as panels
    w = torch.randn(N * K, device=DEV, generator=g) * 0.03
    b = torch.randn(N, device=DEV, generator=g)
    y = torch.empty(M * N, device=DEV)
    args = lambda out: (lib.ptr(x), K, None, 0, lib.ptr(w), lib.ptr(b), 0, 1, lib.ptr(out), M, N, 1, lib.stream())
    lib.check(L().mofa_layer_forward(*args(y)), "layer")
    ref = y.clone()
    side = torch.cuda.Stream()
    junk = torch.empty(1 << 28, device=DEV)
    for it in range(6):
        if it % 2:
            with torch.cuda.stream(side):
                for _ in range(4):
                    junk.add_(1.0)                                # concurrent HBM traffic
        y.fill_(float("nan"))
        lib.check(L().mofa_layer_forward(*args(y)), "layer")
        torch.cuda.synchronize()
        assert torch.equal(y, ref), f"run {it} differs"
    # sampled rows against float64 (un-panel with the documented address formula)
    rows = torch.tensor([0, 1, 255, 256, 70001, M - 1], device=DEV)
    xr = torch.empty(len(rows), K, device=DEV); yr = torch.empty(len(rows), N, device=DEV)
    k = torch.arange(K, device=DEV)
    for i, r in enumerate(rows.tolist()):
        idx = (k // 16) * M * 16 + r * 16 + ((((k % 16) // 4) ^ ((r // 4) % 4)) * 4) + k % 4
        xr[i] = x[idx]
        yr[i] = ref[idx]                                           # K == N: same index map
    n = torch.arange(N, device=DEV)
    kk = torch.arange(K, device=DEV)
    wd = torch.empty(N, K, device=DEV)
    widx = (kk[None, :] // 16) * N * 16 + n[:, None] * 16 + ((((kk[None, :] % 16) // 4) ^ ((n[:, None] // 4) % 4)) * 4) + kk[None, :] % 4
    wd = w[widx]
    want = torch.relu(xr.double() @ wd.double().T + b.double()).float()
    nan_equal_close(yr.cpu().numpy(), want.cpu().numpy(), 3e-5)


@pytest.mark.parametrize("D,W,R,S", [(8, 256, 40, 64), (10, 96, 9, 128), (8, 64, 130, 64), (8, 192, 17, 32), (10, 512, 300, 64), (8, 320, 150, 64),
                                     (10, 256, 1201, 64), (8, 256, 700, 128)])
def test_persistent_fused_network_is_bit_identical_to_per_layer_launches(D, W, R, S, knob):
    """Widths <= 256 run the whole MLP as ONE persistent launch (k_mlp_fused); it must reproduce the per-layer path
    bit for bit, in inference mode (recycled buffers) and in tape mode (every layer output kept).  Widths 512 / 320: several
    256-feature blocks per layer inside one workgroup (MOFA_FUSED=1 forces the persistent kernel there) — the epilogue's LDS
    windows of one block must not be overwritten by the next block's first operand fetch."""
    from mofanerf_amd.autograd import NetFn, fold_torch, view_bias_torch
    from mofanerf_amd.hipnet import HipNet
    from mofanerf_amd.model import NeRF
    rng = np.random.default_rng(D + W + R)
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50,
               use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, 1))
    h = HipNet(net.to(DEV))
    o = dev(rng.uniform(-2, 2, (R, 3)).astype(np.float32))
    d = dev(rng.normal(0, 0.3, (R, 3)).astype(np.float32))
    z = dev(np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1))
    vd = torch.nn.functional.normalize(d, dim=-1).contiguous()
    bm, tex, e = synth.codes(3)
    folded = h.fold(e.to(DEV), bm.to(DEV), tex.to(DEV)).clone()
    outs, tapes = {}, {}
    # "0": per-layer launches; "1": persistent kernels (256-wide layers: the pipelined k_mlp_fused for inference and fp32-tape forwards,
    # k_mlp_fused_generic for mask-tape forwards and every other width); "2": the same with the plain K loops (MOFA_PIPE=0: generic only)
    for mode, (fused, pipe) in {"0": ("0", "1"), "1": ("1", "1"), "2": ("1", "0")}.items():
        knob("MOFA_FUSED", fused)
        knob("MOFA_PIPE", pipe)
        raw = torch.full((R, S, 4), float("nan"), device=DEV)
        h.forward_rays(o, d, z, S, vd, S, raw, folded)
        outs[mode] = raw.clone()
        for fp32 in (False, True):
            h.force_fp32_tape = fp32
            with torch.enable_grad():
                tapes[(mode, fp32)] = NetFn.apply(h, o, d, z, S, S, folded, view_bias_torch(h, vd).detach(), None).detach().clone()
        h.force_fp32_tape = False
        torch.cuda.synchronize()
    assert torch.isfinite(outs["1"]).all()
    for mode in ("1", "2"):
        assert torch.equal(outs["0"], outs[mode]), mode
        for fp32 in (False, True):
            assert torch.equal(tapes[("0", False)], tapes[(mode, fp32)]), (mode, fp32)
    nan_equal_close(tapes[("1", True)].cpu().numpy(), outs["1"].cpu().numpy(), 2e-5)


@pytest.mark.parametrize("D,W,R,S,busy", [(10, 1024, 150, 128, False), (8, 512, 300, 64, True), (10, 1024, 3, 128, False), (8, 768, 77, 64, True),
                                          (10, 1024, 1536, 128, True)])
def test_chained_wide_network_is_bit_identical_to_per_layer_launches(D, W, R, S, busy, knob):
    """Widths > 256 run every MFMA layer of a sub-batch as ONE launch (k_net_chain: the layer kernel's tiles behind per-XCD queues and
    row-tile dependency counters).  Every word of the output must equal the per-layer launches' (MOFA_CHAIN=0) — also on a re-used
    workspace (the queue state of the previous launch is still in it), from 1 to 768 row tiles (the benchmark's sub-batch), and with
    another stream keeping the chip unevenly busy (a hand-off that is only correct on an idle chip shows up there).  The kernel's
    status words say that no dependency wait timed out and that every tile of every layer ran."""
    from mofanerf_amd.hipnet import HipNet
    from mofanerf_amd.model import NeRF
    rng = np.random.default_rng(D + W + R)
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, 1))
    h = HipNet(net.to(DEV))
    o = dev(rng.uniform(-2, 2, (R, 3)).astype(np.float32))
    d = dev(rng.normal(0, 0.3, (R, 3)).astype(np.float32))
    z = dev(np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1))
    vd = torch.nn.functional.normalize(d, dim=-1).contiguous()
    bm, tex, e = synth.codes(3)
    folded = h.fold(e.to(DEV), bm.to(DEV), tex.to(DEV)).clone()

    def run():
        raw = torch.full((R, S, 4), float("nan"), device=DEV)
        h.forward_rays(o, d, z, S, vd, S, raw, folded)
        torch.cuda.synchronize()
        return raw

    knob("MOFA_PIPE", "1")                                   # (the chained launch is built on the pipelined K loop: MOFA_PIPE=0 in the environment would select per-layer launches)
    knob("MOFA_CHAIN", "0")
    ref = run()
    assert torch.isfinite(ref).all()
    knob("MOFA_CHAIN", "1")
    Wp, Hp = (W + 63) // 64 * 64, (W // 2 + 63) // 64 * 64
    mp = (R * S + 255) // 256 * 256
    tiles = (mp // 256) * ((4 + 2 * D) * (Wp // 128) + Hp // 128)
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device=DEV)
    for it in range(3):
        if busy:                                             # a competitor for the CUs while the chained launch runs
            with torch.cuda.stream(side):
                for _ in range(6):
                    a @ a
        before = h.chained_launches()
        out = run()
        assert h.chained_launches() == before + 1            # the chained form really ran (verdict word [1], include/mofanerf_hip.h)
        h.check_verdict(block=True)                          # ... and no wait timed out, no tile is missing
        assert h._verdict_host.tolist()[2:5] == [0, tiles, tiles], (it, h._verdict_host.tolist(), tiles)
        assert torch.equal(out, ref), (it, float((out - ref).abs().max()))
    side.synchronize()


@pytest.mark.parametrize("D,W,R,S", [(8, 256, 300, 64), (10, 256, 90, 128), (8, 192, 77, 64), (8, 64, 50, 64), (10, 1024, 40, 128)])
def test_mask_tape_equals_fp32_tape_across_kernels(D, W, R, S, knob):
    """The mask-only tape (one bit per activation) against the fp32 tape, per-layer launches against the persistent kernels (the
    pipelined one at 256-wide layers, the generic one elsewhere): the mask words are bit-identical between the launch forms, equal
    (activation > 0) of the fp32 tape, and the fitting gradients computed from the bits equal the ones computed from the tape."""
    from mofanerf_amd.autograd import NetFn, fold_torch, view_bias_torch
    from mofanerf_amd.hipnet import HipNet
    from mofanerf_amd.model import NeRF
    rng = np.random.default_rng(D + W + R + 7)
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, 1))
    h = HipNet(net.to(DEV))
    o = dev(rng.uniform(-2, 2, (R, 3)).astype(np.float32))
    d = dev(rng.normal(0, 0.3, (R, 3)).astype(np.float32))
    z = dev(np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1))
    vd = torch.nn.functional.normalize(d, dim=-1).contiguous()
    bm, tex, e = synth.codes(3)
    folded = h.fold(e.to(DEV), bm.to(DEV), tex.to(DEV)).clone()
    vb = view_bias_torch(h, vd).detach().contiguous()
    G = dev(rng.normal(size=(R, S, 4)).astype(np.float32))
    Lb, st = L(), lib.stream()
    n_tape, n_mask = Lb.mofa_net_tape_floats(h.shape, R * S), Lb.mofa_net_mask_tape_words(h.shape, R * S)
    assert n_mask * 64 == n_tape
    masks, grads = {}, {}
    for fused in ("0", "1"):
        knob("MOFA_FUSED", fused)
        ws = h.workspace(R * S, R, DEV)
        raw_m, raw_t = torch.empty(R, S, 4, device=DEV), torch.empty(R, S, 4, device=DEV)
        mask = torch.zeros(n_mask, dtype=torch.int64, device=DEV)
        tape = torch.empty(n_tape, device=DEV)
        for raw, tp, mk in ((raw_m, None, mask), (raw_t, tape, None)):
            lib.check(Lb.mofa_net_forward(h.shape, lib.ptr(h.packed()), lib.ptr(folded), None, None, lib.ptr(o), lib.ptr(d), lib.ptr(z), S, None,
                                          None, R, S, lib.ptr(ws), lib.ptr(raw), lib.ptr(tp), mk.data_ptr() if mk is not None else None, lib.ptr(vb),
                                          None, st), "net_forward")
        torch.cuda.synchronize()
        assert torch.equal(raw_m, raw_t)
        masks[fused] = mask.clone()
        # the bits against the fp32 tape: word 4 b + c, bit l  <->  float 256 b + 4 l + c   (Mp x tape_cols floats, valid rows only matter
        # downstream, but the padding rows are written by both forms too)
        t = (tape.reshape(-1, 64, 4) > 0)                                         # [block, lane, comp]
        bits = (mask.reshape(-1, 4)[:, None, :] >> torch.arange(64, device=DEV)[None, :, None]) & 1
        assert torch.equal(bits.bool(), t)
        for mode in ("mask", "tape"):
            h.force_fp32_tape = mode == "tape"
            og, dg = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
            fo, vbg = folded.clone().requires_grad_(True), vb.clone().requires_grad_(True)
            raw = NetFn.apply(h, og, dg, z, S, S, fo, vbg, None)
            (raw * G).sum().backward()
            grads[(fused, mode)] = [t_.grad.clone() for t_ in (og, dg, fo, vbg)]
        h.force_fp32_tape = False
    assert torch.equal(masks["0"], masks["1"])
    ref = grads[("0", "tape")]
    for k, g in grads.items():
        for a_, b_ in zip(g, ref):
            assert torch.equal(a_, b_), k


@pytest.mark.parametrize("D,W,R,S", [(10, 1024, 70, 128), (8, 512, 33, 64)])
def test_wide_first_layer_through_encoding_panels_is_bit_identical(D, W, R, S, knob):
    """Widths >= 512: the first layer's encoding features are computed once into panels (`mofa_pe_panels`) and the layer runs as a
    K = 64 launch of the pipelined kernel, instead of every feature-tile workgroup regenerating them (k_layer<.., L0>).  MOFA_PIPE=0
    keeps the generated-operand kernel (and the plain loops): the whole network — inference and tape — must agree bit for bit."""
    from mofanerf_amd.autograd import NetFn, view_bias_torch
    from mofanerf_amd.hipnet import HipNet
    from mofanerf_amd.model import NeRF
    rng = np.random.default_rng(D + W)
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, 1))
    h = HipNet(net.to(DEV))
    o = dev(rng.uniform(-2, 2, (R, 3)).astype(np.float32))
    d = dev(rng.normal(0, 0.3, (R, 3)).astype(np.float32))
    z = dev(np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1))
    vd = torch.nn.functional.normalize(d, dim=-1).contiguous()
    bm, tex, e = synth.codes(3)
    folded = h.fold(e.to(DEV), bm.to(DEV), tex.to(DEV)).clone()
    outs, tapes = {}, {}
    for mode in ("0", "1"):
        knob("MOFA_PIPE", mode)
        raw = torch.full((R, S, 4), float("nan"), device=DEV)
        h.forward_rays(o, d, z, S, vd, S, raw, folded)
        outs[mode] = raw.clone()
        with torch.enable_grad():
            tapes[mode] = NetFn.apply(h, o, d, z, S, S, folded, view_bias_torch(h, vd).detach(), None).detach().clone()
        torch.cuda.synchronize()
    assert torch.equal(outs["0"], outs["1"]) and torch.isfinite(outs["1"]).all()
    assert torch.equal(tapes["0"], tapes["1"])
    nan_equal_close(tapes["1"].cpu().numpy(), outs["1"].cpu().numpy(), 2e-5)      # (tape mode takes torch's per-ray view-bias rows)



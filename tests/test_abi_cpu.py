"""CPU-side checks of the C ABI: the library loads without a GPU and exports every symbol the header declares;
argument validation returns MOFA_EINVAL with a message (no compute is launched)."""
import ctypes
import os
import re

from mofanerf_amd import build, lib, schema

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "mofanerf_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mofa_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    so = build.build()
    L = ctypes.CDLL(so)
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/mofanerf_hip.h but not exported"
    assert sorted(lib.SIGNATURES) == syms, "python binding and header disagree"


def test_library_exports_nothing_but_the_declared_abi():
    """Built with -fvisibility=hidden: the dynamic symbol table holds exactly the functions of include/mofanerf_hip.h — no
    mofa_internal_* hand-offs between translation units, no measurement entry points (those live in build_arms/libmofanerf_measure.so,
    tools/build_measure.py), and the product sources carry no measurement arms."""
    import subprocess
    so = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    funcs = sorted(l.split()[-1] for l in out.splitlines() if l.split()[1] in ("T", "W"))
    assert funcs == header_symbols(), sorted(set(funcs) ^ set(header_symbols()))
    csrc = os.path.join(ROOT, "mofanerf_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")):
            src = open(os.path.join(csrc, f)).read()
            for arm in ("MOFA_TIMELINE", "MOFA_ABLATE", "MOFA_SPLIT_FAKE", "MOFA_SETPRIO", "k_layer_persist", "k_layer_ring3", "k_mfma_peak_probe", "k_mfma_valu_probe", "k_layer_split", "MOFA_GEMM"):
                assert arm not in src, (f, arm)


def test_plan_sizes_and_argument_validation():
    L = lib.load()
    assert L.mofa_abi_version() == 5 == lib.ABI_VERSION
    for D, W in ((8, 256), (10, 1024), (8, 64)):
        s = lib.NetShape(D, W)
        assert L.mofa_net_num_layers(s) == 2 * D + 7 == len(schema.nerf_layers(D, W))
        Wp, Hp = (W + 63) // 64 * 64, (W // 2 + 63) // 64 * 64
        n_plain = 3 + 4 + 4 + 2 * (D - 6)
        want = Wp * 64 + n_plain * Wp * Wp + 2 * Wp * Wp + 2 * Wp * 2 * Wp + Hp * Wp + Wp + 3 * Hp
        assert want <= L.mofa_net_packed_floats(s) <= want + 64 * (2 * D + 7)
        assert L.mofa_net_folded_floats(s) == (2 * D + 4) * Wp + 8
        # four activation buffers, the per-ray bias rows, and k_net_chain's queue state (8 heads x 32 words, 32 status words, a counter per row tile, 32 spare)
        assert L.mofa_net_workspace_floats(s, 1000, 10) == 4 * 1024 * Wp + 10 * Hp + 64 + (8 * 32 + 32 + 1024 // 256 + 32)
        assert L.mofa_net_mask_tape_words(s, 1000) * 64 == L.mofa_net_tape_floats(s, 1000)      # one bit per tape float
        # the two backward forms keep different buffers — fitting three more gradient buffers (its chained backward's bias-gradient
        # inputs), training (round 6, widths the chained training backward takes) the partial sums of every weight gradient of one launch
        fit_ws, train_ws = L.mofa_net_backward_workspace_floats(s, 1000, 0), L.mofa_net_backward_workspace_floats(s, 1000, 1)
        one = L.mofa_weight_grad_workspace_floats(1000, Wp, Wp)
        assert fit_ws - train_ws == 3 * 1024 * Wp, (fit_ws, train_ws)
        if Wp % 256 == 0:           # opt-in MOFA_CHAIN_TRAIN=1: the scratch then holds every weight gradient's partial sums of one chained launch
            import os as _os
            _os.environ["MOFA_CHAIN_TRAIN"] = "1"
            lib.reload_env()
            try:
                splits = 4                                               # 4 row tiles, one per XCD range, one split each
                assert one == splits * Wp * (Wp + 1)
                chained = L.mofa_net_backward_workspace_floats(s, 1000, 1)
                assert chained - (train_ws - one) == (D + 4) * ((splits * Wp * (Wp + 1) + 63) // 64 * 64), (chained, train_ws)
            finally:
                del _os.environ["MOFA_CHAIN_TRAIN"]
                lib.reload_env()
    assert L.mofa_net_num_layers(lib.NetShape(3, 256)) == -1
    assert L.mofa_net_num_layers(lib.NetShape(8, 256, pe_point_freqs=17)) == -1
    assert L.mofa_net_num_layers(lib.NetShape(8, 256, ch_tex=-1)) == -1
    assert L.mofa_layer_forward(None, 16, None, 0, None, None, 0, 1, None, 256, 64, 1, None) == -1
    assert b"null pointer" in L.mofa_last_error()
    assert L.mofa_composite_forward(1, 1, 0, 1, None, 4, 1, 0, 1, 1, 1, 1, 1, None) == -1
    assert b"S >= 2" in L.mofa_last_error()
    assert L.mofa_sample_pdf_merge(1, 0, 1, 1, 0, 4, 5000, 5000, 1, 1, 1, None) == -1      # 3 S + Ni floats of LDS per ray: 64 KiB
    assert b"3 S + Ni" in L.mofa_last_error()
    assert L.mofa_composite_backward(1, 1, 0, 1, None, 4, 20000, 0, 1, None, None, None, None, 1, None, None) == -1
    assert L.mofa_layer0_forward(1, 1, 1, 0, None, 4, 1, 99, 1, 1, 1, 256, 64, None, None) == -1
    assert b"n_freqs" in L.mofa_last_error()
    assert [L.mofa_pe_k_padded(f) for f in (0, 6, 10, 11, 16, 17)] == [64, 64, 64, 128, 128, -1]


def test_plan_follows_every_reference_flag():
    """MofaNetShape carries multires / multires_views / the three code widths (tools/config_parser.py:51-56,113-118): the layer shapes
    the C plan assumes equal the reference module's for ANY setting (schema.nerf_layers restates models/model.py:80-114)."""
    import ctypes as C
    L = lib.load()
    no, ni = C.c_int32(), C.c_int32()
    for D, W, mr, mv, ce, cs, ct in ((8, 64, 6, 2, 6, 80, 256), (10, 128, 0, 0, 30, 50, 64), (8, 256, 16, 16, 0, 0, 0), (8, 256, 10, 4, 30, 50, 256)):
        s = lib.NetShape(D, W, mr, mv, ce, cs, ct)
        want = list(schema.nerf_layers(D, W, ch_pts=3 + 6 * mr + ce, ch_shape=cs, ch_tex=ct, ch_views=3 + 6 * mv).values())
        assert L.mofa_net_num_layers(s) == len(want)
        for li, (o, i) in enumerate(want):
            assert L.mofa_net_layer_dims(s, li, C.byref(no), C.byref(ni)) == 0 and (no.value, ni.value) == (o, i), (s, li)
        assert L.mofa_net_layer_dims(s, len(want), C.byref(no), C.byref(ni)) == -1


def test_hipnet_refuses_a_module_the_plan_does_not_describe():
    """VERDICT r3 'boundary hole': NeRF(input_ch=81) (multires=8) used to be accepted and mis-read with the shipped 63/30 split.
    Now the shape is DERIVED from the module + the renderer's embedder, checked against every Linear, and anything else is refused."""
    import pytest
    import torch
    from mofanerf_amd import factory
    from mofanerf_amd.hipnet import HipNet
    from mofanerf_amd.model import NeRF
    mk = lambda **k: NeRF(**{**dict(D=8, W=64, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50,
                                    use_viewdirs=True), **k})
    h = HipNet(mk(input_ch=81), point_freqs=8)                       # multires = 8 -> 51 + 30
    assert (h.shape.pe_point_freqs, h.shape.ch_exp) == (8, 30)
    h = HipNet(mk(input_ch=81))                                      # fed by the shipped 63-wide encoding: 63 + 18, also a valid network
    assert (h.shape.pe_point_freqs, h.shape.ch_exp) == (10, 18)
    h = HipNet(mk(input_ch_views=15, input_ch_shapeCodes=80, input_ch_textureCodes=64))
    assert (h.shape.pe_view_freqs, h.shape.ch_shape, h.shape.ch_tex) == (2, 80, 64)
    with pytest.raises(lib.MofaError, match="narrower than the point encoding"):
        HipNet(mk(input_ch=45))                                      # 39 + 6 fed by a 63-wide encoding
    with pytest.raises(lib.MofaError, match="not a positional-encoding width"):
        HipNet(mk(input_ch_views=16))
    bad = mk()
    bad.linear_BiM_xyz.linears1.Linear0 = torch.nn.Linear(64 + 80, 64)         # a module edited after construction
    with pytest.raises(lib.MofaError, match="refusing to pack"):
        HipNet(bad)
    # the renderer hands its embedder's frequency count to the plan; create_nerf builds both from the same flags
    args = factory.default_args(netdepth=8, netwidth=64, netdepth_fine=8, netwidth_fine=64, multires=6, multires_views=2,
                                input_ch_textureCodes=128, no_reload=True, device="cpu", basedir="/nonexistent")
    _, kw, _, _, _, _, render = factory.create_nerf(args)
    assert (render.point_freqs, render.view_freqs) == (6, 2)
    h = render._hip(kw["network_fn"])
    assert (h.shape.pe_point_freqs, h.shape.pe_view_freqs, h.shape.ch_exp, h.shape.ch_shape, h.shape.ch_tex) == (6, 2, 30, 50, 128)
    render.view_freqs = 4
    for _ in range(2):                                               # refused every time, not only on the first call
        with pytest.raises(lib.MofaError, match="embeddirs_fn encodes 4"):
            render._hip(kw["network_fn"])
    with pytest.raises(lib.MofaError, match="must come from mofanerf_amd.embedder.get_embedder"):
        type(render)(embed_fn=lambda x: x)


def test_profiler_kinds_agree_between_header_binding_and_bench():
    """mofa_prof_end fills arrays of MOFA_PROF_KINDS entries: the header, the ctypes binding and bench.py's kernel table must agree
    (a shorter array on the Python side would be overrun by the library)."""
    import re, sys
    hdr = open(os.path.join(ROOT, "include", "mofanerf_hip.h")).read()
    n = int(re.search(r"#define MOFA_PROF_KINDS (\d+)", hdr).group(1))
    sys.path.insert(0, ROOT)
    import bench
    assert n == lib.PROF_KINDS == len(bench.KERNELS) == 12 and bench.KERNELS[11][0] == "mofa::k_net_chain_train" and 11 in bench.MFMA_KINDS
    assert bench.KERNELS[5][0] == "mofa::k_net_chain<0>" and bench.KERNELS[6][0] == "mofa::k_net_chain<2>" and bench.KERNELS[1][0] == "mofa::k_mlp_fused"
    # the mask-writing chained forward is its own kind (the fit line named <0> while <1> ran); the HBM-bound ray kernels follow
    assert bench.KERNELS[7][0] == "mofa::k_net_chain<1>" and [k[0] for k in bench.KERNELS[8:11]] == ["mofa::k_composite<1>", "mofa::k_composite<2>",
                                                                                                   "mofa::k_sample_pdf_merge<false>"]
    assert set(bench.HBM_KINDS) == {8, 9, 10} and all(bench.HBM_KINDS[k] > 1000 for k in bench.HBM_KINDS)


def test_failure_hooks_are_an_entry_point_not_environment_variables():
    """the two hooks that force k_net_chain's failure paths (and the self-check's mismatch) are set through
    mofa_test_hooks() only — the built library no longer even contains the names of the round-5 environment variables."""
    L = lib.load()
    assert L.mofa_test_hooks(0, -1, 0) == 0 and L.mofa_test_hooks(7, 3, 1) == 0 and L.mofa_test_hooks(0, -1, 0) == 0
    assert L.mofa_test_hooks(0, 8, 0) == -1 and b"chain_skip_xcd" in L.mofa_last_error()
    assert L.mofa_test_hooks(0, -2, 0) == -1
    blob = open(build.build(), "rb").read()
    for name in (b"MOFA_CHAIN_SPIN_LIMIT", b"MOFA_CHAIN_TEST_SKIP_XCD"):
        assert name not in blob, name
    for name in (b"MOFA_PIPE", b"MOFA_FUSED", b"MOFA_CHAIN", b"MOFA_CHAIN_TRAIN"):   # the knobs that choose between bit-identical forms are still read
        assert name in blob, name


def test_product_never_imports_the_oracle():
    """The product package must not reach into oracle/ (nor any CPU fallback): grep the sources."""
    pkg = os.path.join(ROOT, "mofanerf_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "mofa_oracle" not in src and "from oracle" not in src and "import oracle" not in src, f


def test_hot_kernels_fit_their_occupancy_without_scratch():
    """ISA-level regression guard, read from the built library's own code objects (tools/kernel_resources.py; no GPU needed): the MFMA
    kernels are written for TWO workgroups per CU (<= 256 registers per lane in the unified VGPR file) and must not touch scratch —
    a compiler or source change that spills them would halve the matrix pipe's feed long before any parity test noticed."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rs = {r["kernel"]: r for r in kernel_resources.resources(build.build())}
    hot = [k for k in rs if k.startswith(("mofa::k_layer<", "mofa::k_mlp_fused", "mofa::k_wgrad<", "mofa::k_net_chain"))]
    assert len(hot) >= 18 and all(f"mofa::k_net_chain<{m}>" in hot for m in (0, 1, 2)), sorted(rs)
    for k in hot:
        r = rs[k]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 256, (k, r)
    # the chained launch keeps 512 workgroups resident (two per CU): its registers AND its scalar state must leave room for that — an
    # in-kernel queue-adoption variant that reached 100 SGPRs measured 1.6 % slower (profiles/r04_ab_chain.txt)
    for m in (0, 1, 2):        # forward / forward + mask tape / backward-data
        chain = rs[f"mofa::k_net_chain<{m}>"]
        assert chain["vgpr"] <= 240 and chain["sgpr"] <= 100 and chain["sgpr_spill"] == 0, chain
    # the chained training backward holds TWO tile forms (backward-data tile + weight-gradient unit): no scratch, two workgroups per CU; its
    # scalar state overflows into vector lanes at the tile boundaries (v_writelane / v_readlane, not memory) — bounded here
    train = rs["mofa::k_net_chain_train"]
    # (250 vector registers since the K loops carry their LDS-DMA requests' lane offsets in registers of their own; the limit is the 256 of
    #  two workgroups per CU)
    assert train["vgpr"] <= 252 and train["scratch"] == 0 and train["sgpr_spill"] <= 48, train
    dom = rs["mofa::k_layer<128, false, false, false, true, mofa::ShippedPolicy>"]
    assert dom["vgpr"] <= 200 and dom["agpr"] == 0, dom            # 197 since round 2; the refactor into mofa_layer.h + policy did not move it
    for k, r in rs.items():                                        # the ray-side kernels run many rays per CU: keep them light
        if k.startswith(("mofa::k_composite", "mofa::k_sample_pdf_merge", "mofa::k_get_rays")):
            assert r["vgpr"] <= 128 and r["scratch"] == 0, (k, r)


def test_inline_asm_writelanes_keep_the_valu_sgpr_wait_states(tmp_path):
    """ISA-level guard for a hazard hipcc does not cover inside inline asm (round 5: 26 GPU tests failed on it).  On gfx90a+ a VALU that
    READS an SGPR needs two wait states after the VALU that WROTE it; the mask-tape writers move `v_cmp` ballots into lanes with
    `v_writelane_b32` from inline asm (mofa_layer.h, mask_ballots), so the wait states are ours to provide (`s_nop 1` with the ballots as
    operands).  Compile the product's network TU to assembly (no GPU needed) and check every v_writelane that takes an SGPR: none of the two
    instruction slots before it may be a v_cmp writing that SGPR."""
    import re
    import subprocess
    asm = tmp_path / "mlp.s"
    subprocess.run([build.hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fvisibility=hidden", "-S", "--cuda-device-only",
                    "-o", str(asm), os.path.join(build.CSRC, "mofa_mlp.hip")], check=True, capture_output=True)
    lines = [l.strip() for l in asm.read_text().split("\n")]
    lines = [l for l in lines if l and not l.startswith((";", ".")) and not l.endswith(":")]

    def covers(dst, src):          # does the v_cmp destination `dst` ("vcc", "s[10:11]") contain the 32-bit register `src` ("vcc_lo", "s11")?
        if dst.startswith("vcc"):
            return src.startswith("vcc")
        m = re.match(r"s\[(\d+):(\d+)\]", dst)
        return bool(m) and src.startswith("s") and src[1:].isdigit() and int(m.group(1)) <= int(src[1:]) <= int(m.group(2))

    total = hazards = 0
    for i, l in enumerate(lines):
        m = re.match(r"v_writelane_b32 v\d+, (s\d+|vcc_lo|vcc_hi), \d+", l)
        if not m:
            continue
        total += 1
        ws, j = 0, i - 1
        while j >= 0 and ws < 2:
            p = lines[j]
            if p.startswith("s_nop"):
                ws += int(p.split()[1]) + 1
            else:
                if p.startswith("v_cmp") and covers(p.split()[1].rstrip(","), m.group(1)):
                    hazards += 1
                    break
                ws += 1
            j -= 1
    assert total >= 64, total            # the mask writers are there (16 ballots x 2 halves per 4 KiB slice, several instantiations)
    assert hazards == 0, hazards


def test_weight_gradient_split_plan_partitions_the_row_tiles():
    """`wg_split` (csrc/mofa_common.h) — ONE plan of how the weight gradient splits its contraction over the points, shared by the per-layer
    kernel and the chained training backward: whole row tiles, never straddling the row ranges k_net_chain gives the eight XCDs, every row tile
    in exactly one split.  Restated here and tied to the library through the workspace size it implies (splits x N x (K + 1) floats)."""
    L = lib.load()

    from bwd_reference import wg_plan      # the restatement, shared with the weight-gradient tests (tests/test_gpu_bwd_kernels.py)

    def plan(n_points, n_padded, k_padded):
        p = wg_plan(n_points, n_padded, k_padded)
        mpx, m_tiles, rows = p["mpx"], p["m_tiles"], []
        for s, (first, count) in enumerate(p["splits"]):
            end = first + count
            assert first // mpx == (end - 1) // mpx == s // p["nspx"], "a split straddles two XCD ranges"
            rows += list(range(first, end))
        assert rows == list(range(m_tiles)), (n_points, n_padded, k_padded)     # every row tile exactly once, in order
        return p["total"]

    for n_points in (1, 255, 257, 1344, 4096, 131072, 196608, 196609, 524288, 300 * 64):
        for n_padded, k_padded in ((1024, 1024), (512, 1024), (256, 256), (128, 256), (1024, 64), (64, 64), (768, 768)):
            assert L.mofa_weight_grad_workspace_floats(n_points, n_padded, k_padded) == plan(n_points, n_padded, k_padded) * n_padded * (k_padded + 1), \
                (n_points, n_padded, k_padded)
    assert plan(196608, 1024, 1024) == 32 and plan(196608, 512, 1024) == 64 and plan(196608, 256, 256) == 384      # the benchmark's training sub-batch


def test_the_hot_k_loops_carry_no_vector_address_arithmetic():
    """ISA-level regression guard (tools/kloop_census.py; no GPU needed).  On gfx950 a vector instruction between two MFMAs costs the
    matrix pipe 6-13 cycles whatever it computes (profiles/r06_probe_dual_issue.md), and hipcc, left to itself, forms every LDS-DMA
    request's address with 64-bit vector adds inside the MFMA stream.  Round 6 took them out (profiles/r06_ab_kloop_addr.md: +1.3 % on the
    headline, +3.2 % on the persistent kernel, +2.0 % on a training step): the K loops of the chained and the persistent kernels hold NO
    vector instruction but their MFMAs, the pipelined per-layer loops only the weight requests' four adds (which measure faster there than
    the scalar-base form), the weight gradient's loop no 64-bit address arithmetic.  A compiler or source change that brings them back fails
    here, not as a silent 1-3 % in the next benchmark."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kloop_census
    c = kloop_census.census(build.build())
    for m in (0, 1, 2):
        (loop,) = c[f"mofa::k_net_chain<{m}>"]
        assert loop["mfma"] == 128 and loop["vmem"] == 12 and loop["vector"] == 0, loop
    for mask in ("false", "true"):
        loops = [l for l in c[f"mofa::k_mlp_fused<{mask}>"] if l["vmem"] > 0]            # the two pipelined loops (layer 0's loop requests nothing)
        assert sorted(l["mfma"] for l in loops) == [64, 128] and all(l["vector"] == 0 for l in loops), loops
    for k, loops in c.items():
        if k.startswith("mofa::k_layer<128,") and k.endswith("true, mofa::ShippedPolicy>"):                  # PIPE = true
            (loop,) = loops
            assert loop["mfma"] == 128 and loop["vector_ops"] == {"v_lshl_add_u64": 4}, (k, loop)
    main = max(c["mofa::k_wgrad<128, 256>"], key=lambda l: l["mfma"])
    assert main["mfma"] == 128 and not any(op.startswith(("v_lshl_add_u64", "v_cmp")) for op in main["vector_ops"]), main
    assert set(main["vector_ops"]) <= {"v_pk_add_f32", "v_add_u32_e32"}, main      # the bias sums (one wave in eight, behind a scalar branch) + 4 LDS address adds


def test_the_backward_epilogue_requests_its_mask_one_slice_ahead():
    """ISA-level regression guard for round 6's last kernel change (profiles/r06_ab_bwd_epilogue.md; no GPU needed).  The backward-data epilogue
    walks a wave's tile in eight 4 KiB slices; it used to request each slice's ReLU mask at the top of the slice and wait for it with
    `s_waitcnt vmcnt(0)` — eight exposed global round trips per tile — and to apply a mask bit with two 64-bit ands, a 64-bit compare and a select.
    Now the next slice's mask is in flight while the current slice goes through the LDS window, the bits arrive as ONE dword per lane and word and
    are applied as `value & v_bfe_i32(word, lane & 31, 1)`.  In the shipped code object of the chained backward-data kernel that reads: 128 sign-extending
    bit-field extracts per epilogue form (the plain and the accumulating form keep the old one: it runs on two of 26 products), no 64-bit compare in the
    plain form's share, and waits that leave more than a slice's requests in flight."""
    import re
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kloop_census
    kernels = {name: ins for name, ins, _ in kloop_census.disassemble(build.build())}
    ins = kernels["mofa::k_net_chain<2>"]
    ops = [op for op, _ in ins]
    assert ops.count("v_bfe_i32") == 128, ops.count("v_bfe_i32")                      # 8 slices x 16 values of the mask-bit form
    assert ops.count("v_cmp_ne_u64_e32") <= 128                                       # only chain_store_bwd_acc's (the accumulating form) are left
    waits = [int(m.group(1)) for op, args in ins if op == "s_waitcnt" for m in [re.search(r"vmcnt\((\d+)\)", args)] if m]
    assert sum(1 for w in waits if w >= 16) >= 16, sorted(set(waits))                # waits with a whole slice's 16 dword requests still in flight

"""The premise of the sigma-gated forward, on the CPU with the oracle and the committed golden fixtures: a sample whose raw density is
<= 0 has alpha 0 and weight 0 exactly, so zeroing its colour changes no bit of any composited output.  Plus what can be said about the
native entry point without a GPU: it is declared everywhere, refuses bad arguments, and its launch path never waits for the device."""
import os
import re

import numpy as np
import torch

from mofanerf_amd import lib
from oracle import mofa_oracle as orc

T = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def test_zeroing_the_colour_of_dead_samples_changes_no_composited_bit(golden):
    g = golden("kat.npz")
    for S in (64, 128):
        raw, z, d = T(g[f"r2o{S}_raw"]), T(g[f"r2o{S}_z"]), T(g[f"r2o{S}_d"])
        dead = raw[..., 3] <= 0
        assert 0 < int(dead.sum()) < dead.numel()                      # the fixture has both kinds
        gated = raw.clone()
        gated[..., :3][dead] = 0.0
        assert not torch.equal(gated, raw)
        for wb in (False, True):
            full = orc.raw2outputs(raw, z, d, None, wb)
            out = orc.raw2outputs(gated, z, d, None, wb)
            for name, a, b in zip(("rgb", "disp", "acc", "weights", "depth"), out, full):
                if name == "disp":
                    assert _same(a, b) and torch.isnan(b).any(), name  # equal, NaN pattern included (the zero-opacity ray)
                else:
                    assert torch.equal(a, b), (S, wb, name)
            assert (full[3][dead] == 0).all()                          # every dead sample's weight is exactly 0


def test_the_gated_entry_is_declared_everywhere_and_refuses_bad_calls():
    hdr = open(os.path.join(ROOT, "include", "mofanerf_hip.h")).read()
    for name in ("mofa_net_forward_gated", "mofa_net_forward_gated_workspace_floats"):
        assert re.search(r"\b%s\(" % name, hdr) and name in lib.SIGNATURES
    assert "#define MOFA_ABI_VERSION 5" in hdr and lib.ABI_VERSION == 5
    L = lib.load()
    s = lib.NetShape(10, 1024)
    n, r = 196608, 1536
    base, gated = L.mofa_net_workspace_floats(s, n, r), L.mofa_net_forward_gated_workspace_floats(s, n, r)
    # a call that can gate (a device whose census allows the chained launch) needs, behind the ordinary workspace: per-point bias rows
    # [Mp, Hp], the compacted rgb [Mp, 4], the 64-bit scan [Mp], flags, counts, queue state; a call that cannot needs nothing more
    assert gated == base or base + n * 512 + n * 4 + n * 2 + n // 4 + 64 <= gated < base + n * 512 + n * 8
    narrow = lib.NetShape(8, 256)                                      # the persistent kernel's width: never gated
    assert L.mofa_net_forward_gated_workspace_floats(narrow, n, r) == L.mofa_net_workspace_floats(narrow, n, r)
    os.environ["MOFA_GATE"] = "0"
    try:
        lib.reload_env()
        assert L.mofa_net_forward_gated_workspace_floats(s, n, r) == base
    finally:
        del os.environ["MOFA_GATE"]
        lib.reload_env()
    assert L.mofa_net_forward_gated_workspace_floats(s, 0, 1) == 0
    import ctypes as C
    route = C.c_int32(-1)
    assert L.mofa_net_forward_gated(s, None, None, None, None, None, None, None, 0, None, None, 1, 1, None, None, None, None, None, None,
                                    None) == -1
    assert L.mofa_net_forward_gated(s, 16, 16, 16, 16, None, None, None, 0, None, 16, 1, 1, 16, 16, None, None, C.byref(route), None,
                                    None) == -1 and route.value == 0
    assert b"need pts or" in L.mofa_last_error()


def test_the_gated_launch_path_never_waits_for_the_device():
    """The live count stays on the device: between the two chained launches there is no stream synchronisation, no blocking copy, no
    allocation — read off the source of the gated branch and of the kernels it adds."""
    src = open(os.path.join(ROOT, "mofanerf_amd", "csrc", "mofa_net.hip")).read()
    body = src[src.index("// The sigma-gated forward: the geometry half"):src.index("} else if (chain_ok()) {")]
    kernels = src[src.index("// ---- the sigma-gated forward (mofa_net_forward_gated)"):src.index("#define MOFA_SHAPE_FMT")]
    assert "mofa_internal_chain_launch_live" in body and "k_gate_scatter" in body
    for text in (body, kernels):
        for word in ("Synchronize", "hipMemcpy", "hipMalloc", "hipFree", "hipEvent", "getenv"):
            assert word not in text, word
    assert b"MOFA_GATE" in open(lib.LIB_PATH, "rb").read()

"""The occupancy pass (mofa_occ_classify / _gather / _scatter / _scatter_sigma) on PRESCRIBED kept patterns: every mask of
tests/compact_reference.py's catalogue, plus the first two sizes at which the 64-bit scan grows a level (2048^2 samples: one second-level
tile; 2048^2 + 1: two, hence a third level), and the occupancy pass feeding the sigma gate on a partly occupied grid at chain-capable
widths.  tests/test_gpu_occ.py draws its cells at random and stops at 111 K samples.

A prescribed pattern: a sample is kept iff its point lies inside an all-occupied grid, so with d = 0 the origin alone — inside the
lattice or far outside it — decides each ray's flags, for any finite z."""
import numpy as np
import pytest
import torch

import compact_reference as cr
from harness import make_product
from mofanerf_amd import lib, mesh
from test_gpu_gate import _shipped_launch_forms, fine  # noqa: F401  (autouse: the shipped launch forms, MOFA_GATE and MOFA_STREAMS included)
from test_gpu_occ import _classify, ball_occupancy, frame, scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
RES, LO, STEP = mesh.grid_spec(((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), (9, 9, 9))
LEVEL2 = 2048 * 2048            # samples: 2048 scan tiles of 2048, one tile at the second level
BIG = [(LEVEL2, LEVEL2 // 3, "random"), (LEVEL2 + 1, LEVEL2 // 2 + 5, "random")]


def i32(t):
    return t.contiguous().view(torch.int32)


def run_pass(ray_mask, S, z_mode, seed=0):
    """R rays x S samples against the all-occupied grid, ray r kept iff ray_mask[r]; every output compared on the device."""
    L = lib.load()
    R = int(ray_mask.shape[0])
    n = R * S
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    keep_ray = torch.from_numpy(ray_mask).to(DEV)
    o = (1.8 * torch.rand(R, 3, device=DEV, generator=g) - 0.9)
    o[:, 0] += torch.where(keep_ray, 0.0, 5.0)                                # dead rays: x in [4.1, 5.9], the lattice ends at 1
    o = o.contiguous()
    d = torch.zeros(R, 3, device=DEV)
    vd = torch.randn(R, 3, device=DEV, generator=g)
    if z_mode == "per_ray":
        z, zs = 8.0 + 18.0 * torch.rand(R, S, device=DEV, generator=g), S
    else:
        z, zs = torch.linspace(8.0, 26.0, S, device=DEV), 0
    cells = torch.ones(RES[0] - 1, RES[1] - 1, RES[2] - 1, dtype=torch.uint8, device=DEV)
    flags, ws, n_kept, pts, dirs, index = _classify(o, d, vd, z, zs, S, cells, RES, LO, STEP)
    want = keep_ray[:, None].expand(R, S).reshape(-1)
    e = torch.nonzero(want).reshape(-1)                                       # ascending: np.flatnonzero's order
    assert torch.equal(flags.reshape(-1), want.to(torch.uint8))
    assert n_kept == int(ray_mask.sum()) * S == e.numel()
    assert torch.equal(index, e.to(torch.int32))
    assert torch.equal(i32(pts), i32(o[e // S])) and torch.equal(i32(dirs), i32(vd[e // S]))
    for width, entry in ((4, L.mofa_occ_scatter), (1, L.mofa_occ_scatter_sigma)):
        kept = torch.randn(n_kept, width, device=DEV, generator=g)
        kept[::7] = -0.0                                                      # (a kept -0 stays -0: rows are moved, not recomputed)
        out = torch.full((n, width), NAN, device=DEV)
        lib.check(entry(lib.ptr(kept) if n_kept else None, flags.data_ptr(), ws.data_ptr(), n, n_kept, lib.ptr(out), lib.stream()), "mofa_occ_scatter*")
        full = torch.zeros(n, width, device=DEV)
        full[e] = kept
        assert torch.equal(i32(out), i32(full)), width                        # every element written: kept rows in place, +0 elsewhere
    torch.cuda.synchronize()
    return n_kept


# ---- a. the catalogue masks, one sample per ray ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", cr.CATALOGUE, ids=lambda e: f"{e[0]}-{e[1]}-{e[2]}")
@pytest.mark.parametrize("z_mode", ["per_ray", "shared"])
def test_every_catalogue_mask_is_classified_compacted_and_scattered_exactly(entry, z_mode):
    M, L, arrangement = entry
    assert run_pass(cr.mask(M, L, arrangement), 1, z_mode) == L


@pytest.mark.parametrize("entry", BIG, ids=lambda e: f"{e[0]}-{e[1]}-{e[2]}")
def test_a_seeded_mask_at_the_sizes_where_the_scan_grows_a_level(entry):
    M, L, arrangement = entry
    assert run_pass(cr.mask(M, L, arrangement, seed=9), 1, "per_ray", seed=2) == L


def test_the_big_sizes_are_where_the_scan_grows_a_level():
    """2048 samples per scan tile: 2048^2 samples are 2048 first-level sums — one second-level tile, no third level — and one sample
    more makes two second-level sums, which need a third-level scan (scan_exclusive recurses while a level has more than one tile)."""
    L = lib.load()
    tiles = lambda n: (n + 2047) // 2048

    def levels(n):
        return 1 if tiles(n) == 1 else 1 + levels(tiles(n))

    assert [levels(n) for n in (2048, 2049, 111000, LEVEL2, LEVEL2 + 1)] == [1, 2, 2, 2, 3]
    aux = lambda n: (L.mofa_occ_workspace_bytes(n) - (n * 8 + 255) // 256 * 256) // 8        # elements of scan scratch behind the scan itself
    assert aux(LEVEL2) >= 2048 + 2048 + 1 and aux(LEVEL2 + 1) >= 2049 + 2049 + 2 + 2 + 1


# ---- b. several samples per ray ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z_mode", ["per_ray", "shared"])
def test_per_ray_flags_at_37_samples_a_ray(z_mode):
    M, L, arrangement = 2049, 257, "random"
    assert (M, L, arrangement) in cr.CATALOGUE
    assert run_pass(cr.mask(M, L, arrangement), 37, z_mode, seed=1) == 257 * 37


# ---- c. the occupancy pass feeding the sigma gate --------------------------------------------------------------------------------------------
def _same(a, b, nan_aware):
    if nan_aware:
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    return torch.equal(a, b)


@pytest.mark.parametrize("W", [512, 1024])
def test_a_culled_frame_is_the_same_with_and_without_the_gate_on_a_partly_occupied_grid(W, knob):
    """Culled rendering hands the gate explicit points with S = 1; on the ball grid only part of each pass is kept, and of the kept fine
    samples only part is live: MOFA_GATE=1 against MOFA_GATE=0, every returned tensor."""
    render, kw, _ = make_product((8, 64, 10, W), 0, 4096, DEV)
    K, ro, rd = scene(16)
    grid, _, _ = ball_occupancy(dilate=1)
    knob("MOFA_GATE", "0")
    ref = frame(render, kw, K, ro, rd, occupancy=grid, verbose=True)
    h = fine(render, kw)
    assert h.last_gated in (None, 0) and render.gate_stats(reset=True).get((h.D, h.W), {"samples": 0})["samples"] == 0
    knob("MOFA_GATE", "1")
    out = frame(render, kw, K, ro, rd, occupancy=grid, verbose=True)
    occ_stats = {k: dict(v) for k, v in render.occupancy_stats.items()}
    st = render.gate_stats(reset=True)[(h.D, h.W)]
    print("occupancy + gate", W, occ_stats, st)
    assert h.last_gated == 1
    assert 0 < occ_stats["fine"]["kept"] < occ_stats["fine"]["samples"] == 256 * 128
    assert st["samples"] == occ_stats["fine"]["kept"] and 0 < st["live"] < st["samples"]
    for a, b in zip(out[:3], ref[:3]):
        assert _same(a, b, True)
    assert out[3].keys() == ref[3].keys() and {"rgb0", "acc0", "disp0", "z_std", "_z_fine", "_weights0"} <= out[3].keys()
    for k in out[3]:
        if torch.is_tensor(out[3][k]):
            assert _same(out[3][k], ref[3][k], k.startswith("disp")), k
    assert float(out[2].max()) > 0

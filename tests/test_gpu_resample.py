"""The resampler on the GPU (``k_sample_pdf_merge`` behind ``mofa_sample_pdf_merge`` and ``mofa_sample_pdf``), sample by sample, on the
batches of tests/pdf_reference.py: the seams of the 64-wide cdf scan, the 4 / 2 / 1 rays-per-block boundaries up to the 4096 + 4096 limit,
ray counts that fill no block, shared and per-ray rows, threshold bins entered on purpose, ``searchsorted`` ties, NaN rays, and rays whose
sorted ``u`` gives samples with one adjacent pair out of order by an ulp (the general merge pass with finite numbers; the pair placed
inside, across and behind a 64-lane stride of the kernel's sorted-run check and at the row's end).

* ``z_samples`` equals the bit-level restatement BIT FOR BIT (NaN meeting NaN), and ``mofa_sample_pdf`` on the mid-point bins gives the
  same bits.  The library is built with -ffp-contract=off and correctly rounded division and takes its sums in fp64; every batch row's
  rounded sums are the same in any association (``pdf_reference.decided``), so nothing is left open.
* every finite ray's samples lie inside the fp64 window written from the specification — independent of the restatement;
* ``z_fine`` equals the stable, NaN-last sort of ``cat(z, the kernel's own samples)`` bit for bit, in a buffer pre-filled with -7 (no
  position is negative): a slot left unwritten shows.  A ray with one inverted pair must come out sorted: a sorted-run check that missed
  the pair would merge it by binary search and leave the pair in its order.  Before the general merge pass ranked NaN after every
  number, a NaN ray left slots ``S .. S + Ni - 1`` unwritten and raced on slot 0;
* ``z_std`` is within one fp32 ulp of the fp64 population standard deviation of the kernel's samples, 0 for Ni = 1, NaN for a NaN ray;
* one sentinel row behind each output is untouched, and two runs give identical bytes.

No tolerance here comes from the code under test.  Worst err / tolerance of the window per batch on the MI355X (printed by
``test_finite_rays_lie_inside_the_window``; the bits being equal, the restatement's own figure on the CPU is the same): 0.156 over the 91
batches — 0.000 to 0.114 at 4 + 1 and 5 + 2, 0.068 to 0.156 for every shape from 65 + 64 to 4096 + 4096, 0.077 to 0.149 for the
recorded rays, 0.057 to 0.141 for the rays over several binades.  On its first run the file found that a lone NaN sample (Ni = 1)
passed the kernel's sorted-run check and was written over slot 0; the NaN-ray test fails on the library before these changes (slot 0 NaN, one slot left at -7) and passes on this one."""
import numpy as np
import pytest
import torch

import pdf_reference as ref
from mofanerf_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
SENTINEL = -7.0                                                       # positions are positive; NaN is a possible output, so it cannot mark a slot


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_merge(b):
    """(z_samples [R+1, Ni], z_fine [R+1, S+Ni], z_std [R+1]) as NumPy: the last row of each is a sentinel row behind the output."""
    R, S, Ni = b["R"], b["S"], b["Ni"]
    z, w, u = dev(b["z"]), dev(b["w"]), dev(b["u"])
    zs, zf, sd = (torch.full(sh, SENTINEL, dtype=torch.float32, device=DEV) for sh in ((R + 1, Ni), (R + 1, S + Ni), (R + 1,)))
    lib.check(lib.load().mofa_sample_pdf_merge(lib.ptr(z), S if b["z"].ndim == 2 else 0, lib.ptr(w), lib.ptr(u), Ni if b["u"].ndim == 2 else 0,
                                               R, S, Ni, lib.ptr(zs), lib.ptr(zf), lib.ptr(sd), lib.stream()), "mofa_sample_pdf_merge")
    torch.cuda.synchronize()
    return zs.cpu().numpy(), zf.cpu().numpy(), sd.cpu().numpy()


def run_plain(b):
    R, S, Ni = b["R"], b["S"], b["Ni"]
    bins, w, u = dev(ref.midpoints(b["z"])), dev(b["w"][:, 1:S - 1]), dev(b["u"])
    out = torch.full((R + 1, Ni), SENTINEL, dtype=torch.float32, device=DEV)
    lib.check(lib.load().mofa_sample_pdf(lib.ptr(bins), S - 1 if b["z"].ndim == 2 else 0, lib.ptr(w), lib.ptr(u), Ni if b["u"].ndim == 2 else 0,
                                         R, S - 1, Ni, lib.ptr(out), lib.stream()), "mofa_sample_pdf")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def runs():
    """Every batch through the library once: name -> dict(first, second: the merge form twice; plain: the bins form)."""
    return {b["name"]: dict(first=run_merge(b), second=run_merge(b), plain=run_plain(b)) for b in ref.batches()}


def test_z_samples_equal_the_restatement_bit_for_bit(runs):
    for b in ref.batches():
        zs = runs[b["name"]]["first"][0][:-1]
        want = ref.reference(b)["samples"]
        assert ref.same_bits(np.isnan(zs), np.isnan(want)), b["name"]
        n = ref.bits_differing(np.nan_to_num(zs, nan=0.0), np.nan_to_num(want, nan=0.0))
        assert n == 0, (b["name"], n, float(np.nanmax(np.abs(zs - want))))
        for p in ("only_w0", "only_wlast"):                            # the exterior weights are not read
            if "zero" in b["patterns"] and p in b["patterns"]:
                assert ref.same_bits(zs[b["patterns"].index(p)], zs[b["patterns"].index("zero")]), (b["name"], p)


def test_the_bins_form_gives_the_bits_of_the_merge_form(runs):
    for b in ref.batches():
        r = runs[b["name"]]
        assert ref.same_bits(r["plain"][:-1], r["first"][0][:-1]), b["name"]
        assert np.all(r["plain"][-1] == F(SENTINEL)), b["name"]


def test_finite_rays_lie_inside_the_window(runs):
    worst = 0.0
    for b in ref.batches():
        S, R = b["S"], b["R"]
        fin = ref.finite_rows(b)
        zs = runs[b["name"]]["first"][0][:-1]
        ratio = ref.window_ratio(ref.midpoints(ref.rows_of(b["z"], R))[fin], b["w"][fin][:, 1:S - 1], ref.rows_of(b["u"], R)[fin], zs[fin])
        top = float(ratio.max()) if ratio.size else 0.0
        print(f"{b['name']:50s} worst err / tolerance {top:.3f}")
        assert (ratio <= 1).all(), (b["name"], int((ratio > 1).sum()), top)
        worst = max(worst, top)
    print(f"worst over all batches: {worst:.3f}")


def test_z_fine_is_the_stable_nan_last_sort_of_the_kernels_own_samples(runs):
    for b in ref.batches():
        zs, zf, _ = runs[b["name"]]["first"]
        want = ref.merge(b["z"], zs[:-1])
        assert ref.same_bits(zf[:-1], want), (b["name"], ref.bits_differing(np.nan_to_num(zf[:-1], nan=-1.0), np.nan_to_num(want, nan=-1.0)))


def test_a_ray_with_one_inverted_pair_comes_out_sorted(runs):
    """Sorted u, finite samples, ONE adjacent pair out of order by an ulp: the kernel's own samples show the pair where the batch placed it
    (elements 62 .. 65 of the S + Ni positions: inside, across and behind a 64-lane stride of the sorted-run check; and the row's end), and
    z_fine is non-decreasing all the same — the check saw the pair and the ray took the general pass."""
    seen = 0
    for b in ref.batches():
        if "placed" not in b:
            continue
        zs, zf, _ = runs[b["name"]]["first"]
        assert [ref.inversions(x).tolist() for x in zs[:-1]] == [[j] for j in b["placed"]], b["name"]
        assert np.all(zf[:-1, :-1] <= zf[:-1, 1:]), b["name"]
        seen += b["R"]
    assert seen == 4 * len(ref.INVERSION_SEEDS)


def test_a_nan_ray_fills_every_slot_with_its_nans_last(runs):
    """A NaN interior weight makes every new sample NaN: z_fine is the S coarse positions in order, then Ni NaNs — no slot keeps the fill."""
    seen = 0
    for b in ref.batches():
        zs, zf, _ = runs[b["name"]]["first"]
        z = ref.rows_of(b["z"], b["R"])
        for r in np.flatnonzero(~ref.finite_rows(b)):
            assert np.isnan(zs[r]).all(), b["name"]
            assert ref.same_bits(zf[r, :b["S"]], np.ascontiguousarray(z[r])) and np.isnan(zf[r, b["S"]:]).all(), (b["name"], int(r), int((zf[r] == F(SENTINEL)).sum()))
            seen += 1
    assert seen >= 2 * len(ref.SEAMS)


def test_z_std_is_within_an_ulp_of_fp64(runs):
    for b in ref.batches():
        zs, _, sd = runs[b["name"]]["first"]
        fin = ref.finite_rows(b)
        assert ref.std_within_an_ulp(sd[:-1], ref.z_std(zs[:-1])).all(), b["name"]
        assert np.isnan(sd[:-1][~fin]).all() and np.isfinite(sd[:-1][fin]).all(), b["name"]
        if b["Ni"] == 1:
            assert ref.same_bits(sd[:-1][fin], np.zeros(int(fin.sum()), F)), b["name"]


def test_nothing_is_written_behind_the_outputs_and_two_runs_give_the_same_bytes(runs):
    for b in ref.batches():
        r = runs[b["name"]]
        for first, second in zip(r["first"], r["second"]):
            assert np.all(first[-1] == F(SENTINEL)), b["name"]
            assert ref.same_bits(first, second), b["name"]

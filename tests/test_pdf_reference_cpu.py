"""The two statements of tests/pdf_reference.py checked on their own, without a GPU: the bit-level restatement, the fp32 torch oracle, the
reference's recorded samples and the recorded ``sample_pdf`` vectors all lie inside the fp64 window; the batches meet the conditions the
GPU tests rely on (every rounded sum decided, every merge path taken — the general pass from sorted ``u`` by rays with one inverted pair —, the 1e-5 branch entered); and each wrong variant — a ``searchsorted``
from the left, the exterior weights read, the 1e-5 branch missing or taken on ``<=``, the scan's carry dropped, ``above`` not clamped, the
coarse positions for the mid-points, a neighbour's ``u`` row, a ray index off by one block, Ni - 1 in the spread, a merge that loses a tie, a merge that takes every ray for sorted —
is SEEN by the comparison the GPU tests use: the bits always, the window wherever the variant leaves it.  Run with ``-s`` for the counts.

Counts on the batches (samples whose bits change / samples outside the window, of 115,079 finite ones): see ``test_each_fault...``; it
prints them.  ``le_branch`` differs from the specification only where ``den == 1e-5f`` exactly, inside the ``2 eps`` band in which the
window admits both branches, so it is a bits-only fault; ``fp32_cdf`` is the legitimate variant held to its own window."""
import numpy as np
import pytest
import torch

import pdf_reference as ref
from oracle import mofa_oracle as orc

F = np.float32


def window_of(b, samples, rows=None, eps=ref.EPS):
    S, R = b["S"], b["R"]
    rows = ref.finite_rows(b) if rows is None else rows
    return ref.window_ratio(ref.midpoints(ref.rows_of(b["z"], R))[rows], b["w"][rows][:, 1:S - 1], ref.rows_of(b["u"], R)[rows], samples[rows], eps)


def test_the_batches_meet_their_conditions():
    """No undecided row; the shapes and ray counts asked for; per aimed batch the sorted merge, the general merge from unsorted u and
    >= 5 % unit-branch samples; in the batches over several binades also the general merge from SORTED u, by exactly one inverted pair."""
    bs = ref.batches()
    shapes = {(b["S"], b["Ni"]) for b in bs}
    assert set(ref.SEAMS) | set(ref.BLOCKS) <= shapes
    assert [ref.rays_per_block(*s) for s in ref.BLOCKS] == [4, 2, 2, 1, 1] and 3 * 4096 + 4096 == ref.LDS_FLOATS
    for S, Ni in ref.SEAMS:
        assert {1, 2, 3, 5, 9} <= {b["R"] for b in bs if (b["S"], b["Ni"]) == (S, Ni)}
    assert all(b["R"] == 3 for b in bs if (b["S"], b["Ni"]) in ref.BLOCKS[-3:])
    general_from_sorted_u = third_path_batches = 0
    for b in bs:
        S, R = b["S"], b["R"]
        assert ref.decided(b["w"][:, 1:S - 1]).all(), b["name"]
        z = ref.rows_of(b["z"], R)
        assert np.all(z[:, :-1] <= z[:, 1:]), b["name"]                 # the coarse run is always sorted: the samples decide the merge path
        r = ref.reference(b)
        u = ref.rows_of(b["u"], R)
        u_sorted = np.all(u[:, :-1] <= u[:, 1:], -1)
        general_from_sorted_u += int((u_sorted & ~r["sorted"]).sum())
        if b.get("third_path"):                                         # finite samples from sorted u with ONE adjacent pair out of order
            third = np.flatnonzero(u_sorted & ~r["sorted"] & ref.finite_rows(b))
            assert third.size >= 1 and all(ref.inversions(r["samples"][i]).size == 1 for i in third), b["name"]
            third_path_batches += 1
            if "placed" in b:                                          # ... at the element of the ray's S + Ni positions it was placed at
                assert third.size == R and [int(ref.inversions(x)[0]) for x in r["samples"]] == list(b["placed"]), b["name"]
                assert {S + j for j in b["placed"][:3]} == {62, 63, 64}
        assert np.isnan(r["samples"][~ref.finite_rows(b)]).all() and np.isfinite(r["samples"][ref.finite_rows(b)]).all()
        if b["aimed"]:
            assert r["unit"].mean() >= 0.05, (b["name"], r["unit"].mean())
            if b["Ni"] >= 2:
                assert r["sorted"].any() and (~r["sorted"] & ~u_sorted).any(), b["name"]
        if "zero" in b["patterns"]:                                    # w[0] and w[S-1] are not read
            for p in ("only_w0", "only_wlast"):
                if p in b["patterns"]:
                    assert ref.same_bits(r["samples"][b["patterns"].index(p)], r["samples"][b["patterns"].index("zero")]), (b["name"], p)
    assert general_from_sorted_u >= len(ref.SEAMS)                      # NaN rays under linspace u
    assert third_path_batches == 2 * len(ref.INVERSION_SEEDS)
    thr = [b for b in bs if "threshold" in b["patterns"] and b["aimed"]]
    assert thr and all((ref.cdf_bits(b["w"][:, 1:b["S"] - 1])[b["patterns"].index("threshold"), 1] == ref.TINY) for b in thr)


def test_where_sorted_u_gives_unsorted_samples():
    """A record of where the third merge path lies, not a property of the resampler: among 2,000 aimed rays with the positions of this
    model's cameras (8 to 26, neighbouring bin edges within a factor 2) none has an inverted pair.  Over several binades about one
    in 5,000 does: ``pdf_reference.inversion_batches`` holds four, and ``test_the_batches_meet_their_conditions`` asserts that they are there."""
    found, looked_at = ref.search_sorted_u_unsorted_samples(2000)
    print(f"positions in 8 .. 26: rays with sorted u and unsorted samples: {found} of {looked_at}")
    assert found == 0 and looked_at >= 2000


def test_restatement_and_oracle_lie_inside_the_window_on_every_batch():
    worst = {"restatement": 0.0, "oracle": 0.0}
    n = 0
    for b in ref.batches():
        S, R = b["S"], b["R"]
        fin = ref.finite_rows(b)
        z = torch.from_numpy(np.ascontiguousarray(ref.rows_of(b["z"], R)))
        o = orc.sample_pdf(.5 * (z[:, 1:] + z[:, :-1]), torch.from_numpy(b["w"][:, 1:S - 1].copy()), torch.from_numpy(b["u"].copy())).numpy()
        for who, s in (("restatement", ref.reference(b)["samples"]), ("oracle", o)):
            ratio = window_of(b, s)
            assert (ratio <= 1).all(), (b["name"], who, int((ratio > 1).sum()), float(ratio.max()))
            worst[who] = max(worst[who], float(ratio.max()) if ratio.size else 0.0)
        n += int(fin.sum()) * b["Ni"]
    print(f"{n} finite samples; worst err / tolerance: {worst}")


def test_recorded_samples_lie_inside_the_window(golden):
    n = 0
    for fx in ("e2e_small.npz", "e2e_true.npz", "e2e_long.npz"):
        g = golden(fx)
        zc, wc, zs = g["z_coarse"], g["weights_coarse"], g["z_samples"]
        u = np.linspace(0.0, 1.0, zs.shape[1], dtype=F)               # perturb = 0: the deterministic u (run_nerf_helpers.py:212)
        ratio = ref.window_ratio(ref.midpoints(zc), wc[:, 1:-1], u, zs)
        mine = ref.resample(zc, wc, u)[0]
        print(f"{fx}: {zs.size} recorded samples, worst err / tolerance {ratio.max():.3f}, {ref.bits_differing(mine, zs)} differ in bits from the "
              f"restatement, by up to {np.abs(mine - zs).max():.2e}")
        assert (ratio <= 1).all(), (fx, int((ratio > 1).sum()))
        assert (ref.window_ratio(ref.midpoints(zc), wc[:, 1:-1], u, mine) <= 1).all()
        n += zs.size
    assert n == 28_112
    g = golden("kat.npz")
    np.random.seed(0)
    u_rand = np.random.rand(g["spdf_bins"].shape[0], 64).astype(F)
    for u, key in ((np.linspace(0.0, 1.0, 64, dtype=F), "spdf_det"), (u_rand, "spdf_rand")):
        ratio = ref.window_ratio(g["spdf_bins"], g["spdf_w"], u, g[key])
        assert (ratio <= 1).all(), (key, int((ratio > 1).sum()))
    a_bins, a_w = np.linspace(8, 26, 7, dtype=F)[None], F([[0, .1, .6, .2, .05, 0]])
    assert (ref.window_ratio(a_bins, a_w, np.linspace(0.0, 1.0, 8, dtype=F), g["spdf_anchor"]) <= 1).all()


def test_merge_and_std_restatements():
    for b in ref.batches():
        s = ref.reference(b)["samples"]
        z = ref.rows_of(b["z"], b["R"])
        both = np.concatenate([z, s], -1)
        m = ref.merge(b["z"], s)
        assert ref.same_bits(m, np.sort(both, -1)) and ref.same_bits(m, torch.sort(torch.from_numpy(both), stable=True, dim=-1)[0].numpy()), b["name"]
        want = torch.std(torch.from_numpy(s.copy()).double(), -1, unbiased=False).numpy()
        got = ref.z_std(s)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12, equal_nan=True), b["name"]
        if b["Ni"] == 1:
            assert np.all(got[ref.finite_rows(b)] == 0)
    v = F([[3, np.nan, 1, -0.0, 1, np.nan, 0.0, 2]])                    # ties in index order (-0 before +0 here), NaN last
    assert ref.same_bits(ref.merge(v[:, :3], v[:, 3:]), F([[-0.0, 0.0, 1, 1, 2, 3, np.nan, np.nan]]))
    assert ref.std_within_an_ulp(F([1.0, np.nan, 1.0]), np.float64([1.0 + 2.0 ** -24, np.nan, 1.0 + 2.0 ** -22])).tolist() == [True, True, False]


def test_round_f32_and_decided():
    from fractions import Fraction
    rng = np.random.default_rng(8)
    for x in rng.uniform(1e-9, 4, 300):
        N = int(x * 2 ** 60) * (1 << 30) + int(rng.integers(1 << 30))
        r, exact = ref._round_f32(N, -90), Fraction(N, 1 << 90)
        assert float(F(r)) == r                                        # a float32, and no neighbour is nearer
        assert all(abs(Fraction(r) - exact) <= abs(Fraction(float(np.nextafter(F(r), F(d)))) - exact) for d in (-np.inf, np.inf))
    assert ref._round_f32((1 << 24) + 1, 0) == float(1 << 24) and ref._round_f32((1 << 24) + 3, 0) == float((1 << 24) + 4)    # ties to even
    assert ref._round_f32((1 << 25) + 2, -3) == float(1 << 22) and ref._round_f32((1 << 25) + 3, -3) == float((1 << 22) + 0.5)
    assert ref.decided(np.zeros((1, 62), F))[0]
    # a prefix within 2^-60 of a rounding boundary: two associations of the fp64 sum may round it to different floats
    tie = F([1.0, 2.0 ** -24, 2.0 ** -60])
    assert not ref._sums_decided(tie) and ref._sums_decided(tie[:2])   # exactly on the boundary every association is exact: decided
    assert ref.decided(F([[np.nan, 1.0]]))[0]


FAULTS = ref.FAULTS_SAMPLE + ref.FAULTS_STD + ref.FAULTS_MERGE
BITS_ONLY = {"left": "it differs at a tie u == cdf_k alone, where the window admits the reading of either neighbouring bin",
             "le_branch": "den == 1e-5f lies inside the 2 eps band where the window admits both branches",
             "fp32_cdf": "a legitimate accumulation; held to the (k + 3) 2^-24 window instead",
             "unbiased": "z_std is compared with fp64 within an ulp, not through the window",
             "drop_tie": "the merge is compared bit for bit, not through the window",
             "assume_sorted": "the merge is compared bit for bit, not through the window"}


def test_each_fault_changes_bits_and_each_violation_leaves_the_window():
    counts = {}
    for fault in FAULTS:
        bits = outside = wide = 0
        for b in ref.batches():
            good = ref.reference(b)["samples"]
            fin = ref.finite_rows(b)
            if fault in ref.FAULTS_SAMPLE:
                bad = ref.resample(b["z"], b["w"], b["u"], fault=fault)[0]
                bits += ref.bits_differing(good, bad)
                if fault == "ray_shift":                               # a NaN ray's samples on a finite ray (or the reverse) are outside
                    outside += int((np.isnan(bad) != np.isnan(good)).sum())
                    fin = fin & np.isfinite(bad).all(-1)
                outside += int((window_of(b, bad, fin) > 1).sum())
                if fault == "fp32_cdf":
                    wide += int((window_of(b, bad, fin, eps=lambda k: (k + 3) * 2.0 ** -24) > 1).sum())
            elif fault == "unbiased":
                bits += int((~ref.std_within_an_ulp(ref.z_std(good, fault=fault).astype(F), ref.z_std(good))).sum())
            else:
                bits += ref.bits_differing(ref.merge(b["z"], good), ref.merge(b["z"], good, fault=fault, fill=-1.0))
        counts[fault] = (bits, outside)
        print(f"{fault:12s} bits changed: {bits:7d}   outside the window: {outside:7d}" + (f"   outside its own (k + 3) 2^-24 window: {wide}" if fault == "fp32_cdf" else "")
              + (f"   [{BITS_ONLY[fault]}]" if fault in BITS_ONLY else ""))
        if fault == "fp32_cdf":
            assert wide == 0
    for fault, (bits, outside) in counts.items():
        assert bits > 0, fault
        assert outside > 0 or fault in BITS_ONLY, fault
    assert counts["le_branch"][1] == 0


def test_a_missed_inverted_pair_is_seen_at_every_place():
    """A sorted-run check that misses the one inverted pair leaves the pair in its order: on each row of the placed batches the merge
    differs from the stable sort, so the bit-for-bit comparison of z_fine sees a check that is blind at any one of those elements."""
    rows = 0
    for b in ref.batches():
        if "placed" in b:
            s = ref.reference(b)["samples"]
            good, bad = ref.merge(b["z"], s), ref.merge(b["z"], s, fault="assume_sorted", fill=-1.0)
            assert all(ref.bits_differing(g, x) > 0 for g, x in zip(good, bad)), b["name"]
            rows += b["R"]
    assert rows == 4 * len(ref.INVERSION_SEEDS)


def test_each_scan_seam_is_seen():
    """The carry lost at ONE seam alone (64, 128 or 192; every other chunk keeps its carry) changes the cdf in that chunk only, and the
    bits of the samples, at every shape whose S - 2 bin weights reach past that seam."""
    seen = set()
    for S, Ni in ((67, 65), (131, 128), (257, 200)):
        b = next(x for x in ref.batches() if (x["S"], x["Ni"]) == (S, Ni) and x["name"].endswith("all patterns, linspace u"))
        fin = ref.finite_rows(b)
        w = b["w"][fin][:, 1:S - 1]
        good = ref.cdf_bits(w)
        for seam in range(64, S - 2, 64):
            bad = ref.cdf_bits(w, fault=f"carry@{seam}")
            there = slice(seam + 1, seam + 65)                         # cdf_k is the sum of the first k entries
            assert ref.bits_differing(good[:, there], bad[:, there]) > 0, (S, Ni, seam)
            keep = np.ones(good.shape[1], bool)
            keep[there] = False
            assert ref.same_bits(good[:, keep], bad[:, keep]), (S, Ni, seam)
            n = ref.bits_differing(ref.reference(b)["samples"][fin], ref.resample(b["z"], b["w"], b["u"], fault=f"carry@{seam}")[0][fin])
            print(f"{S}+{Ni}: carry lost at {seam}: {n} samples change bits")
            assert n > 0, (S, Ni, seam)
            seen.add(seam)
    assert seen == {64, 128, 192}

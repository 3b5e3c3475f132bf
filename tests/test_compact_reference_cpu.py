"""tests/compact_reference.py on the CPU: the helpers against NumPy's own primitives and hand-written values, and the catalogue, taken
as a whole, against the list of cases the GPU tests of the sigma gate and of the occupancy pass exist to reach."""
import numpy as np
import pytest

import compact_reference as cr

M0 = 17 * 256 + 3


def _f32_bits(*values):
    return np.array(values, dtype=np.float32).view(np.uint32)


def test_live_rule_on_the_special_values():
    tiny = np.array([1], dtype=np.uint32).view(np.float32)[0]                # the smallest denormal, 2^-149
    flt_min = np.float32(np.finfo(np.float32).tiny)
    values = [np.float32(0.0), np.float32(-0.0), tiny, -tiny, flt_min, np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)]
    want = [False, False, True, False, True, True, False, True]
    bits = _f32_bits(*values)
    assert bits[0] == 0 and bits[1] == 0x80000000 and bits[2] == 1 and bits[3] == 0x80000001 and bits[4] == 0x00800000
    assert cr.live_rule(bits).tolist() == want
    assert cr.live_rule(bits.view(np.int32)).tolist() == want and cr.live_rule(bits.view(np.float32)).tolist() == want
    # every NaN, quiet or signalling, of either sign, is live; the rule is "not (x <= 0)" wherever a float compare is trustworthy
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff], dtype=np.uint32)
    assert cr.live_rule(nans).all()
    rng = np.random.default_rng(0)
    some = rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)
    x = some.view(np.float32)
    normal = (some & 0x7f800000) != 0                                        # (a host that flushes denormals would compare them as zero)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(cr.live_rule(some)[normal], ~(x <= 0)[normal])
    assert cr.live_rule(np.zeros((3, 2), np.uint32)).shape == (3, 2)


@pytest.mark.parametrize("arrangement", cr.ARRANGEMENTS)
def test_mask_has_exactly_l_rows_where_the_arrangement_says(arrangement):
    for M in (1, 7, 255, 256, 257, 1000, M0):
        last0 = 256 * ((M + 255) // 256 - 1)
        room = M - last0 if arrangement == "last_tile_only" else M
        for L in sorted({0, 1, min(5, room), room // 2, room - 1 if room > 1 else 0, room}):
            m = cr.mask(M, L, arrangement, seed=3)
            e = np.flatnonzero(m)
            assert m.dtype == bool and m.shape == (M,) and len(e) == L == cr.n_live(m)
            if arrangement == "first":
                assert np.array_equal(e, np.arange(L))
            elif arrangement == "last":
                assert np.array_equal(e, np.arange(M - L, M))
            elif arrangement == "alternate" and L <= (M + 1) // 2:
                assert np.array_equal(e, 2 * np.arange(L))
            elif arrangement == "blocks4" and L <= 4 * (M // 8):
                assert np.array_equal(e, 8 * (np.arange(L) // 4) + np.arange(L) % 4)
            elif arrangement == "last_tile_only":
                assert np.array_equal(e, last0 + np.arange(L))
            elif arrangement == "random":
                assert np.array_equal(m, cr.mask(M, L, arrangement, seed=3))
                if 0 < L < M and M > 200:
                    assert not np.array_equal(m, cr.mask(M, L, arrangement, seed=4))
        with pytest.raises(ValueError):
            cr.mask(M, room + 1, arrangement)
    with pytest.raises(ValueError):
        cr.mask(10, 3, "middle")


def test_scan_counts_and_tiles_against_numpy():
    rng = np.random.default_rng(1)
    for M in (1, 2, 255, 256, 257, 5000):
        for p in (0.0, 0.3, 1.0):
            m = rng.uniform(size=M) < p
            s = cr.scan(m)
            assert s.dtype == np.int64 and np.array_equal(s, np.cumsum(m) - m)
            e = np.flatnonzero(m)
            assert np.array_equal(s[e], np.arange(len(e)))                   # a live row's slot: ascending and complete
            assert cr.n_live(m) == len(e) == (int(s[-1]) + int(m[-1]))       # (what k_gate_count and k_occ_total read)
            assert cr.live_tiles(m) == -(-len(e) // 256)
    assert [cr.row_tiles(n) for n in (0, 1, 255, 256, 257, 512, 513)] == [0, 1, 1, 1, 2, 2, 3]
    assert cr.xcd_split(0) == [0] * 8 and cr.xcd_split(1) == [1, 0, 0, 0, 0, 0, 0, 0] and cr.xcd_split(7) == [1] * 7 + [0]
    assert cr.xcd_split(8) == [1] * 8 and cr.xcd_split(9) == [2, 2, 2, 2, 1, 0, 0, 0] and cr.xcd_split(15) == [2] * 7 + [1]
    assert cr.xcd_split(16) == [2] * 8 and cr.xcd_split(17) == [3, 3, 3, 3, 3, 2, 0, 0] and cr.xcd_split(18) == [3] * 6 + [0, 0]
    assert all(sum(cr.xcd_split(t)) == t for t in range(0, 200))


def test_swizzle_pairs_by_hand():
    assert cr.swizzle_pairs(np.zeros(40, bool)) == set()
    assert cr.swizzle_pairs(np.ones(40, bool)) == {(0, 0), (1, 1), (2, 2), (3, 3)}             # the identity never crosses quads
    m = np.zeros(40, bool)
    m[[5, 13, 14]] = True                                                                      # rows 5, 13, 14 -> slots 0, 1, 2
    assert cr.swizzle_pairs(m) == {(1, 0), (3, 0)}
    m = np.zeros(64, bool)
    m[4:12] = True                                                                             # rows 4 .. 11 -> slots 0 .. 7
    assert cr.swizzle_pairs(m) == {(1, 0), (2, 1)}
    alt = cr.mask(64, 32, "alternate")                                                         # row 2 j -> slot j
    assert cr.swizzle_pairs(alt) == {((j >> 1) & 3, (j >> 2) & 3) for j in range(32)}


def test_expected_raw_on_six_rows():
    nan = np.float32(np.nan)
    full = np.array([[1, 2, 3, 0.5], [4, 5, 6, -1.0], [7, 8, 9, 0.0], [-1, -2, -3, nan], [nan, 1, 1, -0.0], [0.25, 0.5, 0.75, np.inf]], np.float32)
    m = cr.live_rule(full[:, 3])
    assert m.tolist() == [True, False, False, True, False, True]
    want = np.array([[1, 2, 3, 0.5], [0, 0, 0, -1.0], [0, 0, 0, 0.0], [-1, -2, -3, nan], [0, 0, 0, -0.0], [0.25, 0.5, 0.75, np.inf]], np.float32)
    got = cr.expected_raw(full, m)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))          # bits: -0 stays -0 in sigma, a dead NaN colour becomes +0
    assert got is not full and np.array_equal(full[1], np.float32([4, 5, 6, -1.0]))
    assert np.array_equal(cr.expected_raw(full, np.ones(6, bool)).view(np.uint32), full.view(np.uint32))
    with pytest.raises(AssertionError):
        cr.expected_raw(full, m[:5])


def test_the_catalogue_reaches_every_case_the_gpu_tests_are_for():
    cat = cr.CATALOGUE
    assert 25 <= len(cat) <= 35 and len(set(cat)) == len(cat)
    masks = [cr.mask(M, L, a) for M, L, a in cat]
    for (M, L, a), m in zip(cat, masks):
        assert a in cr.ARRANGEMENTS and m.shape == (M,) and cr.n_live(m) == L
    assert M0 == cr.M0 == 4355 and cr.row_tiles(M0) == 18 and M0 % 256 == 3
    at_m0 = {cr.live_tiles(m) for (M, _, _), m in zip(cat, masks) if M == M0}
    assert at_m0 >= {0, 1, 2, 7, 8, 9, 15, 16, 17, 18}
    assert {L for M, L, _ in cat if M == M0} >= {0, 1, 255, 256, 257, 512, M0 - 1, M0}
    assert {M for M, _, _ in cat} >= {1, 255, 256, 257, 2048, 2049, 4355}
    pairs = set().union(*(cr.swizzle_pairs(m) for m in masks))
    assert pairs == {(a, b) for a in range(4) for b in range(4)}
    assert any(cr.swizzle_pairs(m) == pairs for m in masks)                    # and one entry alone moves rows between all 16
    assert any(a == "last_tile_only" and L == 1 for _, L, a in cat)
    assert any(L % 256 == 0 and 0 < L < M for M, L, _ in cat)                  # a live count at a tile boundary, neither 0 nor M
    assert {a for _, _, a in cat} == set(cr.ARRANGEMENTS)
    # what the GPU files pick out of it by name
    assert (M0, M0, "first") in cat and (M0, 1, "last_tile_only") in cat and any(M == M0 and L == 257 for M, L, _ in cat)
    assert any(M % 37 == 0 for M, _, _ in cat) and any(M % 128 == 0 for M, _, _ in cat)

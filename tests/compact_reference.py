"""NumPy restatement of run-time compaction — the sigma gate (mofa_net_forward_gated: k_gate_flags / k_gate_count / k_gate_gather /
k_gate_scatter in mofa_net.hip) and the occupancy pass (mofa_occ_classify / _gather / _scatter in mofa_occ.hip), both on the 64-bit
exclusive scan of mofa_mesh.hip — and the catalogue of PRESCRIBED live patterns that tests/test_gpu_gate_patterns.py and
tests/test_gpu_occ_patterns.py run.

  live       a raw density is live iff it is NOT <= 0: stated here on the fp32 bit pattern, without a float compare
  slot       live row e goes to row j = scan[e], the exclusive scan of the flags: ascending and complete
  row tiles  the colour half runs over ceil(n_live / 256) row tiles, split ceil(live_tiles / 8) to each of the eight XCD queues
  swizzle    a panel row carries the quad swizzle (row / 4) % 4; the gather moves quad c ^ se of row e to quad c ^ sj of row j
  raw        sigma everywhere, rgb of the full forward on the live rows, rgb exactly +0 on the dead ones
"""
import numpy as np

ROW_TILE = 256                  # kRowTile
ARRANGEMENTS = ("first", "last", "alternate", "blocks4", "random", "last_tile_only")


def live_rule(bits):
    """bool, same shape: is the fp32 value with this bit pattern live?  NaN is live; otherwise the sign bit is clear and the magnitude
    bits are not all zero: +denormal, +inf are live; +0, -0, every negative value, -inf are dead."""
    u = np.asarray(bits)
    if u.dtype != np.uint32:
        assert u.dtype in (np.int32, np.float32), u.dtype
        u = u.view(np.uint32)
    mag = u & np.uint32(0x7fffffff)
    nan = mag > np.uint32(0x7f800000)
    return nan | (((u >> np.uint32(31)) == 0) & (mag != 0))


def row_tiles(n):
    return (int(n) + ROW_TILE - 1) // ROW_TILE


def _order(M, arrangement, seed):
    """The rows of a batch of M in the order an arrangement makes them live."""
    rows = np.arange(M, dtype=np.int64)
    if arrangement == "first":
        return rows
    if arrangement == "last":
        return rows[::-1]
    if arrangement == "alternate":                       # rows 0, 2, 4, ...; the odd rows only once every even row is live
        return np.concatenate([rows[0::2], rows[1::2]])
    if arrangement == "blocks4":                         # runs of four rows: 0-3, 8-11, ...; the runs between only once those are live
        even = (rows // 4) % 2 == 0
        return np.concatenate([rows[even], rows[~even]])
    if arrangement == "random":
        return np.random.default_rng(seed).permutation(M).astype(np.int64)
    if arrangement == "last_tile_only":                  # nothing before the last (possibly ragged) row tile
        return rows[ROW_TILE * (row_tiles(M) - 1):]
    raise ValueError(f"arrangement {arrangement!r}: want one of {ARRANGEMENTS}")


def mask(M, L, arrangement, seed=0):
    """bool [M] with exactly L true entries."""
    M, L = int(M), int(L)
    order = _order(M, arrangement, seed)
    if M < 1 or L < 0 or L > len(order):
        raise ValueError(f"mask: L = {L} live rows of M = {M} do not fit arrangement {arrangement!r} ({len(order)} rows to choose from)")
    m = np.zeros(M, dtype=bool)
    m[order[:L]] = True
    return m


def scan(m):
    """Exclusive scan of the flags, int64 [M]: the slot of row e if it is live."""
    m = np.asarray(m, dtype=bool)
    out = np.zeros(m.shape[0], dtype=np.int64)
    run = 0
    for e in range(m.shape[0]):
        out[e] = run
        run += int(m[e])
    return out


def n_live(m):
    return int(np.count_nonzero(np.asarray(m, dtype=bool)))


def live_tiles(m):
    return row_tiles(n_live(m))


def xcd_split(tiles):
    """Row tiles each of the eight XCD queues of a chained launch gets: ceil(tiles / 8) each until none are left."""
    per = (int(tiles) + 7) // 8
    return [max(0, min(per, int(tiles) - x * per)) for x in range(8)]


def swizzle_pairs(m):
    """The set of (se, sj) = ((e / 4) % 4, (scan[e] / 4) % 4) over the live rows e: what the gather's quad move sees."""
    m = np.asarray(m, dtype=bool)
    e = np.flatnonzero(m)
    j = np.arange(len(e), dtype=np.int64)                # scan[e] of the live rows, in ascending order
    return set(zip(((e >> 2) & 3).tolist(), ((j >> 2) & 3).tolist()))


def expected_raw(full_raw, m):
    """What the gated forward must leave in raw [M,4], from the full forward's raw: sigma everywhere, rgb on the live rows, +0 on the dead."""
    full = np.asarray(full_raw, dtype=np.float32)
    m = np.asarray(m, dtype=bool).reshape(-1)
    assert full.ndim == 2 and full.shape == (m.shape[0], 4), (full.shape, m.shape)
    out = full.copy()
    out[~m, :3] = np.float32(0.0)
    return out


M0 = 17 * ROW_TILE + 3          # 4355 rows: 18 row tiles, the last one ragged (3 rows)

# (M, L, arrangement): every GPU test of the gate and of the occupancy pass runs all of them (seed 0).
CATALOGUE = [
    # M0: every queue occupancy of the eight XCDs — 0, 1, 2, 7, 8, 9, 15, 16, 17, 18 live row tiles — and the counts at a tile boundary
    (M0, 0, "first"),                    # 0 tiles: nothing to gather, the colour launch has no work
    (M0, 1, "last_tile_only"),           # 1 tile, its one row the FIRST of the ragged tile (row 4352 -> slot 0)
    (M0, 1, "first"),
    (M0, 255, "random"),                 # 1 tile, one row short of full
    (M0, 256, "alternate"),              # 1 tile, exactly full
    (M0, 257, "blocks4"),                # 2 tiles, one row in the second
    (M0, 512, "random"),                 # 2 tiles, exactly full
    (M0, 1792, "random"),                # 7 tiles, exact: one per queue, the eighth queue empty
    (M0, 2048, "alternate"),             # 8 tiles, exact: one per queue
    (M0, 2049, "blocks4"),               # 9 tiles: two per queue, three queues empty
    (M0, 3840, "random"),                # 15 tiles, exact
    (M0, 3841, "random"),                # 16 tiles
    (M0, 4096, "last"),                  # 16 tiles, exact: every row moves down by 259
    (M0, 4352, "first"),                 # 17 tiles, exact: only the ragged tile is dead
    (M0, 4353, "random"),                # 18 tiles: three per queue, two queues empty
    (M0, M0 - 1, "last"),                # 18 tiles: every row but row 0, each moves down by one
    (M0, M0, "first"),                   # all live: the identity
    (M0, 3, "last_tile_only"),           # the whole ragged tile and nothing else
    # other batch sizes: one row, one row tile minus / plus one row, eight row tiles plus one row
    (1, 0, "first"),
    (1, 1, "first"),
    (255, 100, "random"),
    (255, 255, "first"),
    (256, 256, "first"),
    (256, 128, "alternate"),
    (256, 1, "last"),
    (257, 1, "last_tile_only"),          # the one live row is the one row of the second tile
    (257, 256, "first"),
    (2048, 512, "blocks4"),
    (2048, 1000, "random"),
    (2049, 257, "random"),
    (2049, 1, "last_tile_only"),
    (37 * 118, 2049, "random"),          # 4366 rows = 118 rays x 37 samples: a batch with more than one sample per view direction
]

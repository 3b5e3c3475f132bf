"""The sigma-gated forward (mofa_net_forward_gated) on PRESCRIBED live patterns: every (M, L, arrangement) of
tests/compact_reference.py's catalogue, at widths 512, 768 and 1024, against the full forward of the same batch — every word of raw, the
device-side counts, the verdict words of the colour launch.  tests/test_gpu_gate.py compares frames at whatever pattern a seeded network
produces; here the pattern is chosen and the network made to produce it.

A prescribed pattern from a real network: the density of a point does not depend on where the point sits in a batch, so a pool of points
is evaluated once (Renderer.query_density), split into live and dead points by compact_reference.live_rule, and every batch picks live
points where its mask is true and dead points elsewhere.  The full forward of the batch must then show exactly the mask (asserted, so no
test rests on that property).  The fine network's alpha bias is shifted by the pool's median density, which makes about half the pool live."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import compact_reference as cr
from harness import make_product
from mofanerf_amd import lib
from test_gpu_gate import KNOBS, _shipped_launch_forms, codes, fine, frame, scene  # noqa: F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 10
WIDTHS = (512, 768, 1024)
POOL = 32768
NAN = float("nan")
_POOL_COUNTS = {}


class _Shipped:
    """The module-scoped fixtures are built before the function-scoped ``_shipped_launch_forms`` runs: the same knobs, cleared here too."""

    def __enter__(self):
        self.saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
        lib.reload_env()
        lib.test_hooks()

    def __exit__(self, *exc):
        os.environ.update(self.saved)
        lib.reload_env()


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def box():
    """The box the test scene's rays cross between near = 8 and far = 26."""
    _, rays = scene(8)
    ends = torch.cat([rays[0] + rays[1] * 8.0, rays[0] + rays[1] * 26.0], 0)
    return ends.min(0).values, ends.max(0).values


def draw(n, seed):
    lo, hi = box()
    u = torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return (lo + (hi - lo) * u).contiguous()


def unit(n, seed):
    """n distinct unit view directions."""
    v = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return torch.nn.functional.normalize(v, dim=-1).contiguous()


def pool_density(render, kw, pool):
    bm, _, exp = codes()
    return render.query_density(kw["network_fine"], pool, shapeCodes=bm, expType=20, expCodes=exp)


class GatedNet:
    """One fine network of width W whose density splits a pool of points about in half, its folded codes, and the pool."""

    def __init__(self, W):
        self.W, self.Wp, self.Hp = W, (W + 63) // 64 * 64, (W // 2 + 63) // 64 * 64
        self.tiles_per_row_tile = D * self.Wp // 128 + self.Hp // 128          # the colour half: D texture layers + the view layer
        arch = (8, 64, D, W)
        self.pool = draw(POOL, 11)
        first, kw1, _ = make_product(arch, 0, 8192, DEV)
        median = float(pool_density(first, kw1, self.pool).median())
        del first, kw1
        self.render, self.kw, _ = make_product(arch, 0, 8192, DEV)
        with torch.no_grad():
            self.kw["network_fine"].alpha_linear[0].bias -= median
        K, rays = scene(8)
        frame(self.render, self.kw, 8, K, rays)                                  # folds the codes of the fine network
        self.h, self.folded = fine(self.render, self.kw), self.render._folded_fine.clone()
        sigma = pool_density(self.render, self.kw, self.pool)
        live = torch.from_numpy(cr.live_rule(bits(sigma))).to(DEV)
        self.live_idx, self.dead_idx = torch.nonzero(live).reshape(-1), torch.nonzero(~live).reshape(-1)
        self.render.gate_stats(reset=True)
        _POOL_COUNTS[W] = (int(self.live_idx.numel()), int(self.dead_idx.numel()), median)
        print(f"pool W={W}: {self.live_idx.numel()} live, {self.dead_idx.numel()} dead of {POOL} (median density {median:.6g} taken off the alpha bias)")

    def batch(self, m, seed=0):
        """Pool points [M,3] whose densities show the mask m: distinct live points where it is true, distinct dead ones elsewhere."""
        m = torch.from_numpy(np.asarray(m, dtype=bool)).to(DEV)
        n, L = int(m.numel()), int(m.sum())
        g = torch.Generator().manual_seed(100 + seed)
        pick = lambda idx, k: idx[torch.randperm(int(idx.numel()), generator=g)[:k].to(DEV)]
        idx = torch.empty(n, dtype=torch.int64, device=DEV)
        idx[m] = pick(self.live_idx, L)
        idx[~m] = pick(self.dead_idx, n - L)
        return self.pool[idx].contiguous()

    def counters(self):
        """(verdict words, gate counters) once everything issued so far has been verified."""
        torch.cuda.synchronize()
        self.h.check_verdict(block=True)
        stats = self.h.gate_stats_dev.tolist() if self.h.gate_stats_dev is not None else [0, 0]
        return self.h._verdict.tolist(), [int(v) for v in stats]

    def full_and_gated(self, m, run):
        """``run(out, gate)`` issues one forward into ``out [M,4]``.  The full forward must show the mask; the gated one must equal
        compact_reference.expected_raw of it word for word, count (M, L) and verify ceil(L / 256) row tiles of the colour half."""
        M, L = int(len(m)), cr.n_live(m)
        full, gated = torch.full((M, 4), 7.0, device=DEV), torch.full((M, 4), NAN, device=DEV)
        run(full, False)
        sigma_live = cr.live_rule(bits(full[:, 3]))
        assert np.array_equal(sigma_live, m), f"the full forward shows {int(sigma_live.sum())} live rows, the mask prescribes {L}"
        v0, s0 = self.counters()
        run(gated, True)
        v1, s1 = self.counters()
        assert self.h.last_gated == 1
        want = cr.expected_raw(full.cpu().numpy(), m)
        got = gated.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), \
            f"{int((got.view(np.int32) != want.view(np.int32)).any(-1).sum())} of {M} rows differ"
        assert (s1[0] - s0[0], s1[1] - s0[1]) == (M, L)
        tiles = cr.row_tiles(L)
        assert v1[0] == 0 and v1[1] - v0[1] == 2 and v1[5] == v0[5], (v0, v1)
        assert v1[3] == v1[4] == tiles * self.tiles_per_row_tile, (v1, tiles, self.tiles_per_row_tile)
        return full, gated, v1


@pytest.fixture(scope="module", params=WIDTHS)
def net(request):
    with _Shipped():
        return GatedNet(request.param)


def test_the_pool_holds_enough_live_and_dead_points(net):
    live, dead, median = _POOL_COUNTS[net.W]
    print(f"pool W={net.W}: live {live}, dead {dead}, median {median:.6g}")
    assert live >= cr.M0 and dead >= cr.M0 and live + dead == POOL


# ---- a. the catalogue at the entry point ---------------------------------------------------------------------------------------------
# The expected tiles of the colour launch (verdict word [4]), read off the step list of net_forward (mofa_net.hip): behind the geometry
# half come the texture stack's 5 + (D - 5) layers of Wp / 128 feature tiles each and the view layer's Hp / 128, per live row tile:
# 42 at width 512, 63 at 768, 84 at 1024 (GatedNet.tiles_per_row_tile).
@pytest.mark.parametrize("entry", cr.CATALOGUE, ids=lambda e: f"{e[0]}-{e[1]}-{e[2]}")
def test_every_catalogue_entry_is_the_full_forward_with_dead_colours_zeroed(net, entry):
    M, L, arrangement = entry
    m = cr.mask(M, L, arrangement)
    pts = net.batch(m)
    seen = []
    for S in [1] + [s for s in (128, 37) if M % s == 0][:1]:
        vd = unit(M // S, 7 + S)                                               # one direction per ray, all different: r = e / S matters
        run = lambda out, gate: net.h.forward_points(pts, vd, S, out.view(M // S, S, 4), net.folded, gate=gate)
        _, _, v = net.full_and_gated(m, run)
        seen.append((S, v[4]))
        if L == 0:
            assert v[3] == v[4] == 0
    print(f"W={net.W} M={M} L={L} {arrangement}: live row tiles {cr.row_tiles(L)} (queues {cr.xcd_split(cr.row_tiles(L))}), "
          f"verdict[4] per (S, tiles) {seen}, per live row tile {net.tiles_per_row_tile}")


# ---- b. special densities --------------------------------------------------------------------------------------------------------------
SPECIAL = {"+0": 0x00000000, "-0": 0x80000000, "+denormal": 0x00000001, "-denormal": 0x80000001, "FLT_MIN": 0x00800000,
           "+inf": 0x7f800000, "-inf": 0xff800000, "NaN": 0x7fc00000}


class FlatNet:
    """A fine network whose alpha head has zero weights: the density of every finite point is the head's bias."""

    def __init__(self, W):
        self.W = W
        self.render, self.kw, _ = make_product((8, 64, D, W), 0, 8192, DEV)
        K, rays = scene(8)
        frame(self.render, self.kw, 8, K, rays)
        self.h, self.head = fine(self.render, self.kw), self.kw["network_fine"].alpha_linear[0]
        with torch.no_grad():
            self.head.weight.zero_()
        self.pts = draw(300, 23)
        self.vd = unit(300, 29)

    def set_bias(self, word):
        with torch.no_grad():
            self.head.bias.copy_(torch.from_numpy(np.array([word], dtype=np.uint32).view(np.float32)))
            assert bits(self.head.bias).view(np.uint32)[0] == word
            return self.render._fold_codes(self.kw["network_fine"], self.render.decoding_texCodes).clone()

    def both(self, pts, folded):
        M = pts.shape[0]
        full, gated = torch.full((M, 1, 4), 7.0, device=DEV), torch.full((M, 1, 4), NAN, device=DEV)
        self.h.forward_points(pts, self.vd, 1, full, folded)
        before = self.h.gate_stats_dev.tolist() if self.h.gate_stats_dev is not None else [0, 0]
        self.h.forward_points(pts, self.vd, 1, gated, folded, gate=True)
        torch.cuda.synchronize()
        self.h.check_verdict(block=True)
        assert self.h.last_gated == 1
        after = self.h.gate_stats_dev.tolist()
        return full.reshape(M, 4), gated.reshape(M, 4), (int(after[0] - before[0]), int(after[1] - before[1]))


@pytest.fixture(scope="module", params=WIDTHS)
def flat(request):
    with _Shipped():
        return FlatNet(request.param)


@pytest.mark.parametrize("name", list(SPECIAL))
def test_the_rule_at_zeros_denormals_infinities_and_nan(flat, name):
    """Every row's density is one special value: k_gate_flags and k_gate_scatter must both read it as compact_reference.live_rule does —
    all rows live for +denormal, FLT_MIN, +inf and NaN, all rows dead for +0, -0, -denormal and -inf."""
    word = SPECIAL[name]
    folded = flat.set_bias(word)
    full, gated, (n, n_live) = flat.both(flat.pts, folded)
    sigma = bits(full[:, 3]).view(np.uint32)
    print(f"W={flat.W} bias {name} ({word:#010x}): sigma words {sorted({hex(v) for v in sigma.tolist()})}, counted {n_live} of {n} live")
    # the premise: the density the gate is given IS the special value (0 + b = b exactly; a zero keeps its magnitude; a NaN stays a NaN)
    if name == "NaN":
        assert ((sigma & 0x7fffffff) > 0x7f800000).all()
    elif name in ("+0", "-0"):
        assert ((sigma & 0x7fffffff) == 0).all()
    else:
        assert (sigma == word).all()
    live = cr.live_rule(sigma)
    assert live.all() == live.any() == bool(cr.live_rule(np.array([word], np.uint32))[0])
    want = cr.expected_raw(full.cpu().numpy(), live)
    assert np.array_equal(bits(gated), want.view(np.int32))
    assert np.array_equal(bits(gated[:, 3]), bits(full[:, 3]))
    assert (n, n_live) == (300, int(live.sum()))
    if not live.any():
        assert (bits(full[:, :3]) != 0).any()                                   # the full forward did compute colours: zeroing them is not vacuous


def test_nan_points_are_the_live_rows_of_a_dead_network(flat):
    folded = flat.set_bias(np.array([-1.0], np.float32).view(np.uint32)[0])
    m = cr.mask(300, 77, "random", seed=2)
    pts = flat.pts.clone()
    pts[torch.from_numpy(m).to(DEV)] = NAN
    full, gated, (n, n_live) = flat.both(pts, folded)
    sigma = bits(full[:, 3])
    assert np.array_equal(cr.live_rule(sigma), m) and np.isnan(full[:, 3].cpu().numpy()[m]).all()
    assert (full[:, 3].cpu().numpy()[~m] == -1.0).all()
    assert np.array_equal(bits(gated), cr.expected_raw(full.cpu().numpy(), m).view(np.int32))
    assert np.array_equal(bits(gated[:, 3]), sigma)
    assert (n, n_live) == (300, 77)


# ---- c. recycled and dirty workspace ---------------------------------------------------------------------------------------------------
def test_a_recycled_and_a_nan_filled_workspace_change_nothing(net):
    """The workspace is pure scratch: rows a previous call left behind the live ones, and NaN in every float of it, reach no output."""
    L_ = lib.load()
    M = cr.M0

    def call(entry, seed):
        m = cr.mask(*entry)
        pts, vd = net.batch(m, seed), unit(M, 40 + seed)
        return net.full_and_gated(m, lambda out, gate: net.h.forward_points(pts, vd, 1, out.view(M, 1, 4), net.folded, gate=gate))

    assert (M, M, "first") in cr.CATALOGUE and (M, 1, "last_tile_only") in cr.CATALOGUE and (M, 257, "blocks4") in cr.CATALOGUE
    call((M, M, "first"), 1)                                                   # every compacted row tile holds a live row's values
    call((M, 1, "last_tile_only"), 2)                                          # one live row in front of 255 stale ones of that call
    need = L_.mofa_net_forward_gated_workspace_floats(net.h.shape, M, M)
    ws = net.h.workspace(M, M, torch.device(DEV, torch.cuda.current_device()), 0, floats=need)
    assert ws.numel() >= need > L_.mofa_net_workspace_floats(net.h.shape, M, M)
    ws.fill_(NAN)
    call((M, 257, "blocks4"), 3)
    assert net.h.workspace(M, M, ws.device, 0, floats=need) is ws              # the same tensor served all three calls


# ---- d. rays form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_ray_z,n_live_rays,arrangement", [(True, 59, "random"), (False, 30, "blocks4")])
def test_the_rays_form_gates_whole_rays(net, per_ray_z, n_live_rays, arrangement):
    """forward_rays with o = a pool point and d = 0: every sample of a ray is that point (o + 0 z = o for any finite z), so a ray is
    all live or all dead; 118 rays x 37 samples is 17 row tiles and 14 rows."""
    R, S = 118, 37
    assert (R * S) % 256 != 0
    ray_mask = cr.mask(R, n_live_rays, arrangement, seed=4)
    m = np.repeat(ray_mask, S)
    o = net.batch(ray_mask, 5)
    d = torch.zeros(R, 3, device=DEV)
    vd = unit(R, 53)
    g = torch.Generator().manual_seed(6)
    if per_ray_z:
        z, zs = (8.0 + 18.0 * torch.rand(R, S, generator=g)).sort(-1).values.to(DEV).contiguous(), S
    else:
        z, zs = torch.linspace(8.0, 26.0, S).to(DEV).contiguous(), 0
    run = lambda out, gate: net.h.forward_rays(o, d, z, zs, vd, S, out.view(R, S, 4), net.folded, gate=gate)
    full, _, v = net.full_and_gated(m, run)
    rows = full.view(R, S, 4)
    assert torch.equal(rows, rows[:, :1].expand(R, S, 4))                      # one point, one direction per ray: S equal samples
    print(f"W={net.W} rays per_ray_z={per_ray_z}: {n_live_rays * S} live of {R * S}, verdict[4] {v[4]}")


# ---- e. caller-provided view bias rows --------------------------------------------------------------------------------------------------
def test_caller_provided_view_bias_rows_give_the_same_bits(net):
    """mofa_net_forward_gated with ``view_bias_rows`` from mofa_view_bias ([R, Hp], the layout autograd.view_bias_torch restates) and no
    view-layer tensors or directions at all, against the call that computes the rows itself."""
    L_ = lib.load()
    h = net.h
    M, L, arrangement = 2048, 1000, "random"
    assert (M, L, arrangement) in cr.CATALOGUE
    S, R = 128, M // 128
    m = cr.mask(M, L, arrangement)
    pts, vd = net.batch(m, 8), unit(R, 61)
    own = torch.full((R, S, 4), NAN, device=DEV)
    h.forward_points(pts, vd, S, own, net.folded, gate=True)
    view = h._linears[-3]
    vw, vb = view.weight.detach().contiguous(), view.bias.detach().contiguous()
    rows = torch.full((R, net.Hp), NAN, device=DEV)
    lib.check(L_.mofa_view_bias(lib.ptr(vd), R, h.view_freqs, lib.ptr(vw), view.out_features, view.in_features, lib.ptr(vb), lib.ptr(rows),
                                net.Hp, lib.stream()), "mofa_view_bias")
    dev = torch.device(DEV, torch.cuda.current_device())
    ws = h.workspace(M, R, dev, 0, floats=L_.mofa_net_forward_gated_workspace_floats(h.shape, M, R))
    given = torch.full((R, S, 4), NAN, device=DEV)
    route = C.c_int32(-1)
    lib.check(L_.mofa_net_forward_gated(h.shape, lib.ptr(h.packed()), lib.ptr(net.folded), None, None, None, None, None, 0, lib.ptr(pts), None,
                                        R, S, lib.ptr(ws), lib.ptr(given), lib.ptr(rows), h.gate_stats_buffer(dev).data_ptr(), C.byref(route),
                                        h.verdict_ptr(dev), lib.stream()), "mofa_net_forward_gated")
    h.snapshot_verdict()
    torch.cuda.synchronize()
    h.check_verdict(block=True)
    assert route.value == 1
    assert np.array_equal(bits(given), bits(own))
    assert np.array_equal(cr.live_rule(bits(own[..., 3])).reshape(-1), m) and (bits(own[..., :3]).reshape(M, 3)[~m] == 0).all()

"""The geometry-only render on the GPU (``mofa_ray_points``, ``mofa_composite_sigma``, ``mofa_occ_scatter_sigma``,
``Renderer.render_geometry``).  Everything geometric in a frame depends on density alone, so every comparison here is of BITS (an int32
view, NaN equal to NaN) against pieces that exist without the feature: NumPy's separately rounded ``o + d * z``,
``mofa_composite_forward`` on a raw whose channel 3 is the density, ``mofa_occ_scatter``'s channel 3, and whole ``render_fitting``
frames.  Only the recorded results (kat.npz, the oracle's raw2outputs) are compared at the project's gates for them."""
import ctypes as C

import numpy as np
import pytest
import torch

import occ_reference as occ
from conftest import nan_equal_close
from harness import make_product
from mofanerf_amd import lib, mesh, occupancy, synth
from mofanerf_amd.rays import get_rays, pose_spherical
from oracle import mofa_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = (8, 64, 10, 64)
WIDE = (8, 512, 10, 512)                                             # wide enough for the chained launch
BALL = dict(centre=(0.3, -0.2, 0.5), radius=3.0, res=(33, 29, 37), bounds=((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0)))


@pytest.fixture(autouse=True)
def _shipped_launch_forms(monkeypatch):
    for k in ("MOFA_PIPE", "MOFA_CHAIN", "MOFA_FUSED", "MOFA_CHAIN_TRAIN", "MOFA_GATE"):
        monkeypatch.delenv(k, raising=False)
    lib.reload_env()
    lib.test_hooks()
    yield
    monkeypatch.undo()
    lib.reload_env()
    lib.test_hooks()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    """torch.equal on the bits: NaN equals NaN (disp is NaN where acc == 0), -0 does not equal +0."""
    return tuple(a.shape) == tuple(b.shape) and torch.equal(bits(a), bits(b))


def composite_forward(raw, z, z_stride, rays_d, noise=None, white=0):
    R, S = raw.shape[0], raw.shape[1]
    o = {k: torch.full((R, *sh), 7.0, dtype=torch.float32, device=DEV) for k, sh in (("rgb", (3,)), ("disp", ()), ("acc", ()), ("depth", ()), ("weights", (S,)))}
    lib.check(lib.load().mofa_composite_forward(lib.ptr(raw), lib.ptr(z), z_stride, lib.ptr(rays_d), lib.ptr(noise), R, S, white, lib.ptr(o["rgb"]),
                                                lib.ptr(o["disp"]), lib.ptr(o["acc"]), lib.ptr(o["depth"]), lib.ptr(o["weights"]), lib.stream()),
              "mofa_composite_forward")
    return o


def composite_sigma(sigma, z, z_stride, rays_d, noise=None):
    R, S = sigma.shape
    o = {k: torch.full((R, *sh), 7.0, dtype=torch.float32, device=DEV) for k, sh in (("disp", ()), ("acc", ()), ("depth", ()), ("weights", (S,)))}
    lib.check(lib.load().mofa_composite_sigma(lib.ptr(sigma), lib.ptr(z), z_stride, lib.ptr(rays_d), lib.ptr(noise), R, S, lib.ptr(o["disp"]),
                                              lib.ptr(o["acc"]), lib.ptr(o["depth"]), lib.ptr(o["weights"]), lib.stream()), "mofa_composite_sigma")
    return o


# ---- 1. the points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 9])
@pytest.mark.parametrize("S", [1, 64, 257])
@pytest.mark.parametrize("per_ray_z", [False, True])
def test_ray_points_equal_numpy_with_a_separately_rounded_multiply_and_add(R, S, per_ray_z):
    rng = np.random.default_rng(100 * R + S)
    o = rng.uniform(-3, 3, (R, 3)).astype(np.float32)
    d = rng.normal(size=(R, 3)).astype(np.float32)
    z = rng.uniform(8, 26, (R, S) if per_ray_z else (S,)).astype(np.float32)
    want = occ.points(o, d, z).reshape(-1, 3)
    fused = (o[:, None, :].astype(np.float64) + d[:, None, :].astype(np.float64) * np.broadcast_to(z, (R, S))[..., None]).astype(np.float32).reshape(-1, 3)
    pts = torch.full((R * S + 1, 3), float("nan"), device=DEV)
    od, dd, zd = dev(o), dev(d), dev(z)
    lib.check(lib.load().mofa_ray_points(lib.ptr(od), lib.ptr(dd), lib.ptr(zd), S if per_ray_z else 0, R, S, lib.ptr(pts), lib.stream()),
              "mofa_ray_points")
    got = pts.cpu().numpy()
    assert np.array_equal(got[:-1].view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[-1]).all()                                    # nothing beyond the last point is written
    if R * S >= 64:
        assert not np.array_equal(want, fused)                        # a fused multiply-add would give other bits: the comparison can tell


# ---- 2. compositing against mofa_composite_forward -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 7, 63, 64, 65, 128, 129, 200, 256, 257, 300, 700])
def test_composite_sigma_gives_the_bits_of_composite_forward(S):
    R = 9
    rng = np.random.default_rng(S)
    raw = rng.normal(0, 1.5, (R, S, 4)).astype(np.float32)
    raw[3, :, 3] = -np.abs(raw[3, :, 3])                             # a ray whose densities are all <= 0 ...
    raw[3, S // 2, 3] = 0.0                                          # ... one of them exactly 0
    raw[5, :, 3] = np.abs(raw[5, :, 3]) * 40.0 + 1.0                 # an opaque ray: the transmittance underflows along it
    z_rows = np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1)
    d = dev(rng.normal(size=(R, 3)).astype(np.float32))
    noise = dev((rng.uniform(size=(R, S)) * 0.7).astype(np.float32))
    rawd = dev(raw)
    sigma = rawd[..., 3].contiguous()
    for z, zs in ((dev(z_rows), S), (dev(z_rows[0]), 0)):
        for nz in (None, noise):
            a = composite_forward(rawd, z, zs, d, nz)
            b = composite_sigma(sigma, z, zs, d, nz)
            for k in ("disp", "acc", "depth", "weights"):
                assert same(a[k], b[k]), (k, zs, nz is not None)
            if nz is None:
                assert float(b["acc"][3]) == 0.0 and float(b["depth"][3]) == 0.0 and bool(torch.isnan(b["disp"][3]))
                assert bool((b["weights"][3] == 0).all()) and float(b["acc"][5]) > 0.99
            assert float(b["acc"].max()) > 0.5 and bool(torch.isfinite(b["weights"]).all())
    other = rawd.clone()
    other[..., :3] = 5.0 - other[..., :3]                              # the colour channels are arbitrary: other values, the same geometry
    c = composite_forward(other, dev(z_rows), S, d)
    e = composite_sigma(sigma, dev(z_rows), S, d)
    assert all(same(c[k], e[k]) for k in ("disp", "acc", "depth", "weights"))


# ---- 3. compositing against recorded results -----------------------------------------------------------------------------------------
def test_composite_sigma_golden(golden):
    g = golden("kat.npz")
    for S in (64, 128):
        raw, z, d = (dev(g[f"r2o{S}_{n}"].astype(np.float32)) for n in ("raw", "z", "d"))
        sigma = raw[..., 3].contiguous()
        o = composite_sigma(sigma, z, S, d)
        for wb in (0, 1):                                              # geometry does not depend on the background
            for n in ("disp", "acc", "weights", "depth"):              # SURVEY §8d gate: composite <= 2e-6
                nan_equal_close(o[n].cpu().numpy(), g[f"r2o{S}_{wb}_{n}"], 2e-6, 2e-6)
        assert bool(torch.isnan(o["disp"][0]))
        np.random.seed(0)
        noise = dev((np.random.rand(*raw.shape[:2]) * 0.7).astype(np.float32))
        o = composite_sigma(sigma, z, S, d, noise)
        for n in ("disp", "acc", "weights", "depth"):
            nan_equal_close(o[n].cpu().numpy(), g[f"r2o{S}_noise_{n}"], 2e-6, 2e-6)


def test_composite_sigma_ragged_sample_counts_against_the_oracle():
    rng = np.random.default_rng(2)
    for S in (2, 7, 63, 65, 100, 129, 200, 256):
        R = 9
        raw = torch.from_numpy(rng.normal(0, 1.5, (R, S, 4)).astype(np.float32))
        z = torch.from_numpy(np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1))
        d = torch.from_numpy(rng.normal(size=(R, 3)).astype(np.float32))
        ref = dict(zip(("rgb", "disp", "acc", "weights", "depth"), orc.raw2outputs(raw, z, d, None, False)))
        o = composite_sigma(raw[..., 3].contiguous().to(DEV), z.to(DEV), S, d.to(DEV))
        for n in ("disp", "acc", "weights", "depth"):
            nan_equal_close(o[n].cpu().numpy(), ref[n].numpy(), 3e-6, 3e-6)


# ---- 4. the one-float scatter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [0.0, 0.3, 1.0])
def test_occ_scatter_sigma_is_channel_3_of_occ_scatter(share):
    """Flags and their scan come from mofa_occ_classify on a one-cell lattice whose cell is occupied: a sample is kept iff its point is
    inside the bounds, so the rays' origins choose the flags (random, none, all)."""
    L, st = lib.load(), lib.stream()
    rng = np.random.default_rng(7)
    R, S = 700, 9                                                     # 6300 samples: several scan tiles
    n = R * S
    inside = rng.uniform(size=(R, S)) < share if 0.0 < share < 1.0 else np.full((R, S), share == 1.0)
    z = np.where(inside, 0.5, 5.0).astype(np.float32)                  # p = (0, 0, z): inside [-1, 1]^3 or beyond it
    o, d = np.zeros((R, 3), np.float32), np.tile(np.float32([0, 0, 1]), (R, 1))
    res, lo, step = mesh.grid_spec(((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), (2, 2, 2))
    cells = torch.ones(1, dtype=torch.uint8, device=DEV)
    flags = torch.full((R, S), 7, dtype=torch.uint8, device=DEV)
    ws = torch.empty(L.mofa_occ_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    counts = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    od, dd, zd = dev(o), dev(d), dev(z)
    lib.check(L.mofa_occ_classify(lib.ptr(od), lib.ptr(dd), lib.ptr(zd), S, R, S, cells.data_ptr(), *res, mesh._f3(lo), mesh._f3(step),
                                  flags.data_ptr(), ws.data_ptr(), counts.data_ptr(), st), "mofa_occ_classify")
    n_kept = int(counts.cpu())
    assert np.array_equal(flags.cpu().numpy().astype(bool), inside) and n_kept == int(inside.sum())
    assert {0.0: n_kept == 0, 0.3: 0 < n_kept < n, 1.0: n_kept == n}[share]
    raw_kept = torch.randn(max(n_kept, 1), 4, device=DEV)
    raw_kept[0, 3] = float("nan")                                     # a NaN density travels as it is
    raw = torch.full((R, S, 4), 3.0, device=DEV)
    lib.check(L.mofa_occ_scatter(lib.ptr(raw_kept) if n_kept else None, flags.data_ptr(), ws.data_ptr(), n, n_kept, lib.ptr(raw), st), "mofa_occ_scatter")
    sigma_kept = raw_kept[:, 3].contiguous()
    sigma = torch.full((R, S), 3.0, device=DEV)
    lib.check(L.mofa_occ_scatter_sigma(lib.ptr(sigma_kept) if n_kept else None, flags.data_ptr(), ws.data_ptr(), n, n_kept, lib.ptr(sigma), st),
              "mofa_occ_scatter_sigma")
    assert same(sigma, raw[..., 3])
    assert not bool((sigma == 3.0).any())                             # every element is written by the one kernel
    want = np.zeros(n, np.float32)
    want[np.flatnonzero(inside.reshape(-1))] = sigma_kept.cpu().numpy()[:n_kept]
    assert np.array_equal(sigma.cpu().numpy().reshape(-1).view(np.uint32), want.view(np.uint32))
    if n_kept > 1:                                                    # a count that does not belong to the flags: slots beyond it give NaN, in both
        short = n_kept // 2
        lib.check(L.mofa_occ_scatter(lib.ptr(raw_kept), flags.data_ptr(), ws.data_ptr(), n, short, lib.ptr(raw), st), "mofa_occ_scatter")
        lib.check(L.mofa_occ_scatter_sigma(lib.ptr(sigma_kept), flags.data_ptr(), ws.data_ptr(), n, short, lib.ptr(sigma), st), "mofa_occ_scatter_sigma")
        assert same(sigma, raw[..., 3]) and int(torch.isnan(sigma).sum()) >= n_kept - short


# ---- whole frames ----------------------------------------------------------------------------------------------------------------------
def scene(H=16, angle=25.0):
    K = synth.intrinsics(H, H)
    ro, rd = get_rays(H, H, K, pose_spherical(angle, 0.0, 16.0), device=DEV)
    return K, ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()


def codes(seed=0):
    bm, tex, exp = synth.codes(seed)
    return bm.to(DEV), tex.to(DEV), exp.to(DEV)


def full_frame(render, kw, K, ro, rd, H=16, chunk=4096, tex=None, **more):
    """render_fitting: (rgb, disp, acc, extras)."""
    bm, t, exp = codes()
    torch.manual_seed(11)                                             # the device_rng case: both renders draw from the same generator state
    with torch.no_grad():
        out = render.render_fitting(H, H, K, chunk=chunk, rays=torch.stack([ro, rd], 0), shapeCodes=bm, uvCodes=t if tex is None else tex,
                                    expType=20, expCodes=exp, **dict(kw, **more))
    render.check_launches(block=True)
    return out


def geometry(render, kw, K, ro, rd, H=16, chunk=4096, bm=None, exp=None, **more):
    """render_geometry: (depth, disp, acc, extras)."""
    b, _, e = codes()
    torch.manual_seed(11)
    out = render.render_geometry(H, H, K, chunk=chunk, rays=torch.stack([ro, rd], 0), shapeCodes=b if bm is None else bm, expType=20,
                                 expCodes=e if exp is None else exp, **dict(kw, **more))
    render.check_launches(block=True)
    return out


def same_frames(a, b):
    return (all(same(x, y) for x, y in zip(a[:3], b[:3])) and set(a[3]) == set(b[3]) and all(same(a[3][k], b[3][k]) for k in a[3]))


# device_rng: the draws come from torch.rand on the device, so only the ORDER and SHAPES of the two renders' draws (t_rand [R,S], then
# u [R,Ni]) hold the frames together
_cases = {"det": dict(perturb=0.), "stochastic": dict(perturb=1., pytest=True), "lindisp": dict(lindisp=True), "per_ray_bounds": "bounds",
          "coarse_only": dict(), "device_rng": dict(perturb=1.)}


@pytest.mark.parametrize("case", list(_cases))
def test_a_geometry_frame_is_the_full_frames_geometry_bit_for_bit(case):
    n_imp = 0 if case == "coarse_only" else 64
    render, kw, _ = make_product(ARCH, 0, 4096, DEV, N_importance=n_imp)
    K, ro, rd = scene()
    R, S = ro.shape[0], 64
    flags = _cases[case]
    if flags == "bounds":
        rng = np.random.default_rng(3)
        flags = dict(near=dev(rng.uniform(7.0, 9.0, R).astype(np.float32)), far=dev(rng.uniform(24.0, 27.0, R).astype(np.float32)))
    full = full_frame(render, kw, K, ro, rd, retraw=True, verbose=True, **flags)
    depth, disp, acc, ex = geometry(render, kw, K, ro, rd, retweights=True, **flags)
    assert depth.shape == disp.shape == acc.shape == (R,) and ex["weights"].shape == ex["z_vals"].shape == (R, S + n_imp)
    assert same(disp, full[1]) and same(acc, full[2])
    if n_imp:
        assert set(ex) == {"depth0", "disp0", "acc0", "z_std", "weights", "z_vals"}
        for k in ("disp0", "acc0", "z_std"):
            assert same(ex[k], full[3][k]), k
        z = full[3]["_z_fine"].contiguous()
    else:
        assert set(ex) == {"weights", "z_vals"}
        t = torch.linspace(0., 1., steps=S)                           # the reference's coarse row, built on the host (render_class.py:266-270)
        z = (torch.tensor([[8.0]]) * (1. - t) + torch.tensor([[26.0]]) * t).reshape(1, -1).expand(R, S).contiguous().to(DEV)
    assert same(ex["z_vals"], z)
    want = composite_forward(full[3]["raw"].contiguous(), z, z.shape[1], rd)
    assert same(want["disp"], full[1]) and same(want["acc"], full[2])          # (the restatement is the frame's own compositing)
    assert same(depth, want["depth"]) and same(ex["weights"], want["weights"])
    assert float(acc.max()) > 0.1 and float(depth.max()) > 8.0
    plain = geometry(render, kw, K, ro, rd, **flags)                  # without retweights: the same frame, no weights
    assert same(plain[0], depth) and same(plain[1], disp) and set(plain[3]) == set(ex) - {"weights", "z_vals"}
    if n_imp:                                                        # is_run_fineNet = False returns the coarse outputs
        render.is_run_fineNet = False
        c = geometry(render, kw, K, ro, rd, **flags)
        assert same(c[0], ex["depth0"]) and same(c[1], ex["disp0"]) and same(c[2], ex["acc0"]) and c[3] == {}


def test_geometry_frames_keep_their_shape_and_take_a_pose():
    """c2w instead of rays: [H,W] maps, equal to the frame rendered from the same rays; the verdicts travel as for render."""
    render, kw, _ = make_product(ARCH, 0, 4096, DEV)
    H = 8
    K = synth.intrinsics(H, H)
    pose = pose_spherical(-20.0, 0.0, 16.0)
    bm, tex, exp = codes()
    depth, disp, acc, ex = render.render_geometry(H, H, K, c2w=pose[:3, :4], shapeCodes=bm, expType=20, expCodes=exp, **kw)
    check = render.frame_check()
    with torch.no_grad():
        full = render.render_fitting(H, H, K, c2w=pose[:3, :4], shapeCodes=bm, uvCodes=tex, expType=20, expCodes=exp, **kw)
    check()
    render.check_launches(block=True)
    assert depth.shape == disp.shape == acc.shape == ex["z_std"].shape == (H, H)
    assert same(disp, full[1]) and same(acc, full[2]) and same(ex["z_std"], full[3]["z_std"])
    assert not depth.requires_grad
    grad_codes = bm.clone().requires_grad_(True)                      # inference only, whatever asks for a gradient
    again = render.render_geometry(H, H, K, c2w=pose[:3, :4], shapeCodes=grad_codes, expType=20, expCodes=exp, **kw)
    assert same(again[0], depth) and not again[0].requires_grad


# ---- 6. chunking and launch forms ----------------------------------------------------------------------------------------------------
def test_geometry_frames_do_not_depend_on_chunk_or_netchunk():
    render, kw, _ = make_product(ARCH, 0, 4096, DEV)
    K, ro, rd = scene()
    base = geometry(render, kw, K, ro, rd, retweights=True)
    for chunk in (4096, 1000, 65536, 100, 37):
        for netchunk in (4096, 1000, 65536):
            render.netchunk = netchunk
            out = geometry(render, kw, K, ro, rd, chunk=chunk, retweights=True)
            assert same_frames(base, out), (chunk, netchunk)
    render.netchunk = 50                                              # fewer points than one ray holds: sub-batches of one ray
    assert same_frames(base, geometry(render, kw, K, ro, rd, chunk=64, retweights=True))


def test_geometry_frames_are_the_same_under_per_layer_and_chained_launches(knob):
    K, ro, rd = scene()
    frames = {}
    for chain in ("1", "0"):
        knob("MOFA_CHAIN", chain)
        render, kw, _ = make_product(WIDE, 0, 4096, DEV)
        frames[chain] = geometry(render, kw, K, ro, rd, retweights=True)
        launches = render._hip(kw["network_fine"]).chained_launches()
        assert launches == 0 if chain == "0" else (launches > 0 or lib.chain_selfcheck() != 1)
        if chain == "0":
            full = full_frame(render, kw, K, ro, rd)
    assert same_frames(frames["1"], frames["0"])
    g = frames["1"]
    assert same(g[1], full[1]) and same(g[2], full[2]) and all(same(g[3][k], full[3][k]) for k in ("disp0", "acc0", "z_std"))
    assert float(g[2].max()) > 0


# ---- 7. with an occupancy grid -------------------------------------------------------------------------------------------------------
def ball_occupancy(dilate=1):
    res, lo, step = mesh.grid_spec(BALL["bounds"], BALL["res"])
    g = occ.ball_grid(res, lo, step, BALL["centre"], BALL["radius"])
    return occupancy.occupancy_from_grid(dev(g), 0.0, lo, step, dilate=dilate)


def const_occupancy(value):
    res, lo, step = mesh.grid_spec(((-40.0, -40.0, -40.0), (40.0, 40.0, 40.0)), (9, 9, 9))
    return occupancy.occupancy_from_grid(torch.full(res, float(value), device=DEV), 0.0, lo, step, dilate=0)


@pytest.mark.parametrize("perturb", [0., 1.])
def test_a_culled_geometry_frame_is_the_culled_full_frames_geometry(perturb):
    render, kw, _ = make_product(ARCH, 0, 4096, DEV)
    K, ro, rd = scene()
    grid = ball_occupancy(dilate=1)
    flags = dict(perturb=perturb, pytest=True)
    full = full_frame(render, kw, K, ro, rd, occupancy=grid, retraw=True, verbose=True, **flags)
    stats = {k: dict(v) for k, v in render.occupancy_stats.items()}
    depth, disp, acc, ex = geometry(render, kw, K, ro, rd, occupancy=grid, retweights=True, **flags)
    assert render.occupancy_stats == stats and 0 < stats["coarse"]["kept"] < stats["coarse"]["samples"] and 0 < stats["fine"]["kept"] < stats["fine"]["samples"]
    assert same(disp, full[1]) and same(acc, full[2])
    for k in ("disp0", "acc0", "z_std"):
        assert same(ex[k], full[3][k]), k
    z = full[3]["_z_fine"].contiguous()
    want = composite_forward(full[3]["raw"].contiguous(), z, z.shape[1], rd)
    assert same(ex["z_vals"], z) and same(depth, want["depth"]) and same(ex["weights"], want["weights"])
    unculled = geometry(render, kw, K, ro, rd, retweights=True, **flags)
    assert render.occupancy_stats is None
    assert not same(unculled[2], acc)                                  # the ball does cut density away
    if perturb == 0.:                                                 # (the seeded draws of a stochastic frame are per chunk of rays)
        for chunk, netchunk in ((100, 777), (37, 1 << 20)):           # ... whatever the chunking
            render.netchunk = netchunk
            out = geometry(render, kw, K, ro, rd, chunk=chunk, occupancy=grid, retweights=True, **flags)
            assert render.occupancy_stats == stats and same_frames([depth, disp, acc, ex], out), (chunk, netchunk)
        render.netchunk = 4096
    everything = const_occupancy(1.0)
    out = geometry(render, kw, K, ro, rd, occupancy=everything, retweights=True, **flags)
    n = ro.shape[0]
    assert render.occupancy_stats == {"coarse": {"samples": n * 64, "kept": n * 64}, "fine": {"samples": n * 128, "kept": n * 128}}
    assert same_frames(unculled, out)


def test_an_empty_grid_gives_an_empty_geometry_frame_and_launches_no_network():
    render, kw, _ = make_product(WIDE, 0, 4096, DEV)
    K, ro, rd = scene()
    empty = const_occupancy(-1.0)
    assert empty.fraction == 0.0
    g = geometry(render, kw, K, ro, rd)                                # un-culled: binds the networks and launches them
    assert float(g[2].max()) > 0
    hips = [render._hip(kw["network_fn"]), render._hip(kw["network_fine"])]
    before = [h.chained_launches() for h in hips]
    assert sum(before) > 0 or lib.chain_selfcheck() != 1
    L = lib.load()
    lib.check(L.mofa_prof_begin(), "mofa_prof_begin")
    depth, disp, acc, ex = geometry(render, kw, K, ro, rd, occupancy=empty, retweights=True)
    torch.cuda.synchronize()
    ms, calls, work = (C.c_double * lib.PROF_KINDS)(), (C.c_int64 * lib.PROF_KINDS)(), (C.c_double * lib.PROF_KINDS)()
    lib.check(L.mofa_prof_end(ms, calls, work), "mofa_prof_end")
    assert all(calls[k] == 0 for k in (0, 1, 2, 3, 4, 5, 6, 7, 11)), list(calls)      # every MFMA kernel kind
    assert calls[8] == calls[9] == 0 and calls[10] == 1                              # no colour compositing either; the resampling ran
    assert [h.chained_launches() for h in hips] == before                            # the verdict words show no launch
    assert render.occupancy_stats == {"coarse": {"samples": 256 * 64, "kept": 0}, "fine": {"samples": 256 * 128, "kept": 0}}
    zero = torch.zeros_like(acc)
    assert same(acc, zero) and same(depth, zero) and bool(torch.isnan(disp).all())
    assert same(ex["acc0"], zero) and same(ex["depth0"], zero) and bool(torch.isnan(ex["disp0"]).all())
    assert same(ex["weights"], torch.zeros_like(ex["weights"]))


def test_the_refusals_of_culled_rendering_apply_except_the_autograd_one():
    render, kw, _ = make_product(ARCH, 0, 4096, DEV)
    K, ro, rd = scene(8)
    grid = ball_occupancy()
    with pytest.raises(lib.MofaError, match="occupancy"):
        geometry(render, kw, K, ro, rd, H=8, occupancy=grid.cells())
    cpu_grid = occupancy.OccupancyGrid(grid._cells.cpu(), grid.resolution, grid.lo, grid.step, 0.0, 1, grid.fraction)
    with pytest.raises(lib.MofaError, match="occupancy.*lives on"):
        geometry(render, kw, K, ro, rd, H=8, occupancy=cpu_grid)
    with pytest.raises(lib.MofaError, match="raw_noise_std"):
        geometry(render, kw, K, ro, rd, H=8, occupancy=grid, raw_noise_std=1.0)
    bm = codes()[0].clone().requires_grad_(True)                       # autograd on and a code that asks: the geometry render is detached anyway
    a = geometry(render, kw, K, ro, rd, H=8, occupancy=grid, bm=bm)
    b = geometry(render, kw, K, ro, rd, H=8, occupancy=grid)
    assert same_frames(a, b) and not a[0].requires_grad
    _, kw_cpu, _ = make_product(ARCH, 0, 4096, "cpu")
    with pytest.raises(lib.MofaError, match="GPU"):
        geometry(render, dict(kw, network_fn=kw_cpu["network_fn"]), K, ro, rd, H=8)          # a CPU network
    with pytest.raises(lib.MofaError, match="CPU"):
        geometry(render, kw, K, ro.cpu(), rd.cpu(), H=8)                                     # CPU rays


# ---- 8. what the geometry depends on ---------------------------------------------------------------------------------------------------
def test_geometry_ignores_texture_and_view_and_follows_shape_and_expression():
    render, kw, _ = make_product(ARCH, 0, 4096, DEV)
    K, ro, rd = scene()
    bm, tex, exp = codes()
    base = geometry(render, kw, K, ro, rd, retweights=True)
    rgb_a = full_frame(render, kw, K, ro, rd)[0]
    rgb_b = full_frame(render, kw, K, ro, rd, tex=torch.flip(tex, (0,)) * 1.5)[0]       # another texture code is bound now
    assert not same(rgb_a, rgb_b)
    assert same_frames(base, geometry(render, kw, K, ro, rd, retweights=True))
    with torch.no_grad():                                             # another view bias: the view layers' weights and biases
        for net in (kw["network_fn"], kw["network_fine"]):
            view = render._hip(net)._linears[-3]
            view.bias.add_(0.5)
            view.weight.mul_(-1.0)
    assert not same(rgb_a, full_frame(render, kw, K, ro, rd)[0])
    assert same_frames(base, geometry(render, kw, K, ro, rd, retweights=True))
    other_shape = geometry(render, kw, K, ro, rd, bm=bm * 0.5 + 0.1)
    other_exp = geometry(render, kw, K, ro, rd, exp=exp + 0.25)
    for other in (other_shape, other_exp):
        assert not same(other[0], base[0]) and not same(other[2], base[2])
    assert same_frames(base, geometry(render, kw, K, ro, rd, retweights=True))             # and back

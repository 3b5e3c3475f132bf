"""The surface buffers of the geometry render on the GPU (``mofa_depth_median``, ``mofa_point_normals``, the ``median`` / ``points`` /
``normals`` options of ``Renderer.render_geometry``, ``Renderer.render_path_geometry``) against the NumPy restatements of
tests/geom_reference.py (which tests/test_geom_reference_cpu.py checks on their own).

* The median on weights ``k_i / 1024`` (integers, sum <= 1024): every partial sum is exact in fp32 under any association, so index and
  depth must EQUAL the fp64 restatement's.  On alpha-compositing weights an fp32 prefix sum lies within ``eps = (S-1) 2^-24 sum|w|`` of
  the exact one, so the index must lie in the window that leaves — and the window must be one index wide on nearly every ray.
* The normals are separately rounded fp32 operations in a fixed order: bits.
* Whole frames: the options change nothing that existed; the new buffers follow from the frame's own weights, rays and acc."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import geom_reference as ref
import occ_reference as occ
from harness import make_product
from mofanerf_amd import lib, mesh, occupancy, synth
from mofanerf_amd.rays import get_rays, pose_spherical

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = (8, 64, 10, 64)
GUARD = 8
# the CPU oracle's acc of this scene (seeded networks ARCH, 16 + 16 samples, azimuth 25 degrees, near 8, far 26): 37.5 % of the 8 x 8 view and
# 33.3 % of the 16 x 12 view are >= 0.2, and no pixel's acc is within 3.8e-3 of it (the GPU's acc is within 1e-5 of the oracle's)
ACC_MIN = 0.2
# half of ACC_MIN: the depth at which half of the least mass a usable pixel holds has accumulated — reached on every usable ray; the default
# 0.5 is reached on a few per cent of these rays only (the -1 path of whole frames)
THRESHOLD = 0.1


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


def guarded(n, dtype, fill):
    """A buffer of n elements with GUARD words of `fill` on either side: (whole, the n elements)."""
    whole = torch.full((n + 2 * GUARD,) if isinstance(n, int) else (n[0] + 2 * GUARD, *n[1:]), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + (n if isinstance(n, int) else n[0])]


def guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def depth_median(w, z, zs, threshold):
    """(index, depth) as numpy, from two calls that must agree bit for bit and leave the words around both outputs alone."""
    R, S = w.shape
    got = []
    for _ in range(2):
        dw, d = guarded(R, torch.float32, 7.0)
        iw, i = guarded(R, torch.int32, -77)
        lib.check(lib.load().mofa_depth_median(lib.ptr(w), lib.ptr(z), zs, R, S, threshold, lib.ptr(d), i.data_ptr(), lib.stream()), "mofa_depth_median")
        assert guards_intact(dw, 7.0) and guards_intact(iw, -77)
        got.append((i.cpu().numpy(), d.cpu().numpy()))
    assert ref.same_bits(got[0][0], got[1][0]) and ref.same_bits(got[0][1], got[1][1])
    return got[0]


def point_normals(P, acc, D, acc_min):
    H, W = acc.shape
    got = []
    for _ in range(2):
        nw, n = guarded((H * W, 3), torch.float32, 7.0)
        vw, v = guarded(H * W, torch.uint8, 9)
        lib.check(lib.load().mofa_point_normals(lib.ptr(P), lib.ptr(acc), lib.ptr(D), H, W, acc_min, lib.ptr(n), v.data_ptr(), lib.stream()),
                  "mofa_point_normals")
        assert guards_intact(nw, 7.0) and guards_intact(vw, 9)
        got.append((n.cpu().numpy().reshape(H, W, 3), v.cpu().numpy().reshape(H, W)))
    assert ref.same_bits(got[0][0], got[1][0]) and ref.same_bits(got[0][1], got[1][1])
    return got[0]


# ---- 1. the median where every partial sum is exact ------------------------------------------------------------------------------------
KINDS = ("full", "partial", "zero", "nan", "tie")


def dyadic_rows(R, S, first, rng):
    """k [R,S] integers with row sums <= 1024 (as float64, NaN allowed): a row of kind KINDS[(r + first) % 5] — the whole 1024 spread over the
    row (its last prefix sum EQUALS 1), a random part of it, nothing, a NaN at a random sample, a prefix sum that EQUALS 1/2."""
    k = np.zeros((R, S), np.float64)
    for r in range(R):
        kind = KINDS[(r + first) % 5]
        if kind == "full":
            k[r] = rng.multinomial(1024, rng.dirichlet(np.ones(S)))
        elif kind == "partial":
            k[r] = rng.multinomial(int(rng.integers(1, 1025)), rng.dirichlet(np.ones(S)))
        elif kind == "nan":
            k[r] = rng.multinomial(1024, np.ones(S) / S)
            k[r, rng.integers(0, S)] = np.nan
        elif kind == "tie":
            j = int(rng.integers(0, S))
            k[r, :j + 1] = rng.multinomial(512, np.ones(j + 1) / (j + 1))
            if j + 1 < S:
                k[r, j + 1:] = rng.multinomial(int(rng.integers(0, 513)), np.ones(S - j - 1) / (S - j - 1))
    return k


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 128, 129, 256, 257, 600])
def test_the_median_of_dyadic_weights_is_numpys_exactly(S):
    rng = np.random.default_rng(1000 + S)
    seen = set()
    for R in (1, 3, 4, 5, 257):
        for first in (range(5) if R == 1 else (0,)):
            k = dyadic_rows(R, S, first, rng)
            w = (k / 1024.0).astype(np.float32)
            z_rows = np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1)
            for z, zs in ((z_rows, S), (z_rows[0], 0)):
                for t in (0.5, 1.0, 0.37):
                    want_i, want_d = ref.median_exact(w, z, t)
                    got_i, got_d = depth_median(dev(w), dev(z), zs, t)
                    assert np.array_equal(got_i, want_i), (R, first, zs, t, np.flatnonzero(got_i != want_i)[:8])
                    assert ref.same_bits(got_d, want_d), (R, first, zs, t)
                    if t == 0.5:
                        C = np.cumsum(k, -1)
                        seen |= {"tie"} if (C[np.arange(R), np.maximum(want_i, 0)] == 512).any() else set()
                        seen |= {"none"} if (want_i < 0).any() else set()
                        seen |= {"nan"} if np.isnan(k).any() else set()
    assert seen == {"tie", "none", "nan"}


# ---- 2. the median of compositing weights: the window the rounding of an fp32 prefix sum leaves ----------------------------------------
@pytest.mark.parametrize("S", [2, 64, 65, 192, 257, 600])
def test_the_median_of_composited_weights_lies_in_its_window(S):
    rng = np.random.default_rng(S)
    R = 4096
    sigma = np.maximum(rng.normal(size=(R, S)), 0.0) * rng.uniform(0.0, 3.0, (R, 1))
    w = ref.composite_weights(sigma, 0.1)
    z_rows = np.sort(rng.uniform(8, 26, (R, S)).astype(np.float32), -1)
    for z, zs in ((z_rows, S), (z_rows[0], 0)):
        for t in (0.5, 0.05):
            got_i, got_d = depth_median(dev(w), dev(z), zs, t)
            bad, ambiguous = ref.median_check(w, z, t, got_i, got_d)
            print(f"S={S} stride={zs} t={t}: {bad.size} rays outside their window, {100 * ambiguous:.3f} % admit more than one index, "
                  f"{(got_i < 0).mean():.3f} without a crossing")
            assert bad.size == 0, (zs, t, bad[:8], got_i[bad[:8]])
            assert ambiguous <= 0.01, (zs, t, ambiguous)
            assert (got_i >= 0).any()


# ---- 3. the normals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (7, 9), (33, 65)])
def test_point_normals_are_the_restatements_bits(H, W):
    rng = np.random.default_rng(100 * H + W)
    P = rng.normal(size=(H, W, 3)).astype(np.float32)
    D = rng.normal(size=(H, W, 3)).astype(np.float32)
    acc = rng.uniform(0.3, 0.8, (H, W)).astype(np.float32)
    acc[rng.uniform(size=(H, W)) < 0.15] = np.float32(0.55)           # exactly acc_min
    acc[rng.uniform(size=(H, W)) < 0.1] = np.nan
    if H >= 3 and W >= 3:      # a patch of the plane z = 0 (two components of its normal are exactly 0, of either sign) under a grazing ray
        r, c = np.meshgrid(np.arange(3, dtype=np.float32), np.arange(3, dtype=np.float32), indexing="ij")      # (n . d = 0 exactly) and a
        P[:3, :3] = np.stack([c, r, np.zeros_like(c)], -1)            # ray along the normal: what tells dv x du from du x dv
        acc[:3, :3] = 1.0
        D[1, 1], D[0, 0] = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)
    flat = P.copy()
    if H >= 3 and W >= 3:
        flat[:3, :3] = flat[1, 1]                                     # coincident points: the centre's cross product has length 0
    cases = {"random": (P, acc), "all": (P, np.ones_like(acc)), "none": (P, np.zeros_like(acc)), "flat": (flat, np.ones_like(acc))}
    for name, (pts, a) in cases.items():
        want_n, want_v = ref.point_normals(pts, a, D, 0.55)
        got_n, got_v = point_normals(dev(pts), dev(a), dev(D), 0.55)
        assert ref.same_bits(got_v, want_v), (name, np.argwhere(got_v != want_v)[:8])
        assert ref.same_bits(got_n, want_n), (name, np.argwhere(got_n.view(np.uint32) != want_n.view(np.uint32))[:8])
        if name == "none" or min(H, W) == 1:
            assert not got_v.any() and not got_n.any()
        elif name == "all":
            assert got_v.all()
        elif name == "flat" and H >= 3 and W >= 3:
            assert got_v[1, 1] == 0 and got_v.sum() < got_v.size
    if H * W >= 63:                                                   # the comparison can tell: each wrong stencil gives other bits here
        want = ref.point_normals(P, acc, D, 0.55)
        for fault in ref.FAULTS:
            wrong = ref.point_normals(P, acc, D, 0.55, fault=fault)
            assert not (ref.same_bits(want[0], wrong[0]) and ref.same_bits(want[1], wrong[1])), fault


# ---- 4. whole frames -------------------------------------------------------------------------------------------------------------------
BALL = dict(centre=(0.3, -0.2, 0.5), radius=3.0, res=(33, 29, 37), bounds=((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0)))
NEW_KEYS = {"depth_median", "median_index", "points", "normals", "normals_valid"}


def bits_equal(a, b):
    return tuple(a.shape) == tuple(b.shape) and a.dtype == b.dtype and ref.same_bits(a.cpu().numpy(), b.cpu().numpy())


def ball_occupancy():
    res, lo, step = mesh.grid_spec(BALL["bounds"], BALL["res"])
    g = occ.ball_grid(res, lo, step, BALL["centre"], BALL["radius"])
    return occupancy.occupancy_from_grid(dev(g), 0.0, lo, step, dilate=1)


def view(H, W, angle=25.0):
    K = synth.intrinsics(H, W)
    pose = pose_spherical(angle, 0.0, 16.0)
    ro, rd = get_rays(H, W, K, pose, device=DEV)
    return K, pose, torch.stack([ro.reshape(H, W, 3), rd.reshape(H, W, 3)], 0).contiguous()


def codes():
    bm, _, exp = synth.codes(0)
    return bm.to(DEV), exp.to(DEV)


def frame(render, kw, H, W, K, chunk=1 << 20, **more):
    bm, exp = codes()
    out = render.render_geometry(H, W, K, chunk=chunk, shapeCodes=bm, expType=20, expCodes=exp, **dict(kw, **more))
    render.check_launches(block=True)
    return out


@pytest.mark.parametrize("culled", [False, True])
@pytest.mark.parametrize("H,W", [(8, 8), (16, 12)])
def test_surface_buffers_of_a_frame(H, W, culled):
    render, kw, _ = make_product(ARCH, 0, 4096, DEV, N_samples=16, N_importance=16)
    K, _, rays = view(H, W)
    more = dict(rays=rays, retweights=True, occupancy=ball_occupancy() if culled else None)
    off = frame(render, kw, H, W, K, **more)
    o, d = rays[0].cpu().numpy(), rays[1].cpu().numpy()
    hits = 0
    for surface, threshold in (("median", THRESHOLD), ("expected", THRESHOLD), ("median", 0.5)):
        opts = dict(more, median=True, points=True, normals=True, surface=surface, acc_min=ACC_MIN, median_threshold=threshold)
        on = frame(render, kw, H, W, K, **opts)
        # nothing that existed moves
        assert set(on[3]) == set(off[3]) | NEW_KEYS
        assert all(bits_equal(a, b) for a, b in zip(on[:3], off[:3])) and all(bits_equal(on[3][k], off[3][k]) for k in off[3])
        depth, acc, ex = on[0].cpu().numpy(), on[2].cpu().numpy(), {k: v.cpu().numpy() for k, v in on[3].items()}
        assert ex["depth_median"].shape == ex["median_index"].shape == ex["normals_valid"].shape == (H, W)
        assert ex["points"].shape == ex["normals"].shape == (H, W, 3)
        assert ex["median_index"].dtype == np.int32 and ex["normals_valid"].dtype == np.uint8
        # the median against the frame's own weights
        w, z = ex["weights"].reshape(H * W, -1), ex["z_vals"].reshape(H * W, -1)
        bad, ambiguous = ref.median_check(w, z, threshold, ex["median_index"].reshape(-1), ex["depth_median"].reshape(-1))
        assert bad.size == 0 and ambiguous <= 0.01, (surface, threshold, bad[:8], ambiguous)
        hits += int((ex["median_index"] >= 0).sum())
        assert (ex["median_index"] < 0).any()                         # (rays through empty space: every view has some)
        # the points: o + d * depth_surface, the product and the sum rounded separately
        surf = ex["depth_median"] if surface == "median" else depth
        assert ref.same_bits(ex["points"], (o + (d * surf[..., None]).astype(np.float32)).astype(np.float32)), surface
        # the normals against the restatement on the frame's own points and acc
        want_n, want_v = ref.point_normals(ex["points"], acc, d, ACC_MIN)
        assert ref.same_bits(ex["normals_valid"], want_v) and ref.same_bits(ex["normals"], want_n), surface
        usable = float((acc >= ACC_MIN).mean())
        print(f"{H}x{W} culled={culled} surface={surface} t={threshold}: usable {usable:.3f}, valid normals {want_v.mean():.3f}")
        # ACC_MIN and its two shares are the CPU oracle's, and the oracle renders the un-culled scene: the ball of the culled frames takes
        # density away, their acc is another field, and no reference states its shares — those frames are held to the restatement only
        if not culled:
            assert usable >= 0.2 and 1.0 - usable >= 0.2, usable
            assert 0 < want_v.sum() <= (acc >= ACC_MIN).sum()
            if threshold == THRESHOLD:                                # every usable ray has a crossing
                assert (ex["median_index"][acc >= ACC_MIN] >= 0).all()
        # whatever the chunking
        for chunk in (64, 37):
            again = frame(render, kw, H, W, K, chunk=chunk, **opts)
            assert all(bits_equal(a, b) for a, b in zip(on[:3], again[:3])) and all(bits_equal(on[3][k], again[3][k]) for k in on[3]), (surface, chunk)
    assert hits > 0
    # what is implied is formed and returned; what is not asked for is not
    only_n = frame(render, kw, H, W, K, rays=rays, normals=True, acc_min=ACC_MIN, median_threshold=THRESHOLD)
    assert set(only_n[3]) == (set(off[3]) - {"weights", "z_vals"}) | NEW_KEYS
    only_p = frame(render, kw, H, W, K, rays=rays.reshape(2, H * W, 3), points=True, surface="expected")     # a flat list of rays will do
    assert set(only_p[3]) == (set(off[3]) - {"weights", "z_vals"}) | {"points"} and only_p[3]["points"].shape == (H * W, 3)
    only_m = frame(render, kw, H, W, K, rays=rays, median=True)
    assert set(only_m[3]) == (set(off[3]) - {"weights", "z_vals"}) | {"depth_median", "median_index"}


def test_surface_buffers_of_a_coarse_only_frame_use_the_shared_row_of_depths():
    render, kw, _ = make_product(ARCH, 0, 4096, DEV, N_samples=16, N_importance=0)
    H, W = 8, 8
    K, _, rays = view(H, W)
    on = frame(render, kw, H, W, K, rays=rays, retweights=True, normals=True, acc_min=ACC_MIN, median_threshold=THRESHOLD)
    ex = {k: v.cpu().numpy() for k, v in on[3].items()}
    assert set(ex) == {"weights", "z_vals"} | NEW_KEYS
    bad, ambiguous = ref.median_check(ex["weights"].reshape(H * W, -1), ex["z_vals"].reshape(H * W, -1), THRESHOLD, ex["median_index"].reshape(-1),
                                      ex["depth_median"].reshape(-1))
    assert bad.size == 0 and ambiguous <= 0.01 and (ex["median_index"] >= 0).any()
    want_n, want_v = ref.point_normals(ex["points"], on[2].cpu().numpy(), rays[1].cpu().numpy(), ACC_MIN)
    assert ref.same_bits(ex["normals_valid"], want_v) and ref.same_bits(ex["normals"], want_n)


def read_png(path):
    """[H,W,3] uint8 of an 8-bit RGB PNG whose rows carry filter type 0 (what io.write_png writes)."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(raw):
        n, tag = struct.unpack(">I", raw[pos:pos + 4])[0], raw[pos + 4:pos + 8]
        body = raw[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            size = struct.unpack(">II", body[:8])
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h = size
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3)


def test_render_path_geometry_writes_its_frames_skips_them_and_returns_the_per_pose_renders(tmp_path):
    render, kw, _ = make_product(ARCH, 0, 4096, DEV, N_samples=16, N_importance=16)
    H, W = 16, 12
    K = synth.intrinsics(H, W)
    poses = [pose_spherical(a, 0.0, 16.0) for a in (25.0, -20.0)]
    bm, exp = codes()
    opts = dict(surface="median", acc_min=ACC_MIN, median_threshold=THRESHOLD)
    out = render.render_path_geometry(poses, (H, W, float(K[0][0])), K, 64, kw, expCodes=exp, shapeCodes=bm, savedir=str(tmp_path), **opts)
    assert out["rendered"] == [0, 1] and out["skipped"] == []
    names = sorted(f"{i:03d}_{what}.png" for i in (0, 1) for what in ("normals", "mask", "depth"))
    assert sorted(os.listdir(tmp_path)) == names
    for i, pose in enumerate(poses):
        depth, disp, acc, ex = render.render_geometry(H, W, K, chunk=1 << 20, c2w=pose[:3, :4], shapeCodes=bm, expType=20, expCodes=exp, normals=True,
                                                      **dict(kw, **opts))
        render.check_launches(block=True)
        want = dict(ex, depth=depth, disp=disp, acc=acc, depth_surface=ex["depth_median"])
        assert set(out) == set(want) | {"rendered", "skipped"}
        for k, v in want.items():
            assert ref.same_bits(out[k][i], v.cpu().numpy()), (i, k)
        usable = (acc >= ACC_MIN).cpu().numpy()
        valid = ex["normals_valid"].cpu().numpy()
        assert np.array_equal(read_png(tmp_path / f"{i:03d}_mask.png"), np.repeat((usable * 255).astype(np.uint8)[..., None], 3, -1))
        normals = read_png(tmp_path / f"{i:03d}_normals.png")
        want_img = (255 * np.clip(valid[..., None].astype(np.float32) * ((ex["normals"].cpu().numpy() + np.float32(1)) / np.float32(2)), 0, 1)).astype(np.uint8)
        assert np.array_equal(normals, want_img) and not normals[valid == 0].any()
        grey = read_png(tmp_path / f"{i:03d}_depth.png")
        want_grey = (255 * np.clip((ex["depth_median"].cpu().numpy() - np.float32(8.0)) / np.float32(18.0), 0, 1)).astype(np.uint8)
        assert np.array_equal(grey[..., 0], want_grey) and np.array_equal(grey[..., 0], grey[..., 1]) and np.array_equal(grey[..., 0], grey[..., 2])
    stamps = {n: os.stat(tmp_path / n).st_mtime_ns for n in names}
    again = render.render_path_geometry(poses, (H, W, float(K[0][0])), K, 64, kw, expCodes=exp, shapeCodes=bm, savedir=str(tmp_path), **opts)
    assert again == {"rendered": [], "skipped": [0, 1]}
    assert {n: os.stat(tmp_path / n).st_mtime_ns for n in names} == stamps
    os.remove(tmp_path / "001_depth.png")                             # an unfinished pose is rendered again, a finished one is not
    third = render.render_path_geometry(poses, (H, W, float(K[0][0])), K, 64, kw, expCodes=exp, shapeCodes=bm, savedir=str(tmp_path), **opts)
    assert third["rendered"] == [1] and third["skipped"] == [0] and ref.same_bits(third["normals"][0], out["normals"][1])
    assert sorted(os.listdir(tmp_path)) == names

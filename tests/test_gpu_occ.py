"""Occupancy-culled rendering on the GPU (``mofa_occ_*``, ``occupancy.py``, ``render_rays(..., occupancy=...)``).  Every comparison is
``torch.equal`` / ``np.array_equal``: the grid and the kept flags equal the NumPy restatement (tests/occ_reference.py), and a culled
frame equals the un-culled pipeline with the skipped samples' raw values replaced by zero, assembled from pieces that exist without the
feature (explicit points, ``run_network`` on all samples, ``mofa_composite_forward``, ``mofa_sample_pdf_merge``)."""
import numpy as np
import pytest
import torch

import occ_reference as occ
from harness import make_product
from mofanerf_amd import lib, mesh, occupancy, synth
from mofanerf_amd.rays import get_rays, pose_spherical

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARCH = (8, 64, 10, 64)
BALL = dict(centre=(0.3, -0.2, 0.5), radius=3.0, res=(33, 29, 37), bounds=((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0)))


@pytest.fixture(autouse=True)
def _shipped_launch_forms(monkeypatch):
    for k in ("MOFA_PIPE", "MOFA_CHAIN", "MOFA_FUSED", "MOFA_CHAIN_TRAIN"):
        monkeypatch.delenv(k, raising=False)
    lib.reload_env()
    lib.test_hooks()
    yield
    monkeypatch.undo()
    lib.reload_env()
    lib.test_hooks()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ball_occupancy(dilate=1, **over):
    b = dict(BALL, **over)
    res, lo, step = mesh.grid_spec(b["bounds"], b["res"])
    g = occ.ball_grid(res, lo, step, b["centre"], b["radius"])
    grid = occupancy.occupancy_from_grid(dev(g), 0.0, lo, step, dilate=dilate)
    return grid, occ.occupancy(g, 0.0, dilate), (res, lo, step)


def const_occupancy(value, bounds=((-40.0, -40.0, -40.0), (40.0, 40.0, 40.0)), res=(9, 9, 9)):
    """A grid whose every cell is occupied (value above the threshold 0) or empty (below)."""
    res, lo, step = mesh.grid_spec(bounds, res)
    return occupancy.occupancy_from_grid(torch.full(res, float(value), device=DEV), 0.0, lo, step, dilate=0)


def scene(H=16, angle=25.0):
    K = synth.intrinsics(H, H)
    ro, rd = get_rays(H, H, K, pose_spherical(angle, 0.0, 16.0), device=DEV)
    return K, ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()


def codes():
    bm, tex, exp = synth.codes(0)
    return bm.to(DEV), tex.to(DEV), exp.to(DEV)


def frame(render, kw, K, ro, rd, H=16, chunk=4096, **more):
    bm, tex, exp = codes()
    with torch.no_grad():
        out = render.render_fitting(H, H, K, chunk=chunk, rays=torch.stack([ro, rd], 0), shapeCodes=bm, uvCodes=tex, expType=20,
                                    expCodes=exp, **dict(kw, **more))
    render.check_launches(block=True)
    return out


# ---- 1. the grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dilate", [0, 1, 3])
def test_cells_equal_the_restatement_on_analytic_grids(dilate):
    res, lo, step = mesh.grid_spec(((-1.0, -1.5, -0.5), (1.0, 1.0, 1.5)), (21, 34, 17))          # non-cubic
    ax = [lo[a] + np.arange(res[a], dtype=np.float32) * step[a] for a in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    single = np.full(res, -1.0, np.float32)
    single[7, 30, 2] = 0.5
    corner = np.full(res, -1.0, np.float32)
    corner[0, 0, 0] = corner[20, 33, 16] = 0.5
    grids = {"ball": occ.ball_grid(res, lo, step, (0.1, -0.2, 0.4), 0.6), "slab": (0.2 - np.abs(y + 0.3)).astype(np.float32),
             "single": single, "corners": corner, "empty": np.full(res, -1.0, np.float32), "full": np.full(res, 1.0, np.float32),
             "ties": np.zeros(res, np.float32)}                                               # a sample AT the threshold is not above it
    for name, g in grids.items():
        got = occupancy.occupancy_from_grid(dev(g), 0.0, lo, step, dilate=dilate)
        want = occ.occupancy(g, 0.0, dilate)
        cells = got.cells()
        assert cells.dtype == torch.bool and tuple(cells.shape) == (20, 33, 16) and got.resolution == res
        assert np.array_equal(cells.cpu().numpy(), want), name
        assert got.fraction == pytest.approx(want.mean(), abs=1e-12) and got.dilate == dilate and got.threshold == 0.0
        assert np.array_equal(got.lo, lo) and np.array_equal(got.step, step)
    assert grids["ball"].max() > 0 and 0 < occ.occupancy(grids["ball"], 0.0, 0).mean() < 0.5
    assert occ.occupancy(single, 0.0, 0).sum() == 8 and not occ.occupancy(grids["ties"], 0.0, 3).any()
    bad = grids["ball"].copy()
    bad[3, 3, 3] = np.nan
    with pytest.raises(lib.MofaError, match="non-finite"):
        occupancy.occupancy_from_grid(dev(bad), 0.0, lo, step)


# ---- 2. the grid of two networks -----------------------------------------------------------------------------------------------------
def test_build_occupancy_is_the_union_of_the_networks_density_grids():
    render, kw, _ = make_product(ARCH, 0, 4096, DEV)
    bm, _, exp = codes()
    bounds, res = ((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0)), (17, 19, 15)
    nets = [kw["network_fn"], kw["network_fine"]]
    q = dict(bounds=bounds, resolution=res, shapeCodes=bm, expType=20, expCodes=exp)
    grids = [render.query_density(n, **q).cpu().numpy() for n in nets]
    both = np.concatenate([g.reshape(-1) for g in grids])
    thr = float(np.quantile(both, 0.9))                       # (a seeded network's density is speckle: pick a level that splits it)
    _, lo, step = mesh.grid_spec(bounds, res)
    for dilate in (0, 1):
        got = render.build_occupancy(nets, threshold=thr, dilate=dilate, netchunk=1000, **q)
        want = occ.occupancy(grids, thr, dilate)
        assert np.array_equal(got.cells().cpu().numpy(), want)
        assert np.array_equal(got.lo, lo) and np.array_equal(got.step, step)
    one = render.build_occupancy(nets[0], threshold=thr, dilate=0, **q)
    a, b = occ.occupancy(grids[0], thr, 0), occ.occupancy(grids[1], thr, 0)
    assert np.array_equal(one.cells().cpu().numpy(), a)
    assert 0 < a.sum() < a.size and (a | b).sum() > max(a.sum(), b.sum())           # the union is more than either
    with pytest.raises(TypeError):
        render.build_occupancy(nets, bounds=bounds, resolution=res, shapeCodes=bm)  # threshold has no default


# ---- 3. classify / compact through the C ABI -----------------------------------------------------------------------------------------
def _classify(ro, rd, vd, z, z_stride, S, cells_u8, res, lo, step):
    L, st = lib.load(), lib.stream()
    R = ro.shape[0]
    n = R * S
    flags = torch.full((R, S), 7, dtype=torch.uint8, device=DEV)
    ws = torch.empty(L.mofa_occ_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    counts = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    lib.check(L.mofa_occ_classify(lib.ptr(ro), lib.ptr(rd), lib.ptr(z), z_stride, R, S, cells_u8.data_ptr(), *res, mesh._f3(lo), mesh._f3(step),
                                  flags.data_ptr(), ws.data_ptr(), counts.data_ptr(), st), "mofa_occ_classify")
    n_kept = int(counts.cpu())
    pts = torch.full((n_kept, 3), float("nan"), device=DEV)
    dirs = torch.full((n_kept, 3), float("nan"), device=DEV)
    index = torch.full((n_kept,), -1, dtype=torch.int32, device=DEV)
    if n_kept:
        lib.check(L.mofa_occ_gather(lib.ptr(ro), lib.ptr(rd), lib.ptr(vd), lib.ptr(z), z_stride, R, S, flags.data_ptr(), ws.data_ptr(), n_kept,
                                    lib.ptr(pts), lib.ptr(dirs), index.data_ptr(), st), "mofa_occ_gather")
    return flags, ws, n_kept, pts, dirs, index


@pytest.mark.parametrize("per_ray_z", [False, True])
def test_classify_and_compact_equal_the_restatement(per_ray_z):
    res, lo, step = mesh.grid_spec(((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), (9, 11, 13))
    rng = np.random.default_rng(5)
    cells = rng.uniform(size=(8, 10, 12)) > 0.4
    cells[-1, :, :] = True                                                   # the cells behind the x = hi face
    S = 37
    o = np.float32([[0, 0, -3], [0.3, -0.2, -3], [1.0, 0, -3], [-1.0, 1.0, -3], [1.5, 0, -3], [0, -1.0000001, -3], [np.nan, 0, -3], [0, 0, -3]])
    d = np.float32([[0, 0, 1], [0.1, 0.05, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0]])   # enter, graze two faces, miss
    extra = 3000                                                             # several scan tiles (2048 samples each)
    o = np.concatenate([o, rng.uniform(-2, 2, (extra, 3)).astype(np.float32)])
    d = np.concatenate([d, rng.normal(size=(extra, 3)).astype(np.float32)])
    R = o.shape[0]
    z = rng.uniform(0, 6, (R, S)).astype(np.float32) if per_ray_z else np.linspace(0, 6, S, dtype=np.float32)
    vd = rng.normal(size=(R, 3)).astype(np.float32)
    want = occ.kept(o, d, z, lo, step, res, cells)
    assert want[0].any() and want[2].any() and not want[4].any() and not want[5].any() and not want[6].any() and 0.02 < want.mean() < 0.5
    flags, ws, n_kept, pts, dirs, index = _classify(dev(o), dev(d), dev(vd), dev(z), S if per_ray_z else 0, S, dev(cells.astype(np.uint8)),
                                                    res, lo, step)
    assert np.array_equal(flags.cpu().numpy().astype(bool), want) and int(flags.max()) == 1
    e = np.flatnonzero(want.reshape(-1))
    assert n_kept == len(e) and np.array_equal(index.cpu().numpy(), e.astype(np.int32))          # ascending and complete
    p = occ.points(o, d, z).reshape(-1, 3)[e]
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), p.view(np.uint32))
    assert np.array_equal(dirs.cpu().numpy().view(np.uint32), vd[e // S].view(np.uint32))
    # scatter: every element written; kept rows in place, zeros elsewhere
    raw_kept = torch.randn(n_kept, 4, device=DEV)
    raw = torch.full((R, S, 4), float("nan"), device=DEV)
    lib.check(lib.load().mofa_occ_scatter(lib.ptr(raw_kept), flags.data_ptr(), ws.data_ptr(), R * S, n_kept, lib.ptr(raw), lib.stream()),
              "mofa_occ_scatter")
    full = torch.zeros(R * S, 4, device=DEV)
    full[dev(e)] = raw_kept
    assert torch.equal(raw.reshape(-1, 4), full)
    again = _classify(dev(o), dev(d), dev(vd), dev(z), S if per_ray_z else 0, S, dev(cells.astype(np.uint8)), res, lo, step)
    assert torch.equal(again[0], flags) and torch.equal(again[5], index) and torch.equal(again[3], pts)


# ---- 4. the identity -----------------------------------------------------------------------------------------------------------------
def _composite(raw, z, rays_d, white):
    L = lib.load()
    R, S = raw.shape[0], raw.shape[1]
    o = {k: torch.empty(R, *sh, dtype=torch.float32, device=DEV) for k, sh in (("rgb", (3,)), ("disp", ()), ("acc", ()), ("depth", ()), ("weights", (S,)))}
    lib.check(L.mofa_composite_forward(lib.ptr(raw), lib.ptr(z), S, lib.ptr(rays_d), None, R, S, int(bool(white)), lib.ptr(o["rgb"]),
                                       lib.ptr(o["disp"]), lib.ptr(o["acc"]), lib.ptr(o["depth"]), lib.ptr(o["weights"]), lib.stream()),
              "mofa_composite_forward")
    return o


def _restated_frame(render, kw, ro, rd, z_coarse, cells, spec, perturb, white):
    """The un-culled pipeline with the skipped samples' raw values replaced by zero, from pieces that exist without the feature."""
    res, lo, step = spec
    L = lib.load()
    R, S, Ni = ro.shape[0], z_coarse.shape[1], int(kw["N_importance"])
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)

    def one_pass(net, z):
        pts = ro[:, None, :] + rd[:, None, :] * z[..., None]
        with torch.no_grad():
            raw = render.run_network(pts, vd, net)
        keep = dev(occ.kept(ro.cpu().numpy(), rd.cpu().numpy(), z.cpu().numpy(), lo, step, res, cells))
        assert np.array_equal(pts.cpu().numpy().view(np.uint32), occ.points(ro.cpu().numpy(), rd.cpu().numpy(), z.cpu().numpy()).view(np.uint32))
        raw = torch.where(keep[..., None], raw, torch.zeros_like(raw)).contiguous()
        return raw, keep, _composite(raw, z.contiguous(), rd, white)

    raw0, keep0, c = one_pass(kw["network_fn"], z_coarse)
    if perturb == 0.:
        u, us = torch.linspace(0., 1., steps=Ni).to(DEV), 0
    else:
        np.random.seed(0)
        u, us = torch.Tensor(np.random.rand(R, Ni)).to(DEV).contiguous(), Ni
    z_samples, z_fine, z_std = torch.empty(R, Ni, device=DEV), torch.empty(R, S + Ni, device=DEV), torch.empty(R, device=DEV)
    zc = z_coarse.contiguous()
    lib.check(L.mofa_sample_pdf_merge(lib.ptr(zc), S, lib.ptr(c["weights"]), lib.ptr(u), us, R, S, Ni, lib.ptr(z_samples), lib.ptr(z_fine),
                                      lib.ptr(z_std), lib.stream()), "mofa_sample_pdf_merge")
    raw1, keep1, f = one_pass(kw["network_fine"], z_fine)
    render.check_launches(block=True)
    return dict(rgb_map=f["rgb"], disp_map=f["disp"], acc_map=f["acc"], rgb0=c["rgb"], disp0=c["disp"], acc0=c["acc"], z_std=z_std, raw=raw1,
                _z_fine=z_fine, _weights0=c["weights"]), keep0, keep1


def _same(a, b):
    """torch.equal with NaN == NaN (disp is NaN where acc == 0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("white,perturb,lindisp", [(False, 0., False), (True, 0., False), (False, 1., False), (False, 0., True), (True, 1., True)])
def test_a_culled_frame_is_the_unculled_pipeline_with_skipped_samples_zeroed(white, perturb, lindisp):
    render, kw, _ = make_product(ARCH, 0, 4096, DEV)
    K, ro, rd = scene()
    R = ro.shape[0]
    grid, cells, spec = ball_occupancy(dilate=1)
    flags = dict(white_bkgd=white, perturb=perturb, pytest=True, lindisp=lindisp, retraw=True, verbose=True)
    plain = frame(render, kw, K, ro, rd, **flags)                         # (for the coarse sample positions: code the feature leaves alone)
    z_coarse = plain[3]["_z_coarse"].contiguous().clone()
    got = frame(render, kw, K, ro, rd, occupancy=grid, **flags)
    stats = dict(render.occupancy_stats)
    want, keep0, keep1 = _restated_frame(render, kw, ro, rd, z_coarse, cells, spec, perturb, white)
    share = float(keep0.float().mean())
    per_ray = keep0.any(-1)
    assert 0.1 < share < 0.9 and bool(per_ray.any()) and bool((~per_ray).any()), (share, int(per_ray.sum()))
    assert bool(keep1.any()) and not bool(keep1.all())
    ex = dict(got[3], rgb_map=got[0].reshape(-1, 3), disp_map=got[1].reshape(-1), acc_map=got[2].reshape(-1))
    assert _same(ex["_z_coarse"].reshape(R, -1), z_coarse)
    for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std", "raw", "_z_fine", "_weights0"):
        assert _same(ex[k].reshape(want[k].shape), want[k]), k
    assert stats == {"coarse": {"samples": keep0.numel(), "kept": int(keep0.sum())}, "fine": {"samples": keep1.numel(), "kept": int(keep1.sum())}}
    assert not _same(got[0], plain[0])                                     # the ball does cut density away: the culled frame differs


# ---- 5. / 6. all occupied, none occupied -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,H", [(ARCH, 16), ((8, 256, 10, 1024), 64)])
def test_an_all_occupied_grid_gives_the_unculled_frame_bit_for_bit(arch, H):
    render, kw, _ = make_product(arch, 0, 65536, DEV)
    K, ro, rd = scene(H)
    full = const_occupancy(1.0)
    assert full.fraction == 1.0
    a = frame(render, kw, K, ro, rd, H=H, chunk=2048)
    b = frame(render, kw, K, ro, rd, H=H, chunk=2048, occupancy=full)
    n = H * H
    assert render.occupancy_stats == {"coarse": {"samples": n * 64, "kept": n * 64}, "fine": {"samples": n * 128, "kept": n * 128}}
    for x, y in zip(a[:3], b[:3]):
        assert _same(x, y)
    for k in ("rgb0", "disp0", "acc0", "z_std"):
        assert _same(a[3][k], b[3][k]), k
    assert float(a[2].max()) > 0


@pytest.mark.parametrize("white", [False, True])
def test_an_empty_grid_renders_the_background_and_launches_no_network(white):
    import ctypes as C
    render, kw, _ = make_product((8, 512, 10, 512), 0, 4096, DEV)           # wide enough for the chained launch
    K, ro, rd = scene()
    empty = const_occupancy(-1.0)
    assert empty.fraction == 0.0 and not bool(empty.cells().any())
    frame(render, kw, K, ro, rd, white_bkgd=white)                          # un-culled: binds the networks and launches them
    hips = [render._hip(kw["network_fn"]), render._hip(kw["network_fine"])]
    before = [h.chained_launches() for h in hips]
    assert sum(before) > 0 or lib.chain_selfcheck() != 1       # (a device that failed the self-check takes per-layer launches)
    L = lib.load()
    lib.check(L.mofa_prof_begin(), "mofa_prof_begin")
    rgb, disp, acc, ex = frame(render, kw, K, ro, rd, white_bkgd=white, occupancy=empty, retraw=True)
    torch.cuda.synchronize()
    ms, calls, work = (C.c_double * lib.PROF_KINDS)(), (C.c_int64 * lib.PROF_KINDS)(), (C.c_double * lib.PROF_KINDS)()
    lib.check(L.mofa_prof_end(ms, calls, work), "mofa_prof_end")
    net_kinds = (0, 1, 2, 3, 4, 5, 6, 7, 11)                                  # every MFMA kernel kind; 8 .. 10 are the ray kernels
    assert all(calls[k] == 0 for k in net_kinds), list(calls)
    assert calls[8] + calls[9] >= 2 and calls[10] == 1                        # compositing and resampling still ran
    assert [h.chained_launches() for h in hips] == before
    assert render.occupancy_stats == {"coarse": {"samples": 256 * 64, "kept": 0}, "fine": {"samples": 256 * 128, "kept": 0}}
    assert torch.equal(acc, torch.zeros_like(acc)) and torch.equal(ex["acc0"], torch.zeros_like(acc).reshape(-1))
    assert torch.equal(rgb, torch.full_like(rgb, 1.0 if white else 0.0))
    assert torch.equal(ex["raw"], torch.zeros_like(ex["raw"]))


# ---- 7. chunkings --------------------------------------------------------------------------------------------------------------------
def test_culled_frames_do_not_depend_on_chunk_or_netchunk():
    render, kw, _ = make_product(ARCH, 0, 4096, DEV)
    K, ro, rd = scene()
    grid, cells, spec = ball_occupancy(dilate=1)
    base = frame(render, kw, K, ro, rd, chunk=4096, occupancy=grid, retraw=True)
    stats = dict(render.occupancy_stats)
    kept_coarse = stats["coarse"]["kept"]
    assert kept_coarse > 1000
    for chunk, netchunk in ((4096, kept_coarse - 1), (4096, 777), (4096, 1 << 20), (100, 4096), (37, 500), (1, 4096)):
        render.netchunk = netchunk                                           # kept_coarse - 1: the coarse pass leaves a sub-batch of one point
        out = frame(render, kw, K, ro, rd, chunk=chunk, occupancy=grid, retraw=True)
        assert render.occupancy_stats == stats, (chunk, netchunk)
        for x, y in zip(base[:3], out[:3]):
            assert _same(x, y), (chunk, netchunk)
        for k in ("rgb0", "acc0", "z_std", "raw"):
            assert _same(base[3][k], out[3][k]), (k, chunk, netchunk)


# ---- 8. render_path ------------------------------------------------------------------------------------------------------------------
def test_render_path_with_occupancy_writes_the_frames_rendered_one_by_one(tmp_path):
    render, kw, _ = make_product(ARCH, 0, 4096, DEV, with_tex=True)
    grid, _, _ = ball_occupancy(dilate=1)
    rng = np.random.default_rng(1)
    uv = torch.from_numpy(rng.uniform(0, 1, (1, 512, 512, 3)).astype(np.float32)).to(DEV).expand(2, -1, -1, -1)
    poses = torch.stack([pose_spherical(a, 0.0, 16.0) for a in (-30.0, 25.0)], 0)
    K = synth.intrinsics(16, 16)
    bm = synth.codes(0)[0].to(DEV).expand(2, -1)
    exp_type = torch.tensor([1, 5])
    hwf = [16, 16, float(K[0][0])]
    (tmp_path / "a").mkdir()
    with torch.no_grad():
        rgbs, _ = render.render_path(poses, hwf, K, 4096, dict(kw, occupancy=grid), uvMap=uv, expType=exp_type, savedir=str(tmp_path / "a"),
                                     shapeCodes=bm)
        plain, _ = render.render_path(poses, hwf, K, 4096, kw, uvMap=uv, expType=exp_type, shapeCodes=bm)
        for i in range(2):
            (tmp_path / f"b{i}").mkdir()
            render.render_path(poses[i:i + 1], hwf, K, 4096, dict(kw, occupancy=grid), uvMap=uv[i:i + 1], expType=exp_type[i:i + 1],
                               savedir=str(tmp_path / f"b{i}"), shapeCodes=bm[i:i + 1])
            one = render.render(16, 16, K, chunk=4096, c2w=poses[i][:3, :4], shapeCodes=bm[i:i + 1], uvMap=uv[i], expType=exp_type[i],
                                **dict(kw, occupancy=grid))[0]
            assert np.array_equal(one.cpu().numpy(), rgbs[i])
            assert (tmp_path / "a" / f"{i:03d}.png").read_bytes() == (tmp_path / f"b{i}" / "000.png").read_bytes()
    assert not np.array_equal(rgbs, plain)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_argument_and_none_changes_nothing():
    render, kw, _ = make_product(ARCH, 0, 4096, DEV)
    K, ro, rd = scene(8)
    grid, _, _ = ball_occupancy()
    bm, tex, exp = codes()
    rays = torch.stack([ro, rd], 0)
    call = lambda **more: render.render_fitting(8, 8, K, chunk=64, rays=rays, shapeCodes=bm, uvCodes=tex, expType=20, expCodes=exp, **dict(kw, **more))
    with torch.no_grad():
        a, b = call(), call(occupancy=None)
        for x, y in zip(a[:3], b[:3]):
            assert _same(x, y)
        assert render.occupancy_stats is None
        with pytest.raises(lib.MofaError, match="raw_noise_std"):
            call(occupancy=grid, raw_noise_std=1.0)
        with pytest.raises(lib.MofaError, match="occupancy"):
            call(occupancy=grid.cells())
        call(occupancy=grid)
        assert render.occupancy_stats["coarse"]["samples"] == 64 * 64
    with pytest.raises(lib.MofaError, match="occupancy.*inference only"):         # autograd on, and the codes ask for a gradient
        render.render_fitting(8, 8, K, chunk=64, rays=rays, shapeCodes=bm.clone().requires_grad_(True), uvCodes=tex, expType=20, expCodes=exp,
                              **dict(kw, occupancy=grid))
    with pytest.raises(lib.MofaError, match="occupancy.*inference only"):         # ... or the rays do (pose fitting)
        render.render_fitting(8, 8, K, chunk=64, rays=rays.clone().requires_grad_(True), shapeCodes=bm, uvCodes=tex, expType=20, expCodes=exp,
                              **dict(kw, occupancy=grid))
    if torch.cuda.device_count() > 1:
        other = occupancy.OccupancyGrid(grid._cells.to("cuda:1"), grid.resolution, grid.lo, grid.step, 0.0, 1, grid.fraction)
        with pytest.raises(lib.MofaError, match="occupancy.*lives on"), torch.no_grad():
            call(occupancy=other)
    cpu_grid = occupancy.OccupancyGrid(grid._cells.cpu(), grid.resolution, grid.lo, grid.step, 0.0, 1, grid.fraction)
    with pytest.raises(lib.MofaError, match="occupancy.*lives on"), torch.no_grad():
        call(occupancy=cpu_grid)
    render.rays = torch.cat([ro, rd, torch.full_like(ro[:, :1], 8.0), torch.full_like(ro[:, :1], 26.0), rd], -1).cpu()
    with pytest.raises(lib.MofaError, match="CPU"), torch.no_grad():
        render.render_rays([0, 64], occupancy=grid, **{k: v for k, v in kw.items() if k not in ("near", "far", "ndc", "use_viewdirs")})
    res, lo, step = mesh.grid_spec(BALL["bounds"], BALL["res"])
    with pytest.raises(lib.MofaError, match="CPU"):
        occupancy.occupancy_from_grid(torch.zeros(res), 0.0, lo, step)
    for d in (-1, 9):
        with pytest.raises(lib.MofaError, match="dilate"):
            occupancy.occupancy_from_grid(torch.zeros(res, device=DEV), 0.0, lo, step, dilate=d)
    with pytest.raises(lib.MofaError, match="threshold"):
        occupancy.occupancy_from_grid(torch.zeros(res, device=DEV), float("nan"), lo, step)


# ---- 10. launch forms ----------------------------------------------------------------------------------------------------------------
def test_culled_frames_are_the_same_under_per_layer_and_chained_launches(knob):
    arch = (8, 512, 10, 512)                                                 # wide enough for the chained launch
    K, ro, rd = scene()
    grid, _, _ = ball_occupancy(dilate=1)
    render, kw, _ = make_product(arch, 0, 4096, DEV)
    a = frame(render, kw, K, ro, rd, occupancy=grid, retraw=True)
    chained = render._hip(kw["network_fine"]).chained_launches()
    knob("MOFA_CHAIN", "0")
    render2, kw2, _ = make_product(arch, 0, 4096, DEV)
    b = frame(render2, kw2, K, ro, rd, occupancy=grid, retraw=True)
    assert (chained > 0 or lib.chain_selfcheck() != 1) and render2._hip(kw2["network_fine"]).chained_launches() == 0
    for x, y in zip(a[:3], b[:3]):
        assert _same(x, y)
    assert _same(a[3]["raw"], b[3]["raw"]) and float(a[2].max()) > 0

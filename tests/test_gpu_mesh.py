"""Geometry export on the GPU: grid points, the density-only network forward (``mofa_net_density`` / ``Renderer.query_density``) and the
marching-tetrahedra kernels (``mofa_iso_count`` / ``mofa_iso_emit`` / ``Renderer.extract_mesh``).

* grid points and meshes equal the NumPy restatement (tests/mt_reference.py) exactly: faces equal, vertices bit for bit;
* the density equals ``raw[..., 3]`` of the full forward bit for bit, under every launch form, whatever the texture code and view
  directions, whatever the chunk size;
* parity with the reference comes from the pinned KAT fixture (tests/golden/kat_run_network.npz, g9).
"""
import numpy as np
import pytest
import torch

import mt_reference as mt
from conftest import nan_equal_close
from mofanerf_amd import lib, mesh, synth
from mofanerf_amd.model import NeRF
from mofanerf_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _shipped_launch_forms(monkeypatch):
    """Start from the shipped launch forms whatever MOFA_* the surrounding run exports; tests set what they vary (``knob``)."""
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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(D, W, seed=1, netchunk=1024 * 64):
    render = Renderer(netchunk=netchunk, expCodesLen=30)
    render.idSpecificMod.load_state_dict(synth.style_state(0))
    for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(0)):
        dst.data[:] = src
    render = render.to(DEV).eval()
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, seed))
    return render, net.to(DEV)


def full_sigma(render, net, pts, bm, e, tex, vd):
    """raw[..., 3] of run_network (HipNet.forward_points) on the same points, with a texture code and view directions."""
    render.shapeCodes, render.expType, render.decoding_texCodes = bm, 20, tex
    render.expCodes_Sigma[20] = e
    with torch.no_grad():
        raw = render.run_network(pts[:, None, :], vd, net)
    render.check_launches(block=True)
    return raw[:, 0, 3]


# ---- grid points and marching tetrahedra against the NumPy restatement ---------------------------------------------------------------
def test_grid_points_equal_the_numpy_formula_bit_for_bit():
    res, lo, step = mesh.grid_spec(((-1.1, -0.7, -0.33), (0.9, 1.3, 0.41)), (37, 64, 51))
    n_all = res[0] * res[1] * res[2]
    first, n = n_all // 2 + 17, 40000                               # starts mid-slab, crosses several i-slabs
    out = torch.full((n, 3), float("nan"), device=DEV)
    mesh.grid_points(res, lo, step, first, n, out)
    want = mt.grid_points(res, lo, step)
    assert np.array_equal(bits(out.cpu().numpy()), bits(want[first:first + n]))
    whole = torch.empty(n_all, 3, device=DEV)
    mesh.grid_points(res, lo, step, 0, n_all, whole)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(want))


def _gpu_mesh(grid, level, lo, step):
    v, f = mesh.iso_surface(dev(grid), level, lo, step)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy()


@pytest.mark.parametrize("name,res,chi", [("sphere", (48, 64, 40), 2), ("torus", (70, 56, 33), 0), ("two_spheres", (81, 40, 44), 4)])
def test_marching_tets_equal_the_reference_on_analytic_fields(name, res, chi):
    lo, step = mt.cube_grid(res)
    g = mt.field(name, res, lo, step)
    v, f = _gpu_mesh(g, 0.0, lo, step)
    rv, rf = mt.marching_tets(g, 0.0, lo, step)
    assert len(f) > 500
    assert np.array_equal(f, rf)
    assert np.array_equal(bits(v), bits(rv))
    assert mt.is_closed_oriented_manifold(f) and mt.euler_characteristic(v, f) == chi and mt.signed_volume(v, f) > 0
    v2, f2 = _gpu_mesh(g, 0.0, lo, step)                            # no atomics: the same bytes again
    assert np.array_equal(f2, f) and np.array_equal(bits(v2), bits(v))


def test_marching_tets_equal_the_reference_with_ties_at_the_level():
    rng = np.random.default_rng(7)
    res = (29, 33, 21)
    g = rng.integers(0, 5, res).astype(np.float32)                   # integer values, integer level: many samples == level
    lo, step = mt.cube_grid(res, 2.0)
    v, f = _gpu_mesh(g, 2.0, lo, step)
    rv, rf = mt.marching_tets(g, 2.0, lo, step)
    assert (g == 2.0).sum() > 1000 and len(f) > 1000
    assert np.array_equal(f, rf) and np.array_equal(bits(v), bits(rv))


@pytest.mark.parametrize("value", [0.0, 2.0])
def test_marching_tets_empty_result(value):
    res = (9, 10, 11)
    lo, step = mt.cube_grid(res)
    v, f = _gpu_mesh(np.full(res, value, np.float32), 1.0, lo, step)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    ws = torch.empty(lib.load().mofa_iso_workspace_bytes(*res), dtype=torch.uint8, device=DEV)
    lib.check(lib.load().mofa_iso_count(lib.ptr(dev(np.full(res, value, np.float32))), *res, 1.0, ws.data_ptr(), counts.data_ptr(),
                                        lib.stream()), "mofa_iso_count")
    assert counts.tolist() == [0, 0]


# ---- the density-only forward against the full forward ------------------------------------------------------------------------------
@pytest.mark.parametrize("D,W,forms", [(8, 256, (("MOFA_FUSED", "0"),)), (8, 256, (("MOFA_FUSED", "1"),)), (8, 256, ()),
                                       (10, 1024, ()), (10, 1024, (("MOFA_CHAIN", "0"),))])
def test_density_equals_the_full_forward_bit_for_bit(D, W, forms, knob):
    for k, v in forms:
        knob(k, v)
    render, net = make(D, W)
    h = render._hip(net)
    bm, tex, e = [t.to(DEV) for t in synth.codes(3)]
    rng = np.random.default_rng(D + W)
    chained = W > 256 and dict(forms).get("MOFA_CHAIN") != "0"
    for n in (1, 255, 257, 200000):
        pts = dev(rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32))
        vd = torch.nn.functional.normalize(dev(rng.normal(size=(n, 3)).astype(np.float32)), dim=-1).contiguous()
        before = h.chained_launches()
        sigma = render.query_density(net, pts, shapeCodes=bm, expCodes=e)
        launched = h.chained_launches() - before
        assert sigma.shape == (n,) and not sigma.requires_grad
        want = full_sigma(render, net, pts, bm, e, tex, vd)
        assert torch.isfinite(sigma).all()
        assert torch.equal(sigma, want), (n, (sigma - want).abs().max().item())
        assert launched == (-(-n // render.netchunk) if chained else 0), launched
        w = h._verdict.cpu().tolist()
        assert w[0] == 0 and (not chained or w[3] == w[4] > 0), w      # every chained launch complete


def test_density_of_a_chained_launch_that_ended_incomplete_is_nan_and_loud():
    render, net = make(10, 1024)
    h = render._hip(net)
    bm, _, e = [t.to(DEV) for t in synth.codes(3)]
    pts = dev(np.random.default_rng(0).uniform(-1, 1, (4096, 3)).astype(np.float32))
    ref = render.query_density(net, pts, shapeCodes=bm, expCodes=e)
    lib.test_hooks(chain_spin_limit=1)                                # a dependency wait out of budget: the launch is abandoned
    with pytest.raises(lib.MofaError, match="did not complete"):
        render.query_density(net, pts, shapeCodes=bm, expCodes=e)
    lib.test_hooks()
    out = torch.empty(4096, device=DEV)
    lib.test_hooks(chain_spin_limit=1)
    with torch.no_grad():
        h.density_points(pts, out, render._fold_codes(net, torch.zeros(256, device=DEV)).clone())
    torch.cuda.synchronize()
    lib.test_hooks()
    assert torch.isnan(out).all()
    with pytest.raises(lib.MofaError, match="did not complete"):
        h.check_verdict(block=True)
    again = render.query_density(net, pts, shapeCodes=bm, expCodes=e)
    assert torch.equal(again, ref)


@pytest.mark.parametrize("D,W", [(8, 256), (10, 1024)])
def test_grid_density_conditioning_and_chunking(D, W):
    render, net = make(D, W)
    bm, tex, e = [t.to(DEV) for t in synth.codes(3)]
    bounds, res = ((-1.2, -1.0, -0.8), (1.0, 1.3, 0.9)), (17, 23, 19)
    grid = render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm, expCodes=e)
    assert grid.shape == res and torch.isfinite(grid).all()
    for chunk in (1000, 4097, 17 * 23 * 19):                          # the chunk size does not matter
        assert torch.equal(render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm, expCodes=e, netchunk=chunk), grid)
    with torch.enable_grad():                                         # inference only, whatever autograd says
        g2 = render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm.requires_grad_(True), expCodes=e)
    bm.requires_grad_(False)
    assert not g2.requires_grad and torch.equal(g2, grid)
    # the grid's points through the full forward with two texture codes and two sets of view directions: the same density
    _, lo, step = mesh.grid_spec(bounds, res)
    pts = dev(mt.grid_points(res, lo, step))
    rng = np.random.default_rng(1)
    for t in (tex, tex.flip(0) * 2.0 + 0.3):
        vd = torch.nn.functional.normalize(dev(rng.normal(size=(pts.shape[0], 3)).astype(np.float32)), dim=-1).contiguous()
        assert torch.equal(full_sigma(render, net, pts, bm, e, t, vd), grid.reshape(-1))
    # the shape code and the expression code do change it
    assert not torch.equal(render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm * 1.5 + 0.01, expCodes=e), grid)
    assert not torch.equal(render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm, expCodes=1.0 - e), grid)
    assert not torch.equal(render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm, expType=3, expCodes=e), grid)


@pytest.mark.parametrize("D,W", [(8, 64), (10, 64), (8, 96), (10, 128)])
def test_density_kat_golden(golden, D, W):
    """The sigma column of the reference's own run_network output on its KAT (fixture g9): explicit points, codes, expression slot."""
    g = golden("kat_run_network.npz")
    t = f"rn{D}x{W}"
    _, _, netchunk, wseed, exp_type = [int(v) for v in g[t + "_meta"]]
    render = Renderer(netchunk=netchunk, expCodesLen=30)
    render.idSpecificMod.load_state_dict(synth.style_state(0))
    for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(0)):
        dst.data[:] = src
    render = render.to(DEV).eval()
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, wseed, "kat"))
    net = net.to(DEV)
    pts = dev(g[t + "_pts"].reshape(-1, 3).astype(np.float32))
    sigma = render.query_density(net, pts, shapeCodes=dev(g[t + "_bm"].astype(np.float32)), expType=exp_type)
    err = nan_equal_close(sigma.cpu().numpy(), g[t + "_raw"][..., 3].reshape(-1), 2e-5, 1e-5)
    print(t, f"max abs err of sigma vs reference {err:.2e}")


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_extract_mesh_end_to_end(tmp_path, monkeypatch):
    render, net = make(10, 1024)
    bm, tex, e = [t.to(DEV) for t in synth.codes(3)]
    bounds, res = ((-1.0, -1.1, -0.9), (1.1, 0.9, 1.0)), (40, 48, 36)
    grid = render.query_density(net, bounds=bounds, resolution=res, shapeCodes=bm, expCodes=e)
    level = float(grid.median())
    seen = {}
    iso = mesh.iso_surface

    def spy(g, *a, **k):
        seen["grid"] = g.detach().clone()
        return iso(g, *a, **k)

    monkeypatch.setattr(mesh, "iso_surface", spy)
    verts, faces = render.extract_mesh(net, bounds=bounds, resolution=res, level=level, shapeCodes=bm, expCodes=e)
    assert torch.equal(seen["grid"], grid)
    _, lo, step = mesh.grid_spec(bounds, res)
    rv, rf = mt.marching_tets(seen["grid"].cpu().numpy(), level, lo, step)
    assert len(rf) > 100 and verts.dtype == torch.float32 and faces.dtype == torch.int32
    assert np.array_equal(faces.cpu().numpy(), rf) and np.array_equal(bits(verts.cpu().numpy()), bits(rv))
    v2, f2, rgb = render.extract_mesh(net, bounds=bounds, resolution=res, level=level, shapeCodes=bm, expCodes=e, uvCodes=tex, colors=True)
    assert torch.equal(v2, verts) and torch.equal(f2, faces)
    assert rgb.shape == verts.shape and torch.isfinite(rgb).all() and (rgb >= 0).all() and (rgb <= 1).all()
    path = str(tmp_path / "face.ply")
    mesh.write_ply(path, v2, f2, rgb)
    pv, pf, pc = mesh.read_ply(path)
    assert np.array_equal(pv, v2.cpu().numpy()) and np.array_equal(pf, f2.cpu().numpy())
    assert np.array_equal(pc, mesh.to8b(rgb.cpu().numpy()))
    bad = grid.clone()
    bad[3, 4, 5] = float("nan")
    with pytest.raises(lib.MofaError, match="non-finite"):
        mesh.iso_surface(bad, level, lo, step)

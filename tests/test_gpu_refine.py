"""Vertex refinement on the GPU (``mofa_iso_edge_ids`` / ``mofa_edge_*`` / ``mofa_fd_*``, ``mesh.refine_vertices`` /
``mesh.density_normals``, ``Renderer.extract_mesh(refine=, normals=)``).

* every kernel equals the NumPy restatement (tests/refine_reference.py) bit for bit, counters included, on inputs the CPU tests show
  to tell the kernels from their near misses;
* on the sharp ball the refined vertices and brackets equal the restatement driven by the same torch field, do not depend on the chunk,
  and obey the derived radial bound that the unrefined mesh misses by a factor above 4;
* through the network: nothing changes at ``refine=0``, faces never change, the dense and the narrow-band paths agree, every vertex stays
  on its edge, the brackets are the network's own densities, and the normals are the restatement's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mt_reference as mt
import refine_reference as rr
from mofanerf_amd import hipnet, lib, mesh, synth
from mofanerf_amd.model import NeRF
from mofanerf_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEVEL = 0.25                                                     # of the per-kernel inputs


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


def host(*ts):
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    return np.array_equal(bits(host(got) if torch.is_tensor(got) else got), bits(want))


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def counters():
    return torch.zeros(4, dtype=torch.int64, device=DEV), np.zeros(4, dtype=np.int64)


# ---- the kernels, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rr.KERNEL_SIZES)
def test_edge_points_and_place_equal_the_restatement(n):
    L, first = lib.load(), rr.KERNEL_FIRST
    lo, step = rr.kernel_grid()
    edges = rr.kernel_edges(n, n)
    t_lo, t_hi, s_lo, s_hi, _ = rr.kernel_brackets(n, n, LEVEL)
    d_edges, d_tlo, d_thi, d_slo, d_shi = (dev(a) for a in (edges, t_lo, t_hi, s_lo, s_hi))
    for mode in range(3):
        got, (cnt, want_cnt) = torch.full((n, 3), 7.0, device=DEV), counters()
        lib.check(L.mofa_edge_points(*rr.KERNEL_RES, f3(lo), f3(step), d_edges.data_ptr(), lib.ptr(d_tlo) if mode == 2 else None,
                                     lib.ptr(d_thi) if mode == 2 else None, first, n, mode, lib.ptr(got), cnt.data_ptr(), lib.stream()),
                  "mofa_edge_points")
        want = rr.edge_points(rr.KERNEL_RES, lo, step, edges, t_lo, t_hi, first, n, mode, np.full((n, 3), 7.0, dtype=np.float32), want_cnt)
        assert same_bits(got, want) and np.array_equal(host(cnt), want_cnt), mode      # (a refused edge's point keeps its 7.0)
        assert want_cnt[rr.REFUSED] == (7 if n >= 255 else 0)
    if n >= 255:                                                  # the upper ends are mofa_grid_points' bits, also where interpolating at t = 1 is not
        grid = torch.empty(int(np.prod(rr.KERNEL_RES)), 3, device=DEV)
        mesh.grid_points(rr.KERNEL_RES, lo, step, 0, grid.shape[0], grid)
        a, b, ok = rr.edge_ends(edges[first:first + n], rr.KERNEL_RES)
        flat = (b[:, 0] * rr.KERNEL_RES[1] + b[:, 1]) * rr.KERNEL_RES[2] + b[:, 2]
        upper = rr.edge_points(rr.KERNEL_RES, lo, step, edges, None, None, first, n, 1, np.zeros((n, 3), dtype=np.float32), np.zeros(4, dtype=np.int64))
        assert np.array_equal(bits(upper[ok]), bits(host(grid)[flat[ok]]))
    total = first + n
    got, (cnt, want_cnt) = torch.full((total, 3), 7.0, device=DEV), counters()
    lib.check(L.mofa_edge_place(*rr.KERNEL_RES, f3(lo), f3(step), d_edges.data_ptr(), lib.ptr(d_tlo), lib.ptr(d_thi), lib.ptr(d_slo), lib.ptr(d_shi),
                                LEVEL, total, lib.ptr(got), cnt.data_ptr(), lib.stream()), "mofa_edge_place")
    want = rr.edge_place(rr.KERNEL_RES, lo, step, edges, t_lo, t_hi, s_lo, s_hi, LEVEL, np.full((total, 3), 7.0, dtype=np.float32), want_cnt)
    assert same_bits(got, want) and np.array_equal(host(cnt), want_cnt)


@pytest.mark.parametrize("n", rr.KERNEL_SIZES)
def test_bracket_init_and_update_equal_the_restatement(n):
    L = lib.load()
    t_lo, t_hi, s_lo, s_hi, s_m = (a[:n].copy() for a in rr.kernel_brackets(n, n, LEVEL))
    s_a, s_b = s_lo.copy(), s_hi.copy()
    if n >= 255:                                                  # ends on one side of the level, the level itself, non-finite ends
        s_a[5], s_b[5] = LEVEL + 1, LEVEL + 2
        s_a[6], s_b[6] = LEVEL - 1, LEVEL - 2
        s_a[7], s_b[7] = LEVEL, LEVEL - 1                         # (s == level is inside: a crossing)
        s_a[8], s_b[9], s_b[10] = np.nan, np.inf, -np.inf
    out = [torch.full((n,), 7.0, device=DEV) for _ in range(4)]
    cnt, want_cnt = counters()
    d_sa, d_sb, d_sm = dev(s_a), dev(s_b), dev(s_m)                 # (held: a temporary's memory is the next allocation's)
    lib.check(L.mofa_edge_bracket_init(lib.ptr(d_sa), lib.ptr(d_sb), LEVEL, n, *(lib.ptr(o) for o in out), cnt.data_ptr(), lib.stream()),
              "mofa_edge_bracket_init")
    want = rr.bracket_init(s_a, s_b, LEVEL, want_cnt)
    assert all(same_bits(g, w) for g, w in zip(out, want)) and np.array_equal(host(cnt), want_cnt)
    if n >= 255:
        assert want_cnt[rr.NON_FINITE] == 3 and want_cnt[rr.NO_STRADDLE] >= 2
    br = [dev(a) for a in (t_lo, t_hi, s_lo, s_hi)]
    cnt, want_cnt = counters()
    lib.check(L.mofa_edge_bracket_update(lib.ptr(d_sm), LEVEL, n, *(lib.ptr(o) for o in br), cnt.data_ptr(), lib.stream()),
              "mofa_edge_bracket_update")
    want = rr.bracket_update(s_m, LEVEL, t_lo, t_hi, s_lo, s_hi, want_cnt)
    assert all(same_bits(g, w) for g, w in zip(br, want)) and np.array_equal(host(cnt), want_cnt)
    assert want_cnt[rr.NON_FINITE] == (3 if n >= 255 else 0)
    if n >= 255:                                                  # a non-finite midpoint leaves its bracket; both orders of (s_lo, s_hi) occur
        assert all(w[3] == o[3] for w, o in zip(want, (t_lo, t_hi, s_lo, s_hi)))
        assert (s_lo < s_hi).any() and (s_lo > s_hi).any() and (s_m == np.float32(LEVEL)).any()


@pytest.mark.parametrize("n", rr.KERNEL_SIZES)
def test_fd_points_and_normals_equal_the_restatement(n):
    L, first = lib.load(), rr.KERNEL_FIRST
    rng = np.random.default_rng(n)
    verts = rng.standard_normal((first + n, 3)).astype(np.float32)
    h = np.array([0.05, 0.07, 0.03], dtype=np.float32)
    got = torch.full((6 * n, 3), 7.0, device=DEV)
    d_verts = dev(verts)
    lib.check(L.mofa_fd_points(lib.ptr(d_verts), f3(h), first, n, lib.ptr(got), lib.stream()), "mofa_fd_points")
    assert same_bits(got, rr.fd_points(verts[first:], h))
    s = rng.standard_normal((n, 6)).astype(np.float32)
    s[0] = [1e-20, -1e-20, 3e-21, 0, 0, 1e-21]                    # a tiny gradient: the float64 norm does not underflow
    if n >= 255:
        s[3] = [1, 1, 2, 2, 3, 3]                                 # zero
        s[4, 2], s[5, 1] = np.nan, np.inf
    got, (cnt, want_cnt) = torch.full((n, 3), 7.0, device=DEV), counters()
    d_s = dev(s.reshape(-1))
    lib.check(L.mofa_fd_normals(lib.ptr(d_s), f3(h), n, lib.ptr(got), cnt.data_ptr(), lib.stream()), "mofa_fd_normals")
    want = rr.fd_normals(s.reshape(-1), h, want_cnt)
    assert same_bits(got, want) and np.array_equal(host(cnt), want_cnt)
    assert want_cnt[rr.ZERO_NORMAL] == (3 if n >= 255 else 0) and want[0].any()


@pytest.mark.parametrize("name", ("sphere", "torus", "two_spheres"))
def test_iso_edge_ids_equal_the_reference(name):
    res = (24, 31, 19)
    lo, step = mt.cube_grid(res)
    grid, level = mt.field(name, res, lo, step), 0.013
    verts, faces, ids = mesh.iso_surface(dev(grid), level, lo, step, edge_ids=True)
    want_v, want_f = mt.marching_tets(grid, level, lo, step)
    assert len(want_v) > 200 and ids.dtype == torch.int64
    assert np.array_equal(host(ids), rr.iso_edge_ids(grid, level))
    assert same_bits(verts, want_v) and np.array_equal(host(faces), want_f)
    plain = mesh.iso_surface(dev(grid), level, lo, step)
    assert len(plain) == 2 and torch.equal(plain[0], verts) and torch.equal(plain[1], faces)


# ---- mesh.refine_vertices on the sharp ball --------------------------------------------------------------------------------------------
def ball_host(p):
    """The torch field on the GPU, asked through host copies: what drives the restatement."""
    return host(rr.ball_torch(dev(p)))


@pytest.fixture(scope="module", params=rr.BALL_GRIDS, ids=lambda r: "x".join(map(str, r)))
def ball(request):
    res = request.param
    lo, step = mt.cube_grid(res)
    pts = torch.empty(int(np.prod(res)), 3, device=DEV)
    mesh.grid_points(res, lo, step, 0, pts.shape[0], pts)
    grid = rr.ball_torch(pts).reshape(res)
    verts, faces, ids = mesh.iso_surface(grid, 0.0, lo, step, edge_ids=True)
    want = {k: rr.refine(ball_host, host(ids), res, lo, step, 0.0, k) for k in (0, 1, 6, 20)}
    return dict(res=res, lo=lo, step=step, grid=grid, verts=verts, faces=faces, ids=ids, want=want)


def test_ball_edge_ids_equal_the_band_paths(ball):
    assert np.array_equal(host(ball["ids"]), rr.iso_edge_ids(host(ball["grid"]), 0.0))
    _, _, band_ids, _ = mesh.band_surface(rr.ball_torch, ball["res"], ball["lo"], ball["step"], 0.0, 4, 1000)
    assert np.array_equal(np.sort(host(band_ids)), host(ball["ids"]))


@pytest.mark.parametrize("k", (0, 1, 6, 20))
def test_ball_refinement_equals_the_restatement(ball, k):
    verts, stats = mesh.refine_vertices(rr.ball_torch, ball["ids"], ball["res"], ball["lo"], ball["step"], 0.0, k, 1000)
    want_v, want_br, want_cnt = ball["want"][k]
    V = len(want_v)
    assert V > 1000 and not want_cnt.any()
    assert same_bits(verts, want_v)
    assert all(same_bits(stats[name], w) for name, w in zip(("t_lo", "t_hi", "s_lo", "s_hi"), want_br))
    assert stats["evaluations"] == (2 + k) * V and stats["bracket_width"] == 2.0 ** -k
    if k == 0:
        assert torch.equal(verts, ball["verts"])


def test_ball_refinement_does_not_depend_on_the_chunk(ball):
    want_v, want_br, _ = ball["want"][6]
    for chunk in (7, 1000, 10 ** 6):
        calls = []

        def fn(p):
            calls.append(p.shape[0])
            return rr.ball_torch(p)

        verts, stats = mesh.refine_vertices(fn, ball["ids"], ball["res"], ball["lo"], ball["step"], 0.0, 6, chunk)
        assert same_bits(verts, want_v) and all(same_bits(stats[n], w) for n, w in zip(("t_lo", "t_hi", "s_lo", "s_hi"), want_br))
        assert max(calls) <= chunk and sum(calls) == stats["evaluations"]


def test_ball_refinement_obeys_the_radial_bound_the_plain_mesh_misses(ball):
    verts, _ = mesh.refine_vertices(rr.ball_torch, ball["ids"], ball["res"], ball["lo"], ball["step"], 0.0, 6, 1000)
    bound = rr.radial_bound(host(ball["ids"]), ball["res"], ball["lo"], ball["step"], 6)
    err, plain = rr.radial_error(host(verts)), rr.radial_error(host(ball["verts"]))
    print(f"{ball['res']}: k = 6 max radial error {err.max():.3e} (bound {bound.max():.3e}); unrefined {plain.max():.3e}")
    assert (err <= bound).all()
    assert plain.max() >= 4 * bound.max()


def test_ball_normals_equal_the_restatement_and_point_radially(ball):
    verts, _ = mesh.refine_vertices(rr.ball_torch, ball["ids"], ball["res"], ball["lo"], ball["step"], 0.0, 6, 1000)
    want, _ = rr.density_normals(ball_host, host(verts), ball["step"])
    for chunk in (5, 1000, 10 ** 6):
        calls = []

        def fn(p):
            calls.append(p.shape[0])
            return rr.ball_torch(p)

        normals, n_zero = mesh.density_normals(fn, verts, ball["step"], 0.5, chunk)
        assert n_zero == 0 and same_bits(normals, want) and max(calls) <= chunk and sum(calls) == 6 * len(want)
    radial = host(verts).astype(np.float64) - np.array(rr.BALL_C)
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    worst = rr.angle(host(normals), radial).max()
    print(f"{ball['res']}: largest angle between a density normal and the radial direction {worst:.5f} rad (allowed {rr.NORMAL_TOL:.5f})")
    assert worst <= rr.NORMAL_TOL


def test_a_density_that_changes_its_answer_is_refused(ball):
    args = (ball["ids"], ball["res"], ball["lo"], ball["step"], 0.0, 3, 10 ** 6)
    calls = []

    def second_call_differs(p):
        calls.append(len(p))
        return torch.ones(len(p), device=p.device) if len(calls) == 2 else rr.ball_torch(p)

    with pytest.raises(lib.MofaError, match="straddle"):
        mesh.refine_vertices(second_call_differs, *args)
    calls.clear()

    def third_call_is_nan(p):
        calls.append(len(p))
        d = rr.ball_torch(p)
        if len(calls) == 3:
            d[len(p) // 2] = float("nan")
        return d

    with pytest.raises(lib.MofaError, match="non-finite"):
        mesh.refine_vertices(third_call_is_nan, *args)
    bad = ball["ids"].clone()
    bad[3] = 7 * int(np.prod(ball["res"]))
    with pytest.raises(lib.MofaError, match="not edges"):
        mesh.refine_vertices(rr.ball_torch, bad, *args[1:])
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.refine_vertices(rr.ball_torch, ball["ids"].cpu(), *args[1:])


# ---- through the network ---------------------------------------------------------------------------------------------------------------
BOUNDS, RES = ((-1.0, -1.1, -0.9), (1.1, 0.9, 1.0)), (33, 41, 29)
RES_B8 = (33, 41, 25)                                             # bricks of 8 need (n - 1) % 8 == 0 on every axis: 29 samples cannot


def make(D=10, W=1024, seed=1, netchunk=1024 * 64):
    render = Renderer(netchunk=netchunk, expCodesLen=30)
    render.idSpecificMod.load_state_dict(synth.style_state(0))
    for dst, src in zip(render.expCodes_Sigma, synth.exp_sigma(0)):
        dst.data[:] = src
    render = render.to(DEV).eval()
    net = NeRF(D=D, W=W, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    net.load_state_dict(synth.nerf_state(D, W, seed))
    return render, net.to(DEV)


@pytest.fixture(scope="module")
def face():
    """The seeded network, its density grid and level, and the meshes every test below compares (computed once)."""
    render, net = make()
    bm, tex, e = [t.to(DEV) for t in synth.codes(3)]
    grid = render.query_density(net, bounds=BOUNDS, resolution=RES, shapeCodes=bm, expCodes=e)
    kw = dict(bounds=BOUNDS, resolution=RES, level=float(grid.median()), shapeCodes=bm, expCodes=e)
    out = dict(render=render, net=net, tex=tex, kw=kw, plain=render.extract_mesh(net, **kw), mesh={}, stats={})
    for k in (1, 8):
        out["mesh"][k] = render.extract_mesh(net, refine=k, **kw)
        out["stats"][k] = dict(render.mesh_stats)
    return out


def density(face, pts):
    return face["render"].query_density(face["net"], dev(pts), shapeCodes=face["kw"]["shapeCodes"], expCodes=face["kw"]["expCodes"])


def test_refine_zero_changes_nothing_and_faces_never_change(face):
    render, net, kw = face["render"], face["net"], face["kw"]
    verts, faces = face["plain"]
    assert len(faces) > 1000
    render.mesh_stats = None
    again = render.extract_mesh(net, refine=0, **kw)
    assert len(again) == 2 and torch.equal(again[0], verts) and torch.equal(again[1], faces) and render.mesh_stats is None
    for k in (1, 8):
        v, f = face["mesh"][k]
        assert torch.equal(f, faces) and v.shape == verts.shape and not torch.equal(v, verts)
        st = face["stats"][k]
        assert st["refine"]["evaluations"] == (2 + k) * len(verts) and st["edge_ids"].shape == (len(verts),)
    for bad in (-1, 21, 2.5):
        with pytest.raises(lib.MofaError, match="refine"):
            render.extract_mesh(net, refine=bad, **kw)
    with pytest.raises(lib.MofaError, match="normals"):
        render.extract_mesh(net, normals="vertex", **kw)


@pytest.mark.parametrize("brick,res", ((4, RES), (8, RES_B8)))
def test_dense_and_band_paths_refine_to_the_same_vertices(face, brick, res):
    render, net = face["render"], face["net"]
    kw = dict(face["kw"], resolution=res)
    dense_v, dense_f = face["mesh"][8] if res == RES else render.extract_mesh(net, refine=8, **kw)
    dense_ids = host(render.mesh_stats["edge_ids"]) if res != RES else host(face["stats"][8]["edge_ids"])
    band_v, band_f = render.extract_mesh(net, refine=8, brick=brick, **kw)
    band_ids = host(render.mesh_stats["edge_ids"])
    plain_v, plain_f = render.extract_mesh(net, brick=brick, **kw)
    assert torch.equal(plain_f, band_f) and len(band_ids) > 1000 and render.mesh_stats.get("refine") is None
    # the band holds every surface component that passes through a seeded brick: its vertices are the dense path's on the same edges
    order = np.argsort(band_ids, kind="stable")
    at = np.searchsorted(dense_ids, band_ids[order])
    assert (at < len(dense_ids)).all() and np.array_equal(dense_ids[at], band_ids[order])
    assert same_bits(host(band_v)[order], host(dense_v)[at])
    print(f"brick {brick} on {res}: {len(band_ids)} of the dense path's {len(dense_ids)} vertices")


def edge_geometry(ids):
    _, lo, step = mesh.grid_spec(BOUNDS, RES)
    a, b, ok = rr.edge_ends(ids, RES)
    assert ok.all()
    pa, pb = (np.stack([rr._coord(lo[c], step[c], q[:, c]) for c in range(3)], 1) for q in (a, b))
    return a, b, pa, pb, lo, step


@pytest.mark.parametrize("k", (1, 8))
def test_every_vertex_lies_on_its_edge(face, k):
    verts = host(face["mesh"][k][0]).astype(np.float64)
    _, _, pa, pb, _, _ = edge_geometry(host(face["stats"][k]["edge_ids"]))
    pa, pb = pa.astype(np.float64), pb.astype(np.float64)
    d = pb - pa
    ulp = 2.0 ** -23 * np.maximum(np.abs(pa), np.abs(pb)).max(1, keepdims=True)      # of the largest coordinate of the edge
    moving = d != 0
    t_axis = np.where(moving, (verts - pa) / np.where(moving, d, 1), np.nan)
    t = np.nanmean(t_axis, axis=1, keepdims=True)
    slack = 4 * ulp / np.abs(np.where(moving, d, np.inf)).min(1, keepdims=True)
    assert (t >= -slack).all() and (t <= 1 + slack).all()
    assert (np.abs(verts - (pa + t * d)) <= 4 * ulp).all()                             # collinear with the edge to a few ulp


@pytest.mark.parametrize("k", (1, 8))
def test_the_brackets_are_the_networks_densities_and_straddle_the_level(face, k):
    st, level = face["stats"][k], np.float32(face["kw"]["level"])
    a, b, pa, pb, lo, step = edge_geometry(host(st["edge_ids"]))
    r = {n: host(st["refine"][n]) for n in ("t_lo", "t_hi", "s_lo", "s_hi")}
    assert np.array_equal(r["t_hi"] - r["t_lo"], np.full(len(a), 2.0 ** -k, dtype=np.float32))
    for t, s in ((r["t_lo"], r["s_lo"]), (r["t_hi"], r["s_hi"])):
        p = rr._edge_point(a, b, lo, step, t)
        p = np.where((t == 0)[:, None], pa, np.where((t == 1)[:, None], pb, p))       # the ends themselves are the grid's points
        assert same_bits(density(face, p), s)
    assert (rr.inside(r["s_lo"], level) != rr.inside(r["s_hi"], level)).all()


def test_refinement_brings_the_density_at_the_vertices_to_the_level(face):
    level = face["kw"]["level"]
    off = {k: float((density(face, host(v)) - level).abs().max()) for k, (v, _) in (("plain", face["plain"]), (8, face["mesh"][8]))}
    print(f"max |density(vertex) - level|: unrefined {off['plain']:.3e}, refine = 8 {off[8]:.3e}")
    assert off[8] <= off["plain"]


def test_normals_and_the_unchained_launch_form(face, knob):
    render, net, kw = face["render"], face["net"], face["kw"]
    verts, faces, normals = render.extract_mesh(net, refine=8, normals="density", **kw)
    stats = dict(render.mesh_stats)
    assert torch.equal(verts, face["mesh"][8][0]) and torch.equal(faces, face["plain"][1])
    n = host(normals).astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    assert normals.shape == verts.shape and ((np.abs(length - 1) <= 2.0 ** -23) | (length == 0)).all()
    assert stats["zero_normals"] == int((length == 0).sum()) and stats["refine"]["evaluations"] == 10 * len(n)
    # the restatement from the network's densities at the six offset points
    _, _, step = mesh.grid_spec(BOUNDS, RES)
    h = (np.float32(0.5) * step).astype(np.float32)
    want = rr.fd_normals(host(density(face, rr.fd_points(host(verts), h))), h, np.zeros(4, dtype=np.int64))
    assert same_bits(normals, want)
    only = render.extract_mesh(net, normals="density", **kw)          # normals without refinement: the plain vertices
    assert len(only) == 3 and torch.equal(only[0], face["plain"][0]) and render.mesh_stats.get("refine") is None
    fv, ff, fn = render.extract_mesh(net, refine=8, normals="faces", **kw)
    # (vertex_normals sums a vertex's faces with index_add_, in no fixed order: unit vectors equal to a few ulp, not bit for bit)
    assert torch.equal(fv, verts) and torch.equal(ff, faces) and float((fn - mesh.vertex_normals(verts, faces)).abs().max()) <= 1e-5
    cv, cf, rgb, cn = render.extract_mesh(net, refine=8, normals="density", colors=True, uvCodes=face["tex"], **kw)
    assert torch.equal(cv, verts) and torch.equal(cn, normals)
    assert rgb.shape == verts.shape and torch.isfinite(rgb).all() and (rgb >= 0).all() and (rgb <= 1).all()
    knob("MOFA_CHAIN", "0")                                          # the per-layer launches give the same mesh
    uv, uf, un = render.extract_mesh(net, refine=8, normals="density", **kw)
    assert torch.equal(uv, verts) and torch.equal(uf, faces) and torch.equal(un, normals)


def test_a_non_finite_density_during_refinement_raises(face, monkeypatch):
    render, net, kw = face["render"], face["net"], face["kw"]
    real, calls = hipnet.HipNet.density_points, []

    def poisoned(self, pts, sigma_out, folded=None):
        out = real(self, pts, sigma_out, folded)
        calls.append(int(pts.shape[0]))
        if len(calls) == 4:                                           # the grid, the two ends, then the first midpoints
            sigma_out[len(sigma_out) // 3] = float("inf")
        return out

    monkeypatch.setattr(hipnet.HipNet, "density_points", poisoned)
    with pytest.raises(lib.MofaError, match="non-finite values at the bracket midpoints"):
        render.extract_mesh(net, refine=2, netchunk=2 ** 20, **kw)       # (one launch per round: the fourth is the first midpoints)
    assert calls[0] == int(np.prod(RES)) and len(calls) == 5 and len(set(calls[1:])) == 1

"""The NumPy restatement of the mesh ray casting (tests/ray_reference.py) judged without a GPU: its exact values on the cubes, its slab
walk against its own brute force on every grid, ``front`` and the watertightness tied to the winding number the project already
trusts, the catalogue's own conditions (a test cannot pass on rays that all miss), and every injected fault seen by ``mismatches``,
the comparison the GPU tests use.  Also the refusals of mesh.ray_cast / ray_bounds that need no GPU."""
import numpy as np
import pytest
import torch

import ray_reference as rr
import wind_reference as wr
from mofanerf_amd import lib, mesh

GRIDS = (1, 2, 7, 16, 32, (5, 9, 3), None)
WALK_RAYS = 120          # rays per catalogue member in the walk's matrix of grids, directions and sides


def args_of(case, n=None):
    return tuple(case[k][:n] if k in ("origins", "dirs") else case[k] for k in ("origins", "dirs", "verts", "faces"))


def default_grid(verts, faces):
    v = np.asarray(verts, dtype=np.float32)
    return mesh.default_dist_grid(v.min(0), v.max(0), len(faces))


def by_name(name):
    (case,) = [c for c in rr.catalogue() if c["name"] == name]
    return case


# ---- exact values -----------------------------------------------------------------------------------------------------------------------
def test_the_unit_cube_on_its_lattice_rays():
    verts, faces = wr.cube()
    o, d, inside = rr.cube_axis_rays()
    assert len(o) == 216 and 0 < inside.sum() < len(o)
    first, last = rr.brute_force(o, d, verts, faces), rr.brute_force(o, d, verts, faces, which="last")
    for res, t, front in ((first, 2.0, True), (last, 3.0, False)):
        assert np.array_equal(res["hit"], inside) and np.array_equal(res["face"] >= 0, inside)
        assert np.array_equal(res["t64"][inside], np.full(inside.sum(), t)) and np.array_equal(res["t"][inside], np.full(inside.sum(), t, np.float32))
        assert (res["front"][inside] == front).all() and not res["front"][~inside].any()
        assert np.isinf(res["t64"][~inside]).all() and np.isnan(res["bary"][~inside]).all() and np.isnan(res["point"][~inside]).all()
        assert np.array_equal(res["point"][inside], (o.astype(np.float64) + t * d)[inside].astype(np.float32))
        b = res["bary"][inside].astype(np.float64)
        assert (b >= 0).all() and np.array_equal(b.sum(1), np.ones(len(b)))
        tri = verts[faces[res["face"][inside]]].astype(np.float64)
        assert np.array_equal(np.einsum("nk,nkx->nx", b, tri).astype(np.float32), res["point"][inside])       # lattice weights are dyadic: exact
        assert res["counts"] == {"bad_rays": 0, "degenerate_faces": 0}
    # the first hit along +z lies on the -z quad (faces 8, 9), the last on the +z quad (10, 11); the quad's diagonal belongs to the lower face
    up = slice(4 * 36, 5 * 36)
    assert set(first["face"][up][inside[up]]) == {8, 9} and set(last["face"][up][inside[up]]) == {10, 11}


def test_equal_t_goes_to_the_lower_index_and_an_inward_cube_flips_front():
    two, inward = by_name("coincident_cubes"), by_name("inward_cube")
    for which in rr.WHICH:
        got = rr.brute_force(*args_of(two), which=which)
        one = rr.brute_force(two["origins"], two["dirs"], *wr.cube(), which=which)
        assert got["hit"].any() and np.array_equal(got["face"], one["face"]) and (got["face"] < 12).all()
        assert rr.mismatches(got, one) == []
        flipped = rr.brute_force(*args_of(inward), which=which)
        plain = rr.brute_force(inward["origins"], inward["dirs"], *wr.cube(), which=which)
        assert np.array_equal(flipped["t64"], plain["t64"]) and np.array_equal(flipped["front"][plain["hit"]], ~plain["front"][plain["hit"]])
    back = rr.brute_force(*args_of(inward), cull="back")                  # an inward cube seen from outside: the far side is its front
    assert np.array_equal(back["t64"][back["hit"]], np.full(back["hit"].sum(), 3.0)) and back["front"][back["hit"]].all()


def test_windows_include_both_ends():
    want = {"cube_window0": 3.0, "cube_window1": 2.0, "cube_window2": None, "cube_window3": 2.0, "cube_window4": 3.0, "cube_window5": None}
    for name, t in want.items():
        c = by_name(name)
        res = rr.brute_force(*args_of(c), c["t_min"], c["t_max"])
        inside = rr.cube_axis_rays()[2][:36]
        if t is None:
            assert not res["hit"].any()
        else:
            assert np.array_equal(res["hit"], inside) and (res["t64"][inside] == t).all()
    c = by_name("cube_window3")
    assert (rr.brute_force(*args_of(c), 2.0, 3.0, "last")["t64"][rr.cube_axis_rays()[2][:36]] == 3.0).all()


def test_bad_rays_and_the_sliver():
    c = by_name("bad_rays")
    res = rr.brute_force(*args_of(c))
    bad = rr.bad_rays(c["origins"].astype(np.float64), c["dirs"].astype(np.float64))
    assert bad.sum() == 6 == res["counts"]["bad_rays"] and np.isnan(res["t"][bad]).all() and np.isnan(res["t64"][bad]).all()
    assert (res["face"][bad] == -1).all() and not res["hit"][bad].any() and res["hit"][~bad].any()
    c = by_name("sliver")
    res = rr.brute_force(*args_of(c))
    assert list(res["hit"]) == [True, False, False, True, True] and list(res["t64"][[0, 3]]) == [5.0, 0.5]


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
def test_the_walk_equals_brute_force_on_every_grid():
    for c in rr.catalogue():
        a = args_of(c, WALK_RAYS)
        table = rr.pair_table(*a)
        grids = [g if g is not None else default_grid(c["verts"], c["faces"]) for g in GRIDS]
        for which in rr.WHICH:
            for cull in rr.CULL:
                want = rr.brute_force(*a, c["t_min"], c["t_max"], which, cull, table=table)
                for g in grids:
                    got = rr.grid_walk(*a, g, c["t_min"], c["t_max"], which, cull, table=table)
                    assert rr.mismatches(got, want) == [], (c["name"], which, cull, g, rr.mismatches(got, want))


def test_the_default_grid_tests_a_fraction_of_the_faces():
    for name in rr.FIELD_CASES:
        c = by_name(f"aimed_{name}")
        a = args_of(c, 200)
        table = rr.pair_table(*a)
        fine = rr.grid_walk(*a, default_grid(c["verts"], c["faces"]), table=table)["counts"]["face_tests"]
        brute = rr.grid_walk(*a, 1, table=table)["counts"]["face_tests"]
        assert brute == 200 * (len(c["faces"])) and 0 < fine < brute / 10, (name, fine, brute)


# ---- front and watertightness against the winding number --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("sphere", "torus"))
def test_signed_crossings_equal_the_winding_number(name):
    verts, faces, _, _ = wr.field_case(name)
    rng = np.random.default_rng(len(name))
    o = rng.uniform(-1.2, 1.2, (300, 3)).astype(np.float32)
    d = (rng.standard_normal((300, 3)) * rng.uniform(0.1, 10, (300, 1))).astype(np.float32)
    table = rr.pair_table(o, d, verts, faces)
    ok = rr.accepted(table, 0.0, np.inf, None)
    crossings = -(np.where(ok, table[1], 0).astype(np.int64)).sum(1)
    want = wr.brute_force(o, verts, faces, axis=2)["winding"]
    assert np.array_equal(crossings, want.astype(np.int64)) and 0 < (want != 0).sum() < 300
    assert not table[2].any()                                                     # the box rule refuses nothing here


def test_the_box_rule_is_what_keeps_the_walk_equal_to_brute_force():
    """Faces of size 2^-55 at the cube's corner, rays that pass them at up to 0.4: the edge functions' signs agree by rounding on some
    pairs.  Without the rule those are hits to brute force, which no walk visits; with it they are refused whatever the grid, and only
    the count of refused pairs a walk meets depends on the grid."""
    c = by_name("specks")
    a = args_of(c)
    table = rr.table_of(c)
    assert table[2].sum() > 100 and table[2].any(1).sum() > 10
    want = rr.brute_force(*a, table=table)
    assert (want["face"][want["hit"]] < 12).all()                                  # every hit is the cube's
    met = [rr.grid_walk(*a, g, table=table) for g in (1, 7, 16)]
    assert all(rr.mismatches(w, want) == [] for w in met)
    assert met[0]["counts"]["off_box"] == int(table[2].sum()) > met[1]["counts"]["off_box"] > met[2]["counts"]["off_box"] > 0
    loose = rr.pair_table(*a, faults={"no_box_rule"})
    brute = rr.brute_force(*a, faults={"no_box_rule"}, table=loose)
    assert (brute["face"] >= 12).any()                                             # a speck "hit" from far away
    assert rr.mismatches(rr.grid_walk(*a, 16, faults={"no_box_rule"}, table=loose), brute) != []


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------
def test_the_catalogue_is_complete_and_its_rays_hit_and_miss():
    cat = {c["name"]: c for c in rr.catalogue()}
    want = {"cube_axes", "cube_diagonals", "cube_surface", "cube_random_axis", "bad_rays", "degenerate", "sliver", "single", "coincident_cubes",
            "inward_cube", "slanted", "specks"} | {f"cube_window{k}" for k in range(6)} | {f"{kind}_{n}" for kind in ("aimed", "axes") for n in rr.FIELD_CASES}
    assert set(cat) == want
    sizes = [len(c["origins"]) for c in cat.values()]
    assert all(n % 64 for n in sizes) and {1, 63, 65} <= set(sizes) and any(900 <= n <= 1100 for n in sizes) and max(sizes) <= 1100
    assert all(len(c["faces"]) <= 6000 for c in cat.values())
    for c in cat.values():
        assert c["origins"].dtype == c["dirs"].dtype == c["verts"].dtype == np.float32 and c["faces"].dtype == np.int32
    for name in rr.FIELD_CASES:
        c = cat[f"aimed_{name}"]
        hit = rr.brute_force(*args_of(c), table=rr.table_of(c))["hit"].mean()
        assert 0.5 <= hit <= 0.8, (name, hit)
        norms = np.linalg.norm(c["dirs"], axis=1)
        assert norms.min() < 0.5 * norms.max()                                     # un-normalised
        c = cat[f"axes_{name}"]
        v = c["verts"].astype(np.float64)
        through = 0
        for o, d in zip(c["origins"].astype(np.float64), c["dirs"]):
            k = int(np.flatnonzero(d)[0])
            rest = [x for x in range(3) if x != k]
            through += bool(((v[:, rest] == o[rest]).all(1) & ((v[:, k] - o[k]) * d[k] > 0)).any())
        res = rr.brute_force(*args_of(c), table=rr.table_of(c))
        assert through >= 5 and 0 < res["hit"].sum() < len(res["hit"]), (name, through)
    deg = cat["degenerate"]
    assert rr.table_of(deg)[3] == 2 and rr.brute_force(*args_of(deg), table=rr.table_of(deg))["hit"].any()
    surf = rr.brute_force(*args_of(cat["cube_surface"]))
    assert surf["t64"][0] == 0.0 and not surf["hit"][4] and not surf["hit"][5] and surf["hit"][8:].all()      # on the surface, away, inside
    diag = rr.brute_force(*args_of(cat["cube_diagonals"]))
    assert diag["hit"].all()                                                       # corners and edges are hit, not passed between faces


# ---- injected faults --------------------------------------------------------------------------------------------------------------------
WALK_FAULT_GRIDS = {"no_slack": 49, "stop_first_hit": 7, "centroid_binning": 7}


@pytest.mark.parametrize("fault", rr.FAULTS)
def test_mismatches_sees_every_injected_fault(fault):
    seen = []
    for c in rr.catalogue():
        a = args_of(c, WALK_RAYS)
        for which in rr.WHICH:
            for cull in (None, "back"):
                want = rr.brute_force(*a, c["t_min"], c["t_max"], which, cull)
                if fault in WALK_FAULT_GRIDS:
                    got = rr.grid_walk(*a, WALK_FAULT_GRIDS[fault], c["t_min"], c["t_max"], which, cull, faults={fault})
                else:
                    got = rr.brute_force(*a, c["t_min"], c["t_max"], which, cull, faults={fault})
                if rr.mismatches(got, want):
                    seen.append((c["name"], which, cull))
        if seen:
            break
    assert seen, fault


def test_mismatches_is_bit_level_and_nan_aware():
    c = by_name("cube_axes")
    want = rr.brute_force(*args_of(c))
    assert rr.mismatches(want, want) == [] and rr.mismatches(want, want, rr.COUNTERS) == []
    for key in ("t", "t64", "bary", "point"):
        got = {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in want.items()}
        i = int(np.flatnonzero(want["hit"])[0])
        got[key].reshape(-1)[i * (got[key].size // len(want["hit"]))] = np.nextafter(got[key].reshape(-1)[i * (got[key].size // len(want["hit"]))], np.inf,
                                                                                   dtype=got[key].dtype)
        assert rr.mismatches(got, want) == [key]
    got = dict(want, t64=want["t64"].astype(np.float32))
    assert rr.mismatches(got, want) == ["t64"]
    got = dict(want, counts={"bad_rays": 1, "degenerate_faces": 0})
    assert rr.mismatches(got, want) == ["bad_rays"]


def test_ray_bounds_restated():
    c = by_name("cube_axes")
    b = rr.ray_bounds(*args_of(c), 0.5, 3.0625, 0.125)
    inside = rr.cube_axis_rays()[2]
    assert np.array_equal(b["hit"], inside) and b["near"].dtype == b["far"].dtype == np.float32
    assert (b["near"][inside] == 1.875).all() and (b["far"][inside] == 3.0625).all()          # t_last + margin = 3.125 is clipped to far
    assert (b["near"][~inside] == 0.5).all() and (b["far"][~inside] == 3.0625).all()
    b = rr.ray_bounds(*args_of(c), 0.5, 2.75, 0.125)                                         # the far side lies outside the window: the near side is the last hit
    assert np.array_equal(b["hit"], inside) and (b["far"][inside] == 2.125).all()
    b = rr.ray_bounds(*args_of(c), 0.0, 8.0, 0.25)
    assert (b["near"][inside] == 1.75).all() and (b["far"][inside] == 3.25).all()


# ---- refusals that need no GPU ----------------------------------------------------------------------------------------------------------
def test_refusals_before_anything_touches_the_gpu():
    verts, faces = (torch.from_numpy(x) for x in wr.cube())
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.ray_cast(o, d, verts, faces)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.ray_bounds(o, d, verts, faces, 0.0, 1.0, 0.1)
    assert "mofa_ray_query" in lib.SIGNATURES and mesh._RAY_COUNTS[0] == "degenerate_faces"

"""The NumPy restatement of the depth-map fusion (tests/fuse_reference.py) checked on its own, without a GPU:

* the exact scene's state and field equal their closed forms;
* frames streamed in batches give the bits of one call;
* every fault switch changes the field of at least one catalogue entry (so a GPU kernel with that mistake cannot equal the restatement);
* the three ``unobserved`` modes and the border behave as specified, and the field is finite;
* the sphere's quality CONDITION: every vertex of the marched field lies within one grid step of the sphere (carving on);
* the argument checks of ``mesh.tsdf_*`` that need no GPU raise ``MofaError``, CPU tensors included.
"""
import numpy as np
import pytest
import torch

import fuse_reference as fr
import mt_reference as mt
from mofanerf_amd import lib, mesh

CATALOGUE = fr.catalogue()
STATES = {c["name"]: fr.fuse(c) for c in CATALOGUE}              # computed once, never modified


def case_of(name):
    (c,) = [c for c in CATALOGUE if c["name"] == name]
    return c


def test_the_catalogue_holds_what_it_promises():
    names = [c["name"] for c in CATALOGUE]
    assert names == ["sphere", "exact", "non_cubic", "camera_inside", "depth_classes", "weights", "trunc_small", "trunc_large", "no_carving",
                     "view_order"]
    assert case_of("non_cubic")["res"] == (9, 17, 33) and len(set(case_of("non_cubic")["step"].tolist())) == 3
    d = case_of("depth_classes")["depth"]
    assert np.isnan(d).any() and np.isneginf(d).any() and (d == 0).any() and (d < 0).any() and np.isposinf(d).any() and (d > 0).any()
    assert (case_of("weights")["weight"] == 0).any()
    assert case_of("trunc_small")["trunc"] < case_of("trunc_small")["step"].min()
    assert case_of("trunc_large")["trunc"] > np.linalg.norm(case_of("trunc_large")["step"] * 14)
    assert not case_of("no_carving")["carve"] and len(case_of("camera_inside")["cams"]) == 1
    # the camera inside the volume: voxels behind it and voxels out of its frame
    c = case_of("camera_inside")
    x = fr.lattice(c["res"], c["lo"], c["step"])
    cam = c["cams"][0].astype(np.float64)
    p = (x - cam[4:].reshape(3, 4)[:, 3]) @ cam[4:].reshape(3, 4)[:, :3]
    t = -p[:, 2]
    u = cam[2] + cam[0] * p[:, 0] / np.where(t > 0, t, 1)
    assert (t <= 0).sum() > 100 and ((t > 0) & ((u < -0.5) | (u >= c["depth"].shape[2] - 0.5))).sum() > 100
    s = STATES["camera_inside"]
    assert (s["front"] > 0).any() and (s["front"][t <= 0] == 0).all() and (s["behind"][t <= 0] == 0).all()


def test_the_exact_scene_has_its_closed_form():
    c, s = case_of("exact"), STATES["exact"]
    acc, wsum, front, behind = fr.exact_expected()
    assert np.array_equal(s["acc"], acc) and np.array_equal(s["wsum"], wsum)
    assert np.array_equal(s["front"], front) and np.array_equal(s["behind"], behind)
    # per plane t = 1 .. 3 in steps of 1/4, frames D = 2 (w 1) and 2.25 (w 2), trunc 1/2: s = min((D - t) / 0.5, 1), behind where t > D + 0.5
    t = 3.0 - 0.25 * np.arange(9)                                     # z runs from -3 up to -1
    want_acc = {1.0: 3.0, 1.5: 3.0, 1.75: 2.5, 2.0: 1.0, 2.25: -0.5, 2.5: -2.0, 2.75: -2.0, 3.0: 0.0}
    want_wsum = {1.0: 3.0, 2.5: 3.0, 2.75: 2.0, 3.0: 0.0}
    plane = lambda a: a.reshape(c["res"])[0, 0]
    for tt, a in want_acc.items():
        assert plane(s["acc"])[list(t).index(tt)] == a, tt
    for tt, w in want_wsum.items():
        assert plane(s["wsum"])[list(t).index(tt)] == w, tt
    assert plane(s["behind"]).tolist() == [2, 1, 0, 0, 0, 0, 0, 0, 0] and plane(s["front"]).tolist() == [0, 1, 2, 2, 2, 2, 2, 2, 2]
    fld, counts = fr.field(s, c["res"], close_border=False)
    want = np.where(wsum > 0, -(acc / np.where(wsum > 0, wsum, 1)), 1.0).astype(np.float32).reshape(c["res"])
    assert fr.same_bits(fld, want)
    assert fld[4, 4].tolist()[7:] == [-1.0, -1.0] and fld[4, 4, 5] == np.float32(-2.5 / 3) and fld[4, 4, 1] == 1.0 and fld[4, 4, 0] == 1.0
    assert counts == {"observed": 8 * 81, "filled_inside": 81, "filled_outside": 0, "border": 0}


@pytest.mark.parametrize("name", [c["name"] for c in CATALOGUE])
def test_two_batches_give_the_bits_of_one(name):
    c = case_of(name)
    n = len(c["depth"])
    for batches in ([1] * n, [1, n - 1], [n - 1, 1]):
        s = fr.fuse(c, batches=[b for b in batches if b])
        assert all(fr.same_bits(s[k], STATES[name][k]) for k in ("acc", "wsum", "front", "behind")), (name, batches)


@pytest.mark.parametrize("fault", fr.FAULTS)
def test_every_fault_is_seen(fault):
    seen = []
    for c in CATALOGUE:
        good, _ = fr.field(STATES[c["name"]], c["res"], close_border=False)
        bad, _ = fr.field(fr.fuse(c, fault), c["res"], close_border=False, fault=fault)
        if not fr.same_bits(good, bad):
            seen.append(c["name"])
    assert seen, fault
    if fault == "reverse_views":          # the order of the views is visible in the FIELD where the sum cancels, and only there
        assert seen == ["view_order"]
    if fault == "no_weights":
        assert set(seen) == {"exact", "weights", "view_order"}
    if fault == "no_carve":
        assert "no_carving" not in seen and "sphere" in seen


def test_the_view_order_scene_loses_the_small_term_in_any_other_order():
    c = case_of("view_order")
    plane = list(3.0 - 0.25 * np.arange(9)).index(2.25)
    acc = STATES["view_order"]["acc"].reshape(c["res"])[:, :, plane]
    assert (acc == 0.25).all()
    assert (fr.fuse(c, "reverse_views")["acc"].reshape(c["res"])[:, :, plane] == 0.0).all()


@pytest.mark.parametrize("name", ["sphere", "camera_inside", "no_carving", "depth_classes"])
def test_field_modes_and_border(name):
    c, s = case_of(name), STATES[name]
    res = c["res"]
    n = int(np.prod(res))
    observed = (s["wsum"] > 0).reshape(res)
    only_behind = (~observed) & (s["behind"] > 0).reshape(res)
    never = (~observed) & (s["behind"] == 0).reshape(res)
    interior = np.zeros(res, bool)
    interior[1:-1, 1:-1, 1:-1] = True
    open_fields = {}
    for mode in fr.UNOBSERVED:
        fld, counts = fr.field(s, res, mode, close_border=False)
        open_fields[mode] = fld
        assert np.isfinite(fld).all() and fld.dtype == np.float32 and np.abs(fld).max() <= 1.0
        assert counts["observed"] + counts["filled_inside"] + counts["filled_outside"] == n and counts["border"] == 0
        assert counts["observed"] == observed.sum()
        closed, counts_closed = fr.field(s, res, mode, close_border=True)
        assert (closed[~interior] == -1).all() and fr.same_bits(closed[interior], fld[interior])
        assert counts_closed["border"] == n - (res[0] - 2) * (res[1] - 2) * (res[2] - 2)
        assert {k: v for k, v in counts_closed.items() if k != "border"} == {k: v for k, v in counts.items() if k != "border"}
    assert (open_fields["auto"][only_behind] == 1).all() and (open_fields["auto"][never] == -1).all()
    assert (open_fields["outside"][~observed] == -1).all() and (open_fields["inside"][~observed] == 1).all()
    for mode in fr.UNOBSERVED:
        assert fr.same_bits(open_fields[mode][observed], open_fields["auto"][observed])
    assert only_behind.any() and (never.any() or name == "sphere")          # (the sphere's eight views see every voxel)


def test_depth_frame_encodes_background_and_unknown():
    d = np.array([[1.5, 0.0, -2.0], [np.nan, 3.0, 4.0]], np.float32)
    m = np.array([[True, True, False], [True, False, True]])
    e = fr.depth_frame(d, m, "empty")
    assert e.dtype == np.float32 and e[0, 0] == 1.5 and e[0, 1] == 0.0 and np.isposinf(e[0, 2]) and np.isnan(e[1, 0]) and np.isposinf(e[1, 1])
    u = fr.depth_frame(d, m, "unknown")
    assert np.isnan(u[0, 2]) and np.isnan(u[1, 1]) and u[1, 2] == 4.0
    with pytest.raises(KeyError):
        fr.depth_frame(d, m, "white")


def test_the_sphere_lies_within_one_grid_step_with_carving():
    """The quality CONDITION of the fusion (not a measurement): on the sphere scene every vertex of the marched field — and every zero
    crossing of a lattice axis edge — lies within ONE grid step of the analytic sphere; a surface a full cell off is wrong.  The committed
    restatement gives max 0.947 step / median 0.143 step over the 8,826 vertices of the marching-tetrahedra mesh and max 0.716 / median 0.129
    over the 2,990 axis-edge crossings.  With background="unknown" the same frames leave the shadows between the views
    filled (max 14.0 steps on the axis edges): the condition applies to carving only."""
    c, s = case_of("sphere"), STATES["sphere"]
    fld, counts = fr.field(s, c["res"])
    assert counts["filled_outside"] == 0 and counts["filled_inside"] > 3000          # every voxel is seen; the core only from behind
    cross = fr.sphere_error(fr.crossings(fld, c["res"], c["lo"], c["step"]), c["step"])
    verts, faces = mt.marching_tets(fld, 0.0, c["lo"], c["step"])
    err = fr.sphere_error(verts, c["step"])
    print(f"sphere: axis-edge crossings n = {len(cross)} max {cross.max():.4f} median {np.median(cross):.4f} steps; "
          f"marched vertices n = {len(err)} max {err.max():.4f} median {np.median(err):.4f} steps")
    assert len(cross) > 2000 and cross.max() <= 1.0
    assert len(err) > 5000 and err.max() <= 1.0
    assert mt.is_closed_oriented_manifold(faces) and mt.euler_characteristic(verts, faces) == 2
    assert mt.signed_volume(verts, faces) > 0                                       # normals toward the outside
    assert abs(mt.signed_volume(verts, faces) / (4 / 3 * np.pi) - 1) < 0.05
    # without carving the background says nothing and the space between the views' shadows stays filled: far more than a step
    unknown = dict(c, depth=fr.depth_frame(c["depth"], np.isfinite(c["depth"]), "unknown"))
    fu, _ = fr.field(fr.fuse(unknown), c["res"])
    assert fr.sphere_error(fr.crossings(fu, c["res"], c["lo"], c["step"]), c["step"]).max() > 5.0


def _cpu_state(res=(3, 3, 3)):
    n = int(np.prod(res))
    return {"acc": torch.zeros(n, dtype=torch.float64), "wsum": torch.zeros(n, dtype=torch.float64), "front": torch.zeros(n, dtype=torch.int32),
            "behind": torch.zeros(n, dtype=torch.int32), "resolution": res, "lo": np.zeros(3, np.float32), "step": np.ones(3, np.float32),
            "trunc": 1.0, "frames": 0}


def test_cpu_tensors_and_bad_arguments_raise():
    lo, step = np.zeros(3, np.float32), np.ones(3, np.float32)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.tsdf_volume((4, 4, 4), lo, step, 0.5, device="cpu")
    for trunc in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(lib.MofaError, match="trunc"):
            mesh.tsdf_volume((4, 4, 4), lo, step, trunc)
    for res in ((1, 4, 4), (4, 4), (2048, 2048, 512), (2 ** 31, 2, 2)):
        with pytest.raises(lib.MofaError, match="tsdf_volume"):
            mesh.tsdf_volume(res, lo, step, 0.5)
    with pytest.raises(lib.MofaError, match="step"):
        mesh.tsdf_volume((4, 4, 4), lo, np.array([1, 0, 1], np.float32), 0.5)
    depth, K, pose = torch.ones(2, 3), np.eye(3, dtype=np.float32), np.eye(4, dtype=np.float32)[:3]
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.tsdf_integrate(_cpu_state(), depth, K, pose)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.tsdf_field(_cpu_state())
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.tsdf_surface(_cpu_state())
    with pytest.raises(lib.MofaError, match="state dict"):
        mesh.tsdf_integrate({"acc": None}, depth, K, pose)
    with pytest.raises(lib.MofaError, match="GPU"):
        mesh.depth_frame(depth, depth > 0)
    L = lib.load()
    assert L.mofa_tsdf_state_bytes(33, 33, 33) == 24 * 33 ** 3 and L.mofa_tsdf_state_bytes(2048, 2048, 512) == 0 == L.mofa_tsdf_state_bytes(1, 9, 9)
    assert L.mofa_tsdf_state_bytes(2047, 2048, 512) == 24 * 2047 * 2048 * 512
    assert L.mofa_tsdf_workspace_bytes(33, 33, 33) == 16 * ((33 ** 3 + 255) // 256) and L.mofa_tsdf_workspace_bytes(2, 2, 1) == 0
    f3 = (lib.C.c_float * 3)(0, 0, 0)
    assert L.mofa_tsdf_integrate(4, 4, 4, f3, f3, 0.5, None, None, 1, 2, 2, None, 1, 1, None, None, None, None, None) == -1
    assert b"null pointer" in L.mofa_last_error()
    for args, msg in (((1, 4, 4, f3, f3, 0.5, 1, None, 1, 2, 2, 1, 1, 1, 1, 1, 1, 1, None), b"2 samples"),
                      ((4, 4, 4, f3, f3, 0.0, 1, None, 1, 2, 2, 1, 1, 1, 1, 1, 1, 1, None), b"trunc"),
                      ((4, 4, 4, f3, f3, float("nan"), 1, None, 1, 2, 2, 1, 1, 1, 1, 1, 1, 1, None), b"trunc"),
                      ((4, 4, 4, f3, f3, 0.5, 1, None, 1, 65536, 32768, 1, 1, 1, 1, 1, 1, 1, None), b"H W"),
                      ((4, 4, 4, f3, f3, 0.5, 1, None, 0, 2, 2, 1, 1, 1, 1, 1, 1, 1, None), b"n_views"),
                      ((4, 4, 4, f3, f3, 0.5, 1, None, 3, 2, 2, 1, 2, 1, 1, 1, 1, 1, None), b"cameras")):
        assert L.mofa_tsdf_integrate(*args) == -1 and msg in L.mofa_last_error(), (msg, L.mofa_last_error())
    assert L.mofa_tsdf_field(4, 4, 4, 1, 1, 1, 3, 1, 1, 1, 1, None) == -1 and b"unobserved" in L.mofa_last_error()
    assert L.mofa_tsdf_field(4, 4, 4, 1, 1, 1, 0, 1, None, 1, 1, None) == -1 and b"null pointer" in L.mofa_last_error()

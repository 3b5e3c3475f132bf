"""The yardsticks of the mesh rasteriser hold each other up (no GPU): the NumPy restatement of the kernels' arithmetic
(tests/raster_reference.py: ``rasterize``) against an independent fp64 ray caster (``raycast``), and the proof that the comparison can
tell — each injected fault breaks it by a wide margin.

The conditions (``raster_reference.agreement``):

* pixels where the masks differ plus pixels where the face indices differ are at most 2 % of the covered pixels (samples within the snap
  distance, 1/512 px per axis, of an edge may fall to either side);
* at EVERY covered pixel the restatement's depth lies within the fp64 range of its own face's plane over the window
  ``(i +- 1/256, j +- 1/256)``, widened by 2^-22 relative: with the corners moved by at most 1/512 px per axis and 1/z affine on the screen,
  the rasterised 1/z at p is the exact one at a point within 1/512 px of p; the other half of the window covers the fp32 rounding of
  u, v and zc.

"A wide margin" for a fault: at least 10 % of the covered pixels disagree (five times the cap) or leave their window (none may)."""
import numpy as np
import pytest

import raster_reference as ref

WIDE = 0.10


def frames(scene, fault=None, **kw):
    s = dict(scene, **kw)
    rast = ref.rasterize(s["verts"], s["faces"], s["H"], s["W"], s["K"], s["c2w"], fault=fault)
    cast = ref.raycast(s["verts"], s["faces"], s["H"], s["W"], s["K"], s["c2w"])
    return rast, cast, ref.agreement(rast, cast, s["verts"], s["faces"], s["K"], s["c2w"])


SCENES = {"A": ref.scene_a, "B": ref.scene_b, "C": ref.scene_c, "B_first_pose": lambda: ref.scene_b((25.0, -20.0, 4.0)), "quad": ref.quad_scene,
          "quad_doubled": lambda: ref.quad_scene(doubled=True), "behind": ref.behind_scene}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_restatement_and_the_ray_caster_agree(name):
    scene = SCENES[name]()
    rast, cast, a = frames(scene)
    print(name, a, "counts", rast["counts"].tolist())
    assert a["covered"] >= 81
    assert a["disagree"] <= ref.DISAGREE_CAP, a
    assert a["outside"] == 0, a
    if name in ("A", "B", "B_first_pose"):
        stacks, slices = (12, 16) if name == "A" else (24, 32)
        assert len(scene["faces"]) == 2 * stacks * slices
        drawn, culled, degenerate, wave = rast["counts"].tolist()
        assert drawn + degenerate == 2 * stacks * slices and culled == wave == 0
        # the pole faces have no area; a sub-pixel face of scene B may snap onto a line as well
        assert degenerate == 2 * slices if name == "A" else 2 * slices <= degenerate <= 2 * slices + 8
        assert 0.1 < a["covered"] / (scene["H"] * scene["W"]) < 0.9                                     # a silhouette inside the image
    if name.startswith("quad"):                       # exact coordinates: nothing is within a snap of an edge, the two agree everywhere
        assert a["mask_diff"] == a["face_diff"] == 0 and a["covered"] == 81
    if name == "behind":
        assert rast["counts"].tolist() == [352, 1, 32, 0]


def test_the_restatements_own_invariants():
    s = ref.scene_a()
    attrs = np.random.default_rng(0).normal(size=(len(s["verts"]), 3)).astype(np.float32)
    r = ref.rasterize(s["verts"], s["faces"], s["H"], s["W"], s["K"], s["c2w"], attrs=attrs)
    hit = r["face"] >= 0
    assert r["depth"].dtype == r["bary"].dtype == r["normal"].dtype == r["attr"].dtype == np.float32 and r["face"].dtype == np.int32
    assert not r["depth"][~hit].any() and not r["bary"][~hit].any() and not r["normal"][~hit].any() and not r["attr"][~hit].any()
    assert (r["depth"][hit] > 2.5).all() and (r["depth"][hit] < 5.5).all()
    assert np.abs(r["bary"][hit].astype(np.float64).sum(-1) - 1).max() <= 3 * 2.0 ** -24 and (r["bary"][hit] >= 0).all()
    assert np.abs(np.linalg.norm(r["normal"][hit].astype(np.float64), axis=-1) - 1).max() < 1e-6
    d = ref.ray_dirs(s["H"], s["W"], s["K"], s["c2w"])
    assert ((r["normal"] * d).sum(-1)[hit] <= 1e-6).all()                       # turned to the camera
    # whichever path a face would take on the GPU, the frame is the same and only the fourth counter moves
    for wmp, wave in ((0, 352), (ref.INT32_MAX, 0)):
        again = ref.rasterize(s["verts"], s["faces"], s["H"], s["W"], s["K"], s["c2w"], attrs=attrs, wave_min_pixels=wmp)
        assert all(ref.same_bits(again[k], r[k]) for k in ("depth", "face", "bary", "normal", "attr"))
        assert again["counts"].tolist() == [352, 0, 32, wave]
    # reversed winding: the same coverage and faces
    rev = ref.rasterize(s["verts"], s["faces"][:, ::-1], s["H"], s["W"], s["K"], s["c2w"])
    assert np.array_equal(rev["face"], r["face"])
    assert np.abs(rev["depth"].view(np.int32).astype(np.int64) - r["depth"].view(np.int32)).max() <= 1


# which scene shows which fault: the sphere for what moves or bends the image, the exact quad for what happens ON an edge, the face behind
# the camera for the missing cull
FAULT_SCENES = {"affine": "A", "half_pixel": "A", "v_flip": "A", "swap_c": "A", "strict": "quad", "tie_high": "quad_doubled", "no_znear": "behind"}


def test_every_fault_is_listed():
    assert set(FAULT_SCENES) == set(ref.FAULTS)


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_an_injected_fault_breaks_the_checks_by_a_wide_margin(fault):
    scene = SCENES[FAULT_SCENES[fault]]()
    _, _, good = frames(scene)
    assert good["disagree"] <= ref.DISAGREE_CAP and good["outside"] == 0
    rast, cast, a = frames(scene, fault=fault)
    print(fault, a)
    # shares of the pixels the SOUND frame covers (a fault may cover more or fewer)
    assert max((a["mask_diff"] + a["face_diff"]) / good["covered"], a["outside"] / good["covered"]) >= WIDE, (fault, a)
    if fault == "strict":             # the crack: the diagonal through pixel centres is left uncovered
        n = 8
        assert all(rast["face"][2 + k, 2 + k] == -1 and cast[1][2 + k, 2 + k] == 0 for k in range(n + 1))
    if fault == "tie_high":
        assert (rast["face"][cast[1] >= 0] >= 2).all() and (cast[1][cast[1] >= 0] <= 1).all()

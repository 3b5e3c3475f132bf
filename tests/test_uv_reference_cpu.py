"""What the yardsticks of the UV texture baking (tests/uv_reference.py) must get right on their own, without a GPU: closed forms on the
quad, every grid against brute force, every fault switch visible somewhere in the catalogue, the atlas' geometry, the OBJ reader and
writer, and the argument refusals of the public calls that need no GPU."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import bake_reference as br
import uv_reference as uvr
from mofanerf_amd import lib, mesh

CATALOGUE = uvr.catalogue()
NAMES = [c["name"] for c in CATALOGUE]
MAPS = {(c["name"], s): uvr.texel_map(c["uvs"], c["uv_faces"], s, grid=1) for c in CATALOGUE for s in c["sizes"]}     # brute force, computed once


def case_of(name):
    (c,) = [c for c in CATALOGUE if c["name"] == name]
    return c


def same_map(a, b):
    return uvr.same_bits(a["face"], b["face"]) and uvr.same_bits(a["bary"], b["bary"]) and np.array_equal(a["index"], b["index"]) and \
        {k: v for k, v in a["counts"].items() if k != "face_tests"} == {k: v for k, v in b["counts"].items() if k != "face_tests"}


def test_closed_forms_on_the_quad():
    c = case_of("quad")
    for size in c["sizes"]:
        m = MAPS["quad", size]
        Ht, Wt = size
        assert m["covered"].all() and m["counts"]["covered"] == Ht * Wt and m["counts"]["multi"] == 0 and m["counts"]["degenerate"] == 0
        assert m["counts"]["faces_without_texels"] == 0
        assert np.abs(m["bary"].sum(-1) - 1.0).max() <= 4 * np.finfo(np.float64).eps
        points, normals = uvr.texel_surface(m, c["verts"], c["faces"])
        want = uvr.centres(size)
        assert np.abs(points[:, :2].astype(np.float64) - want).max() <= np.finfo(np.float32).eps and (points[:, 2] == 0).all()
        assert (normals == np.array([0, 0, 1], np.float32)).all()                 # D > 0: the flat normal of xy is +z
    m = MAPS["quad", (4, 4)]
    diagonal = [(i, 3 - i) for i in range(4)]                                     # u = v exactly: on the shared edge of the two faces
    for i, j in diagonal:
        assert m["face"][i, j] == 0 and (m["bary"][i, j] == 0).sum() == 1, (i, j, m["bary"][i, j])
    off = np.ones((4, 4), bool)
    for i, j in diagonal:
        off[i, j] = False
    assert (m["bary"][off] > 0).all()
    assert uvr.texel_map(c["uvs"], c["uv_faces"], (4, 4), fault="strict_inside")["counts"]["covered"] == 12
    assert (uvr.texel_map(c["uvs"], c["uv_faces"], (4, 4), fault="highest_face")["face"][[0, 1, 2, 3], [3, 2, 1, 0]] == 1).all()


def test_the_catalogue_holds_the_cases_it_names():
    sphere = case_of("sphere")
    assert len(sphere["uvs"]) > len(sphere["verts"])
    for size in sphere["sizes"]:
        m = MAPS["sphere", size]
        assert m["covered"].all() and m["counts"]["multi"] == 0 and m["counts"]["degenerate"] == 0, m["counts"]
    m = MAPS["mirrored", (8, 8)]
    mirrored = case_of("mirrored")
    assert m["counts"]["covered"] == 36 and m["counts"]["faces_without_texels"] == 0
    assert uvr.texel_map(mirrored["uvs"], mirrored["uv_faces"], (8, 8), fault="reject_mirrored")["counts"]["covered"] == 0
    m = MAPS["overlap", (8, 8)]
    assert m["counts"]["multi"] > 0 and m["face"].max() == 1 and m["counts"]["faces_without_texels"] == 2
    m = MAPS["degenerate", (8, 8)]
    assert m["counts"]["degenerate"] == 2 and set(np.unique(m["face"])) == {-1, 0} and m["counts"]["faces_without_texels"] == 2
    m = MAPS["outside", (8, 8)]
    assert m["covered"].all() and ((m["bary"] >= 0) & (m["bary"] < 0.75)).all()     # every texel well inside a chart four times the image
    m = MAPS["sliver", (8, 8)]
    assert m["counts"]["faces_without_texels"] == 1 and m["counts"]["degenerate"] == 0 and set(np.unique(m["face"])) == {-1, 0}


@pytest.mark.parametrize("name", NAMES)
def test_every_grid_equals_brute_force(name):
    c = case_of(name)
    q = uvr.random_queries(c, 300)
    brute = uvr.locate(q, c["uvs"], c["uv_faces"], grid=1)
    assert brute["counts"]["non_finite_queries"] == 4 and (brute["face"] >= 0).any()
    for grid in (None, 2, (3, 5), 64):
        got = uvr.locate(q, c["uvs"], c["uv_faces"], grid=grid)
        assert uvr.same_bits(got["face"], brute["face"]) and uvr.same_bits(got["bary"], brute["bary"]), (name, grid)
        assert {k: got["counts"][k] for k in ("degenerate", "non_finite_queries", "multi")} == \
            {k: brute["counts"][k] for k in ("degenerate", "non_finite_queries", "multi")}
        assert got["counts"]["face_tests"] <= brute["counts"]["face_tests"]
        for size in c["sizes"][:1]:
            assert same_map(uvr.texel_map(c["uvs"], c["uv_faces"], size, grid=grid), MAPS[name, size]), (name, size, grid)


def _outputs(c, size, fault):
    """Everything the restatement computes for one layout and size, with one fault."""
    m = uvr.texel_map(c["uvs"], c["uv_faces"], size, grid=1, fault=fault)
    out = [m["face"], m["bary"]]
    rng = np.random.default_rng(5)
    texture = rng.uniform(0, 1, size + (3,)).astype(np.float32)
    valid = m["covered"] & (rng.uniform(0, 1, size) < 0.6)
    out += list(uvr.dilate(texture, valid, 2, fault)[:2])
    H, W = 9, 11
    face = rng.integers(-1, len(c["uv_faces"]), (H, W)).astype(np.int32)
    bary = rng.dirichlet((1, 1, 1), (H, W)).astype(np.float32)
    out.append(uvr.sample(texture, face, bary, c["uvs"], c["uv_faces"], 0.25, fault))
    return out


def test_every_fault_switch_changes_some_output():
    base = {(c["name"], s): _outputs(c, s, None) for c in CATALOGUE for s in c["sizes"] if s[0] * s[1] <= 2048}
    for fault in uvr.FAULTS:
        changed = [key for key, want in base.items()
                   if any(not uvr.same_bits(a, b) for a, b in zip(_outputs(case_of(key[0]), key[1], fault), want))]
        assert changed, fault
    c = case_of("sphere")                                                         # index-ordered edges: the two faces of an edge disagree in rounding
    q = uvr.random_queries(c, 1000)
    assert not uvr.same_bits(uvr.locate(q, c["uvs"], c["uv_faces"], 1, "index_order_edges")["bary"], uvr.locate(q, c["uvs"], c["uv_faces"], 1)["bary"])


def test_the_texture_pipeline_and_its_bound_on_the_sphere():
    """The sphere scene of tests/bake_reference.py baked into a 64 x 128 texture through the restatement: every covered texel is coloured
    and within the bound at its own surface point; streamed 3 + 3 + 4 the state is the same bytes."""
    c = case_of("sphere")
    scene = br.sphere_scene()
    m = MAPS["sphere", (64, 128)]
    points, normals = uvr.texel_surface(m, c["verts"], c["faces"], c["normals"])
    texels = dict(scene, verts=points, normals=normals)
    state = br.bake(texels)
    again = br.bake(texels, batches=[3, 3, 4])
    assert all(uvr.same_bits(state[k], again[k]) for k in br.STATE_KEYS)
    bound, parts = uvr.interior_bound(c["verts"], c["faces"], c["normals"], scene["cams"], scene["depth_tol"], scene["cos_min"], br.SPHERE["H"],
                                      br.SPHERE["W"])
    want = br.sphere_field(points).astype(np.float64)
    for blend in ("mean", "best"):
        out = uvr.texture_image(state, m, blend, dilate_steps=1)
        assert out["counts"]["colored"] == m["counts"]["covered"] == 64 * 128 and out["valid"].all() and out["remaining"] == 0
        err = np.linalg.norm(out["texture"].reshape(-1, 3)[m["index"]].astype(np.float64) - want, axis=1)
        print(f"sphere texture, {blend}: max |colour - (A x + b)| = {err.max():.5f}, bound {bound:.5f}")
        assert err.max() <= bound, (blend, err.max(), bound)


def test_face_atlas_properties():
    for name in ("atlas_octahedron", "atlas_patch"):
        c = case_of(name)
        (size,) = c["sizes"]
        F = len(c["faces"])
        uvs, uv_faces, info = mesh.face_atlas(F, size)
        assert uvr.same_bits(uvs, c["uvs"]) and np.array_equal(uv_faces, c["uv_faces"]) and info["n"] == c["info"]["n"]      # mesh's closed form = the loop
        n, (h, w) = info["n"], info["cell"]
        assert n == int(np.ceil(np.sqrt(np.ceil(F / 2)))) and (h, w) == (size[0] / n, size[1] / n)
        x, y = uvs[:, 0].astype(np.float64) * size[1], (1.0 - uvs[:, 1].astype(np.float64)) * size[0]
        k = np.repeat(np.arange(F) // 2, 3)
        assert (x >= (k % n) * w + 0.999).all() and (x <= (k % n + 1) * w - 0.999).all()                # inside the cell, a padding from its border
        assert (y >= (k // n) * h + 0.999).all() and (y <= (k // n + 1) * h - 0.999).all()
        t = uvs[uv_faces].astype(np.float64)
        D = (t[:, 1, 0] - t[:, 0, 0]) * (t[:, 2, 1] - t[:, 0, 1]) - (t[:, 1, 1] - t[:, 0, 1]) * (t[:, 2, 0] - t[:, 0, 0])
        assert (D > 0).all()
        m = MAPS[name, size]
        assert m["counts"]["multi"] == 0 and m["counts"]["faces_without_texels"] == 0 and m["counts"]["degenerate"] == 0, m["counts"]
        # the two triangles of a cell are 2 padding apart: no texel centre within half a texel of one chart lies in the other's
        assert len(np.unique(m["face"][m["covered"]])) == F
    with pytest.raises(lib.MofaError, match="size = 10"):                         # 2 x 2 cells of 4 texels: 1 + (2 + sqrt 2) texels are needed
        mesh.face_atlas(8, 8)
    with pytest.raises(ValueError):
        uvr.face_atlas(8, 8)
    assert mesh.face_atlas(8, 10)[2]["min_size"] == 10
    assert mesh.face_atlas(7, 16)[0].shape == (21, 2) and mesh.face_atlas(0, 8)[0].shape == (0, 2)
    for bad, match in ((dict(n_faces=-1, size=16), "n_faces"), (dict(n_faces=2.5, size=16), "n_faces"), (dict(n_faces=8, size=0), "size"),
                       (dict(n_faces=8, size=(16, 16, 16)), "size"), (dict(n_faces=8, size=16, padding=-1.0), "padding"),
                       (dict(n_faces=8, size=16, padding=float("nan")), "padding"), (dict(n_faces=8, size=2 ** 16), "2\\^31")):
        with pytest.raises(lib.MofaError, match=match):
            mesh.face_atlas(**bad)


def _decode_png(path):
    """[H,W,3] uint8 of an 8-bit RGB PNG whose rows all use filter type 0 (what io.write_png writes)."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, shape = 8, b"", None
    while at < len(data):
        (n,), tag = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if tag == b"IHDR":
            w, h, depth, colour = struct.unpack(">IIBB", body[:10])
            assert (depth, colour) == (8, 2)
            shape = (h, w)
        elif tag == b"IDAT":
            idat += body
        at += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(shape[0], 1 + 3 * shape[1])
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(shape[0], shape[1], 3)


def test_obj_round_trips(tmp_path):
    c = case_of("sphere")
    verts, faces, uvs, uv_faces, normals = c["verts"], c["faces"], c["uvs"], c["uv_faces"], c["normals"]
    rng = np.random.default_rng(3)
    texture = rng.uniform(-0.2, 1.2, (6, 9, 3)).astype(np.float32)
    for with_vt, with_vn in ((False, False), (True, False), (False, True), (True, True)):
        path = str(tmp_path / f"m{int(with_vt)}{int(with_vn)}.obj")
        mesh.write_obj(path, verts, faces, uvs if with_vt else None, uv_faces if with_vt else None, normals if with_vn else None,
                       texture if with_vt else None)
        got = mesh.read_obj(path)
        assert uvr.same_bits(got["verts"], verts) and np.array_equal(got["faces"], faces) and got["faces"].dtype == np.int32
        if with_vt:
            assert uvr.same_bits(got["uvs"], uvs) and np.array_equal(got["uv_faces"], uv_faces)
            stem = path[:-4]
            assert got["mtllib"] == os.path.basename(stem) + ".mtl" and f"map_Kd {os.path.basename(stem)}.png" in open(stem + ".mtl").read()
            assert np.array_equal(_decode_png(stem + ".png"), mesh.to8b(texture))
        else:
            assert got["uvs"] is None and got["uv_faces"] is None and got["mtllib"] is None
        if with_vn:
            used = np.unique(faces)
            assert uvr.same_bits(got["normals"][used], normals[used])
        else:
            assert got["normals"] is None
    first = open(str(tmp_path / "m11.obj")).read().splitlines()
    assert [ln for ln in first if ln.startswith("f ")][0] == "f 1/1/1 17/18/17 2/2/2"
    path = str(tmp_path / "poly.obj")
    with open(path, "w") as fh:                                                   # a quad, a pentagon with relative indices, comments
        fh.write("# quad\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1 2/2 3/3 4/4\n"
                 "v 2 0 0 # fifth\nvt 0.5 0.5\nf -5/-5 -4/-4 -3/-3 -2/-2 -1/-1\nf -1 1 2\n")
    with pytest.raises(ValueError, match="with and faces without"):
        mesh.read_obj(path)
    text = open(path).read().replace("f -1 1 2\n", "")
    open(path, "w").write(text)
    got = mesh.read_obj(path)
    assert got["faces"].tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4]] and got["uv_faces"].tolist() == got["faces"].tolist()
    assert got["verts"].shape == (5, 3) and got["uvs"][4].tolist() == [0.5, 0.5] and got["normals"] is None
    for body, match in (("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2 3\n", "mixes"), ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", "outside"),
                        ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n", "outside"), ("v 0 0 0\nv 1 0 0\nf 1 2\n", "corners")):
        open(path, "w").write(body)
        with pytest.raises(ValueError, match=match):
            mesh.read_obj(path)
    with pytest.raises(ValueError, match="together"):
        mesh.write_obj(path, verts, faces, uvs=uvs)
    with pytest.raises(ValueError, match="texture"):
        mesh.write_obj(path, verts, faces, texture=texture)
    with pytest.raises(ValueError, match="Ht,Wt,3"):
        mesh.write_obj(path, verts, faces, uvs, uv_faces, texture=texture[..., :1])


def test_the_public_calls_refuse_cpu_tensors_and_bad_arguments_without_a_gpu():
    c = case_of("quad")
    uvs, uv_faces = torch.from_numpy(c["uvs"]), torch.from_numpy(c["uv_faces"])
    q = torch.zeros(4, 2, dtype=torch.float64)
    for call in (lambda: mesh.uv_locate(q, uvs, uv_faces), lambda: mesh.texel_map(uvs, uv_faces, 8),
                 lambda: mesh.sample_texture(torch.zeros(4, 4, 3), torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, 3), uvs, uv_faces),
                 lambda: mesh.dilate_texture(torch.zeros(4, 4, 3), torch.zeros(4, 4, dtype=torch.bool), 1)):
        with pytest.raises(lib.MofaError, match="GPU"):
            call()
    with pytest.raises(lib.MofaError, match="uvs"):
        mesh.texel_map(c["uvs"], uv_faces, 8)
    for tmap in (None, {}, {"face": 1}):
        with pytest.raises(lib.MofaError, match="texel_map"):
            mesh.texture_state(tmap)
        with pytest.raises(lib.MofaError, match="texel_map"):
            mesh.texel_surface(tmap, torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    assert mesh.default_uv_grid(0) == (1, 1) and mesh.default_uv_grid(384) == uvr.default_grid(384) == (10, 10)
    assert mesh.default_uv_grid(10 ** 9) == (256, 256)
    assert uvr.same_bits(mesh.texel_centres((5, 3), "cpu").numpy(), uvr.centres((5, 3)))

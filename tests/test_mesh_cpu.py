"""Geometry export without a GPU: the marching-tetrahedra rules (tests/mt_reference.py, the restatement the GPU kernels are held to)
on analytic fields, the PLY writer / reader, and the argument checks of the new C-ABI entry points (which refuse before any launch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mt_reference as mt
from mofanerf_amd import lib, mesh

RES = (64, 64, 64)


@pytest.fixture(scope="module")
def meshes():
    lo, step = mt.cube_grid(RES)
    out = {}
    for name in ("sphere", "torus", "two_spheres"):
        out[name] = mt.marching_tets(mt.field(name, RES, lo, step), 0.0, lo, step)
    return out


@pytest.mark.parametrize("name,chi", [("sphere", 2), ("torus", 0), ("two_spheres", 4)])
def test_reference_mesh_is_a_closed_oriented_manifold_of_the_right_topology(meshes, name, chi):
    verts, faces = meshes[name]
    assert len(faces) > 1000 and verts.dtype == np.float32 and faces.dtype == np.int32
    assert faces.min() == 0 and faces.max() == len(verts) - 1
    assert mt.is_closed_oriented_manifold(faces)
    assert mt.euler_characteristic(verts, faces) == chi
    assert mt.signed_volume(verts, faces) > 0                   # normals toward lower density: outward


def test_reference_sphere_volume_and_radius(meshes):
    verts, faces = meshes["sphere"]
    R = 0.6
    vol = mt.signed_volume(verts, faces)
    assert abs(vol / (4.0 / 3.0 * math.pi * R ** 3) - 1.0) < 0.02, vol
    r = np.linalg.norm(verts.astype(np.float64), axis=1)
    assert np.abs(r - R).max() < 2e-3


def test_reference_is_empty_when_nothing_crosses():
    lo, step = mt.cube_grid((5, 6, 7))
    for value in (0.0, 2.0):
        v, f = mt.marching_tets(np.full((5, 6, 7), value, np.float32), 1.0, lo, step)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_reference_orientation_follows_the_field_sign(meshes):
    """The complement {-sigma >= 0} is the same surface facing the other way: the same vertices (no ties on this field), a closed
    manifold whose signed volume is minus the sphere's (the two split a quad along different diagonals: equal up to those)."""
    lo, step = mt.cube_grid(RES)
    g = mt.field("sphere", RES, lo, step)
    v, f = mt.marching_tets(-g, 0.0, lo, step)
    v0, f0 = meshes["sphere"]
    assert np.array_equal(v, v0) and len(f) == len(f0)
    assert mt.is_closed_oriented_manifold(f)
    vol, vol0 = mt.signed_volume(v, f), mt.signed_volume(v0, f0)
    assert vol < 0 and abs(vol + vol0) < 1e-3 * vol0


def test_grid_spec_is_float32_host_arithmetic():
    res, lo, step = mesh.grid_spec(((-1, -0.5, 0.1), (1, 0.5, 0.7)), (37, 64, 51))
    assert res == (37, 64, 51) and lo.dtype == step.dtype == np.float32
    want = (np.float32([1, 0.5, 0.7]) - np.float32([-1, -0.5, 0.1])) / (np.float32([37, 64, 51]) - np.float32(1))
    assert np.array_equal(step, want.astype(np.float32))
    with pytest.raises(lib.MofaError):
        mesh.grid_spec(((0, 0, 0), (1, 1, 1)), (1, 4, 4))
    with pytest.raises(lib.MofaError):
        mesh.grid_spec(((0, 0, 0), (1, -1, 1)), (4, 4, 4))


@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_round_trip(tmp_path, meshes, with_colors):
    verts, faces = meshes["torus"]
    rgb = np.random.default_rng(0).uniform(-0.2, 1.2, verts.shape).astype(np.float32) if with_colors else None
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, torch.from_numpy(verts), torch.from_numpy(faces), None if rgb is None else torch.from_numpy(rgb))
    v, f, c = mesh.read_ply(path)
    assert np.array_equal(v, verts) and np.array_equal(f, faces)
    if with_colors:
        assert c.dtype == np.uint8 and np.array_equal(c, (255 * np.clip(rgb, 0, 1)).astype(np.uint8))
    else:
        assert c is None
    head = open(path, "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"property list uchar int vertex_indices" in head
    mesh.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v, f, c = mesh.read_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c is None


def _f3(*v):
    return (C.c_float * 3)(*v)


def test_geometry_entry_points_validate_before_launching():
    L = lib.load()
    ws, grid, out = 1, 1, 1                                       # (never dereferenced: every call below is refused first)
    lo, step = _f3(-1, -1, -1), _f3(0.1, 0.1, 0.1)
    # workspace size: 0 for a refused grid
    assert L.mofa_iso_workspace_bytes(8, 9, 10) > 8 * 9 * 10 * 7 * 9
    assert L.mofa_iso_workspace_bytes(1, 9, 10) == 0
    assert L.mofa_iso_workspace_bytes(1300, 1300, 1300) == 0
    # fewer than 2 samples on an axis
    for shape in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4)):
        assert L.mofa_iso_count(grid, *shape, 0.0, ws, out, None) == lib_einval()
        assert b"at least 2 samples" in L.mofa_last_error()
        assert L.mofa_iso_emit(grid, *shape, lo, step, 0.0, ws, out, out, None) == lib_einval()
    # a non-finite level
    for level in (float("nan"), float("inf"), -float("inf")):
        assert L.mofa_iso_count(grid, 4, 4, 4, level, ws, out, None) == lib_einval()
        assert b"level" in L.mofa_last_error()
        assert L.mofa_iso_emit(grid, 4, 4, 4, lo, step, level, ws, out, out, None) == lib_einval()
    # null pointers
    assert L.mofa_iso_count(None, 4, 4, 4, 0.0, ws, out, None) == lib_einval()
    assert L.mofa_iso_count(grid, 4, 4, 4, 0.0, None, out, None) == lib_einval()
    assert L.mofa_iso_count(grid, 4, 4, 4, 0.0, ws, None, None) == lib_einval()
    assert b"null pointer" in L.mofa_last_error()
    for i in range(6):
        args = [grid, lo, step, ws, out, out]
        args[i] = None
        g, lo_, st_, w_, v_, f_ = args
        assert L.mofa_iso_emit(g, 4, 4, 4, lo_, st_, 0.0, w_, v_, f_, None) == lib_einval()
    # an oversized grid: 7 nx ny nz >= 2^31
    n = int(math.ceil((2 ** 31 / 7) ** (1 / 3))) + 1
    assert L.mofa_iso_count(grid, n, n, n, 0.0, ws, out, None) == lib_einval()
    assert b"too large" in L.mofa_last_error()
    assert L.mofa_iso_count(grid, 2 ** 40, 2, 2, 0.0, ws, out, None) == lib_einval()
    assert L.mofa_iso_emit(grid, n, n, n, lo, step, 0.0, ws, out, out, None) == lib_einval()
    # emit: the grid geometry must be finite with positive steps
    assert L.mofa_iso_emit(grid, 4, 4, 4, lo, _f3(0.1, 0.0, 0.1), 0.0, ws, out, out, None) == lib_einval()
    assert L.mofa_iso_emit(grid, 4, 4, 4, _f3(float("nan"), 0, 0), step, 0.0, ws, out, out, None) == lib_einval()
    # grid points
    assert L.mofa_grid_points(4, 4, 4, lo, step, 0, 64, None, None) == lib_einval()
    assert L.mofa_grid_points(4, 4, 4, None, step, 0, 64, out, None) == lib_einval()
    assert L.mofa_grid_points(4, 4, 4, lo, step, 10, 55, out, None) == lib_einval()          # past the last point
    assert L.mofa_grid_points(0, 4, 4, lo, step, 0, 1, out, None) == lib_einval()
    # the density form
    s = lib.NetShape(10, 1024)
    assert L.mofa_net_density(s, None, 1, 1, 100, 1, 1, None, None) == lib_einval()
    assert L.mofa_net_density(s, 1, 1, 1, 100, 1, None, None, None) == lib_einval()
    assert b"null pointer" in L.mofa_last_error()
    assert L.mofa_net_density(s, 1, 1, 1, 0, 1, 1, None, None) == lib_einval()
    assert L.mofa_net_density(lib.NetShape(3, 256), 1, 1, 1, 100, 1, 1, None, None) == lib_einval()
    assert L.mofa_abi_version() == 5


def lib_einval():
    return -1                                                     # MOFA_EINVAL


def test_density_and_mesh_refuse_the_cpu():
    from mofanerf_amd import synth
    from mofanerf_amd.model import NeRF
    from mofanerf_amd.renderer import Renderer
    render = Renderer(expCodesLen=30)
    net = NeRF(D=8, W=64, input_ch=93, input_ch_views=27, input_ch_textureCodes=256, input_ch_shapeCodes=50, use_viewdirs=True)
    bm, tex, e = synth.codes(0)
    with pytest.raises(lib.MofaError):
        render.query_density(net, torch.zeros(10, 3), shapeCodes=bm, expCodes=e)
    with pytest.raises(lib.MofaError):
        render.query_density(net, bounds=((0, 0, 0), (1, 1, 1)), resolution=(4, 4, 4), shapeCodes=bm, expCodes=e)
    with pytest.raises(lib.MofaError):
        render.extract_mesh(net, bounds=((0, 0, 0), (1, 1, 1)), resolution=(4, 4, 4), level=None, shapeCodes=bm, expCodes=e)
    with pytest.raises(lib.MofaError):
        render.extract_mesh(net, bounds=((0, 0, 0), (1, 1, 1)), resolution=(4, 4, 4), level=0.0, shapeCodes=bm, expCodes=e, colors=True)
    with pytest.raises(lib.MofaError):
        mesh.iso_surface(torch.zeros(4, 4, 4), 0.0, np.zeros(3, np.float32), np.ones(3, np.float32))

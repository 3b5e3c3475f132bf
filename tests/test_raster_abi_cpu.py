"""The rasteriser's entry points without a GPU: sizes, refusals and their messages (no kernel is launched for a refused argument), and
the things the feature must leave alone."""
import ctypes

from mofanerf_amd import build, lib, mesh


def L():
    build.build()
    return lib.load()


def test_workspace_sizes_and_refused_sizes():
    ws = L().mofa_raster_workspace_bytes
    assert ws(0, 0, 1, 1) > 0 and ws(100, 200, 48, 64) >= 8 * 48 * 64 + 16 * 100 + 4 * 200
    assert ws(100, 200, 48, 64) % 256 == 0
    assert ws(2 ** 31 - 1, 2 ** 31 - 1, 1, 1) > 16 * (2 ** 31 - 1)
    assert ws(0, 0, 32768, 65535) > 0 and ws(0, 0, 1, 2 ** 31 - 1) > 0                  # H W = 2^31 - 32768 and 2^31 - 1
    for refused in ((0, 0, 0, 8), (0, 0, 8, 0), (0, 0, -1, 8), (0, 0, 32768, 65536), (0, 0, 65536, 65536), (-1, 0, 8, 8), (0, -1, 8, 8),
                    (2 ** 31, 0, 8, 8), (0, 2 ** 31, 8, 8)):
        assert ws(*refused) == 0, refused


def test_bad_arguments_return_einval_with_a_message_and_launch_nothing():
    lb = L()
    buf = ctypes.create_string_buffer(1 << 16)             # host memory stands in: a refused call touches nothing
    p = ctypes.addressof(buf)
    for znear in (0.0, -1.0, float("nan"), float("inf")):
        assert lb.mofa_raster_project(p, 3, 1, 8, 8, 1.0, 1.0, 0.0, 0.0, p, znear, p, None) == -1
        assert b"znear" in lb.mofa_last_error()
    assert lb.mofa_raster_project(p, 3, 1, 0, 8, 1.0, 1.0, 0.0, 0.0, p, 0.1, p, None) == -1 and b"H = 0" in lb.mofa_last_error()
    assert lb.mofa_raster_project(None, 3, 1, 8, 8, 1.0, 1.0, 0.0, 0.0, p, 0.1, p, None) == -1 and b"null" in lb.mofa_last_error()
    assert lb.mofa_raster_faces(p, 1, 3, 8, 8, -1, p, p, None) == -1 and b"wave_min_pixels" in lb.mofa_last_error()
    assert lb.mofa_raster_faces(p, 1, 3, 8, 0, 64, p, p, None) == -1 and b"W = 0" in lb.mofa_last_error()
    assert lb.mofa_raster_faces(p, 1, 3, 8, 8, 64, p, None, None) == -1 and b"null" in lb.mofa_last_error()
    for C in (0, 17, -3):
        assert lb.mofa_raster_resolve(p, 3, p, 1, p, C, 8, 8, 1.0, 1.0, 0.0, 0.0, p, p, p, p, None, p, None, None) == -1
        assert f"C = {C}".encode() in lb.mofa_last_error()
    assert lb.mofa_raster_resolve(p, 3, p, 1, None, 3, 8, 8, 1.0, 1.0, 0.0, 0.0, p, p, p, p, None, p, None, None) == -1
    assert b"attrs" in lb.mofa_last_error()
    assert lb.mofa_raster_resolve(p, 3, p, 1, None, 0, 8, 8, 1.0, 1.0, 0.0, 0.0, p, p, None, p, None, None, None, None) == -1
    assert b"null" in lb.mofa_last_error()


def test_the_feature_leaves_the_abi_version_and_the_profiler_kinds_alone():
    assert L().mofa_abi_version() == 5 == lib.ABI_VERSION and lib.PROF_KINDS == 12
    assert "mofa_raster.hip" in build.SOURCES
    assert {"mofa_raster_workspace_bytes", "mofa_raster_project", "mofa_raster_faces", "mofa_raster_resolve"} <= set(lib.SIGNATURES)
    assert 0 <= mesh.WAVE_MIN_PIXELS <= mesh.INT32_MAX

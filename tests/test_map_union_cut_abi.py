"""cape_map_union_cut and cape_debug_polygon_union_cut: the declarations of the header, the new flag and the bindings against it, and the
argument checks that need no device.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_map_union_abi import _code

NAMES = ("cape_map_union_cut", "cape_debug_polygon_union_cut")


def test_the_entry_points_are_declared_exported_and_typed(hip_library):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code())
    assert "int cape_map_union_cut(cape_handle h, int32_t n_frames, void* stream);" in flat
    assert ("int cape_debug_polygon_union_cut(cape_handle h, const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, "
            "const double* ring_b, int32_t n_b, const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out, "
            "double* vertices_out);") in flat
    assert "#define CAPE_ABI_VERSION 2" in _code()
    lib = cape_amd.load_library()
    assert set(NAMES) <= set(cape_amd.EXPORTED_SYMBOLS)
    for name in NAMES:
        getattr(lib, name)
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.cape_map_union_cut.argtypes == lib.cape_map_union_holes.argtypes == [vp, i32, vp]
    assert lib.cape_debug_polygon_union_cut.argtypes == lib.cape_debug_polygon_union.argtypes == [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp]


def test_the_twins_are_declared_and_exported(host_binaries):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code("cape_host_map.h", os.path.join("rgb-d-slam_amd", "host")))
    assert ("int cape_host_map_union_cut(const cape_host_map* map, const int32_t* match, const cape_plane_fusion* fusion, "
            "const cape_plane_measurement* measurements, const double* world_vertices, int32_t n_cur, cape_plane_union* rows_out, "
            "cape_plane_union_rings* rings_out, double* vertices_out);") in flat
    assert ("int cape_host_polygon_union_cut(const double* rings_a, const int32_t* counts_a, int32_t n_rings_a, const double* ring_b, int32_t n_b, "
            "const double* frames27, cape_plane_union* row_out, cape_plane_union_rings* rings_out, double* vertices_out);") in flat
    L = cape_amd._host_library()
    assert L.cape_host_map_union_cut.argtypes == L.cape_host_map_union_holes.argtypes
    assert L.cape_host_polygon_union_cut.argtypes == L.cape_host_polygon_union.argtypes
    for name in ("host_map_union_cut", "host_polygon_union_cut"):
        assert callable(getattr(cape_amd, name))
    for name in ("map_union_cut", "debug_polygon_union_cut"):
        assert callable(getattr(cape_amd.Extractor, name))


def test_the_flag_mirrors_the_header_and_the_older_ones_stay(hip_library):
    import cape_amd

    code = _code()
    for bit, name in ((0, "SERVED"), (5, "HOST_CAPACITY"), (6, "HOST_AMBIGUOUS"), (7, "HOLES"), (8, "HOST_HOLE_CUT"), (9, "HOLE_PIECES")):
        assert re.search(rf"CAPE_UNION_{name}\s*=\s*1u << {bit}\b", code), name
        assert getattr(cape_amd, f"UNION_{name}") == 1 << bit, name
    assert not cape_amd.UNION_HOST & cape_amd.UNION_HOLE_PIECES  # a flag of a served pair, not a reason to go to the host


def test_the_argument_checks_run_before_the_device_probe(hip_library):
    """No handle can be created here: a NULL handle, a negative frame count, a NULL argument and counts out of range are refused with
    CAPE_ERR_INVALID_ARGUMENT before anything touches a device, and the binding turns that into CapeError."""
    import cape_amd

    lib = cape_amd.load_library()
    sq = np.array([[0, 0], [0, 1], [1, 1], [1, 0.0]])
    counts = np.array([4], np.int32)
    row, rr, ver = np.zeros(1, cape_amd.PLANE_UNION_DTYPE), np.zeros(1, cape_amd.PLANE_UNION_RINGS_DTYPE), np.zeros((2048, 2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.cape_map_union_cut(None, 1, None) == -1
    assert lib.cape_map_union_cut(None, -1, None) == -1
    fake = C.c_void_p(8)  # (never dereferenced: the checks below come first)
    assert lib.cape_map_union_cut(fake, -1, None) == -1
    ok = [fake, p(sq), p(counts), 1, p(sq), 4, None, p(row), p(rr), p(ver)]
    for k in (0, 1, 2, 4, 7, 8, 9):
        assert lib.cape_debug_polygon_union_cut(*(ok[:k] + [None] + ok[k + 1:])) == -1, k
    for n_rings in (0, 10):
        assert lib.cape_debug_polygon_union_cut(*(ok[:3] + [n_rings] + ok[4:])) == -1
    for n_b in (2, 4097):
        assert lib.cape_debug_polygon_union_cut(*(ok[:5] + [n_b] + ok[6:])) == -1
    for bad in (2, 4097):
        assert lib.cape_debug_polygon_union_cut(*(ok[:2] + [p(np.array([bad], np.int32))] + ok[3:])) == -1
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h, ex.max_batch, ex.boundary_capacity = lib, None, 1, 8
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_union_cut failed \(-1\)"):
        ex.map_union_cut(1)
    with pytest.raises(cape_amd.CapeError, match=r"cape_debug_polygon_union_cut failed \(-1\)"):
        ex.debug_polygon_union_cut([sq], sq)

"""cape_map_union, its two companions and cape_debug_ring_union: the declarations of the header, the layout of cape_plane_union and the
constants of the binding against it, and the argument checks that need no device.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cape_map_union", "cape_copy_map_union", "cape_device_map_union", "cape_debug_ring_union")
FLAGS = ("SERVED", "UNCHANGED", "DISJOINT", "HOST_MAP_HOLES", "HOST_NEW_HOLE", "HOST_CAPACITY", "HOST_AMBIGUOUS")


class _PlaneUnion(C.Structure):
    _fields_ = [("x_axis", C.c_double * 3), ("y_axis", C.c_double * 3), ("center", C.c_double * 3), ("area", C.c_double),
                ("vertex_offset", C.c_uint32), ("vertex_count", C.c_uint32), ("map_plane", C.c_int32), ("flags", C.c_uint32),
                ("n_nodes", C.c_uint32), ("pad", C.c_uint32)]


def _code(name="cape_hip.h", where="include"):
    hdr = open(os.path.join(ROOT, where, name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_the_entry_points_are_declared_exported_and_typed(hip_library):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code())
    assert "int cape_map_union(cape_handle h, int32_t n_frames, void* stream);" in flat
    assert "int cape_copy_map_union(cape_handle h, int32_t n_frames, cape_plane_union* rows , double* vertices);" in flat
    assert "int cape_device_map_union(cape_handle h, cape_plane_union** rows, double** vertices);" in flat
    assert ("int cape_debug_ring_union(cape_handle h, const double* ring_a, int32_t n_a, const double* ring_b, int32_t n_b, "
            "const double* frames27, cape_plane_union* row_out, double* vertices_out);") in flat
    assert "#define CAPE_ABI_VERSION 2" in _code()
    lib = cape_amd.load_library()
    assert set(NAMES) <= set(cape_amd.EXPORTED_SYMBOLS)
    for name in NAMES:
        getattr(lib, name)
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.cape_map_union.argtypes == [vp, i32, vp]
    assert lib.cape_copy_map_union.argtypes == [vp, i32, vp, vp]
    assert lib.cape_device_map_union.argtypes == [vp, C.POINTER(vp), C.POINTER(vp)]
    assert lib.cape_debug_ring_union.argtypes == [vp, vp, i32, vp, i32, vp, vp, vp]


def test_the_twins_are_declared_and_exported(host_binaries):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code("cape_host_map.h", os.path.join("rgb-d-slam_amd", "host")))
    assert ("int cape_host_map_union(const cape_host_map* map, const int32_t* match, const cape_plane_fusion* fusion, "
            "const cape_plane_measurement* measurements, const double* world_vertices, int32_t n_cur, cape_plane_union* rows_out, "
            "double* vertices_out);") in flat
    assert ("int cape_host_ring_union(const double* ring_a, int32_t n_a, const double* ring_b, int32_t n_b, const double* frames27, "
            "cape_plane_union* row_out, double* vertices_out);") in flat
    L = cape_amd._host_library()
    assert L.cape_host_map_union and L.cape_host_ring_union
    for name in ("host_map_union", "host_ring_union"):
        assert callable(getattr(cape_amd, name))
    for name in ("map_union", "map_unions", "map_union_rows", "debug_ring_union"):
        assert callable(getattr(cape_amd.Extractor, name))


def test_the_union_row_mirrors_the_header(hip_library):
    import cape_amd

    code = _code()
    body = re.search(r"typedef struct cape_plane_union\s*\{(.*?)\}\s*cape_plane_union;", code, re.S).group(1)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == [
        "double x_axis[3], y_axis[3], center[3]", "double area", "uint32_t vertex_offset, vertex_count", "int32_t map_plane",
        "uint32_t flags", "uint32_t n_nodes, pad"]
    dt = cape_amd.PLANE_UNION_DTYPE
    assert dt.itemsize == C.sizeof(_PlaneUnion) == 104
    assert dt.names == tuple(name for name, _ in _PlaneUnion._fields_)
    for name, _ in _PlaneUnion._fields_:
        assert dt.fields[name][1] == getattr(_PlaneUnion, name).offset, name


def test_the_constants_mirror_the_header(hip_library):
    import cape_amd

    code = _code()
    for bit, name in enumerate(FLAGS):
        assert re.search(rf"CAPE_UNION_{name}\s*=\s*1u << {bit}\b", code), name
        assert getattr(cape_amd, f"UNION_{name}") == 1 << bit, name
    for name, value in (("MAX_RING", 128), ("MAX_NODES", 512), ("FRAME_VERTICES", 2048)):
        assert re.search(rf"#define CAPE_MAP_UNION_{name} {value}\b", code), name
        assert getattr(cape_amd, f"MAP_UNION_{name}") == value


def test_the_argument_checks_run_before_the_device_probe(hip_library):
    """No handle can be created here: a NULL handle and a negative frame count are refused with CAPE_ERR_INVALID_ARGUMENT before
    anything touches a device, and the binding turns that into CapeError."""
    import cape_amd

    lib = cape_amd.load_library()
    sq = np.array([[0, 0], [0, 1], [1, 1], [1, 0.0]])
    row, ver = np.zeros(1, cape_amd.PLANE_UNION_DTYPE), np.zeros((512, 2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.cape_map_union(None, 1, None) == -1
    assert lib.cape_map_union(None, -1, None) == -1
    assert lib.cape_copy_map_union(None, 1, None, None) == -1
    assert lib.cape_device_map_union(None, None, None) == -1
    assert lib.cape_debug_ring_union(None, p(sq), 4, p(sq), 4, None, p(row), p(ver)) == -1
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h, ex.max_batch, ex.boundary_capacity = lib, None, 1, 8
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_union failed \(-1\)"):
        ex.map_union(1)
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_map_union failed \(-1\)"):
        ex.map_unions(1)
    with pytest.raises(cape_amd.CapeError, match=r"cape_debug_ring_union failed \(-1\)"):
        ex.debug_ring_union(sq, sq)

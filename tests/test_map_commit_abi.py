"""cape_map_commit, cape_map_info and cape_map_download: the declarations of the header, the layout of cape_map_commit_result and the
constants of the binding against it, the twin's declaration, and the argument checks that need no device.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cape_map_commit", "cape_map_info", "cape_map_download")
FLAGS = ("DONE", "FRAME_OVERFLOW", "BAD_POSE_COV", "HOST_PAIR", "FAIL_POLYGON", "CAPACITY")


class _CommitResult(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("frame", C.c_int32), ("n_planes", C.c_int32), ("n_rings", C.c_int32), ("n_vertices", C.c_int64),
                ("n_updated", C.c_int32), ("n_appended", C.c_int32), ("n_host_pairs", C.c_int32), ("n_fail_polygon", C.c_int32),
                ("next_id", C.c_uint64)]


def _code(name="cape_hip.h", where="include"):
    hdr = open(os.path.join(ROOT, where, name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_the_entry_points_are_declared_exported_and_typed(hip_library):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code())
    assert ("int cape_map_commit(cape_handle h, int32_t frame, uint32_t flags, uint64_t* next_id, cape_map_commit_result* out, "
            "void* stream);") in flat
    assert "int cape_map_info(cape_handle h, int32_t* n_planes, int32_t* n_rings, int64_t* n_vertices);" in flat
    assert ("int cape_map_download(cape_handle h, cape_map_plane* planes, int32_t planes_capacity, cape_map_ring* rings, "
            "int32_t rings_capacity, double* vertices, int64_t vertices_capacity, cape_map_track* tracks );") in flat
    assert "#define CAPE_ABI_VERSION 2" in _code()
    lib = cape_amd.load_library()
    assert lib.cape_abi_version() == 2
    assert set(NAMES) <= set(cape_amd.EXPORTED_SYMBOLS)
    for name in NAMES:
        getattr(lib, name)
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.cape_map_commit.argtypes == [vp, i32, C.c_uint32, C.POINTER(C.c_uint64), vp, vp]
    assert lib.cape_map_info.argtypes == [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_int64)]
    assert lib.cape_map_download.argtypes == [vp, vp, i32, vp, i32, vp, C.c_int64, vp]


def test_the_twin_is_declared_and_exported(host_binaries):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code("cape_host_map.h", os.path.join("rgb-d-slam_amd", "host")))
    assert ("int cape_host_map_commit(const cape_host_map* map, int32_t frame, const cape_frame_map_kalman* frame_header, "
            "const cape_map_track_result* track_results, const cape_plane_fusion* fusion, const cape_plane_measurement* measurements, "
            "const double* world_vertices, const cape_plane_union* union_rows, const cape_plane_union_rings* rings, const double* slab, "
            "uint32_t flags, uint64_t* next_id, cape_host_map* map_out, cape_map_commit_result* result_out);") in flat
    assert cape_amd._host_library().cape_host_map_commit
    assert callable(cape_amd.host_map_commit)
    for name in ("map_commit", "map_info", "download_map"):
        assert callable(getattr(cape_amd.Extractor, name))


def test_the_result_mirrors_the_header(hip_library):
    import cape_amd

    body = re.search(r"typedef struct cape_map_commit_result\s*\{(.*?)\}\s*cape_map_commit_result;", _code(), re.S).group(1)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == [
        "uint32_t flags", "int32_t frame", "int32_t n_planes, n_rings", "int64_t n_vertices",
        "int32_t n_updated, n_appended, n_host_pairs, n_fail_polygon", "uint64_t next_id"]
    dt = cape_amd.MAP_COMMIT_RESULT_DTYPE
    assert dt.itemsize == C.sizeof(_CommitResult) == 48
    assert dt.names == tuple(name for name, _ in _CommitResult._fields_)
    for name, _ in _CommitResult._fields_:
        assert dt.fields[name][1] == getattr(_CommitResult, name).offset, name


def test_the_constants_mirror_the_header(hip_library):
    import cape_amd

    code = _code()
    for bit, name in enumerate(FLAGS):
        assert re.search(rf"CAPE_COMMIT_{name}\s*=\s*1u << {bit}\b", code), name
        assert getattr(cape_amd, f"COMMIT_{name}") == 1 << bit, name
    assert re.search(r"CAPE_COMMIT_ADD_STAGED\s*=\s*1u << 0\b", code) and cape_amd.COMMIT_ADD_STAGED == 1


def test_the_argument_checks_run_before_the_device_probe(hip_library):
    """No handle can be created here: a NULL handle, result or next_id, an unknown flag and a negative frame are refused with
    CAPE_ERR_INVALID_ARGUMENT before anything touches a device, and the binding turns that into CapeError."""
    import cape_amd

    lib = cape_amd.load_library()
    nid, result = C.c_uint64(3), np.zeros(1, cape_amd.MAP_COMMIT_RESULT_DTYPE)
    out = result.ctypes.data_as(C.c_void_p)
    assert lib.cape_map_commit(None, 0, 0, C.byref(nid), out, None) == -1
    assert lib.cape_map_commit(None, -1, 0, C.byref(nid), out, None) == -1
    assert lib.cape_map_commit(None, 0, 2, C.byref(nid), out, None) == -1
    assert lib.cape_map_commit(None, 0, 0, None, out, None) == -1
    assert lib.cape_map_commit(None, 0, 0, C.byref(nid), None, None) == -1
    assert nid.value == 3 and not result.view(np.uint8).any()
    assert lib.cape_map_info(None, None, None, None) == -1
    assert lib.cape_map_download(None, None, 0, None, 0, None, 0, None) == -1
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h, ex.max_batch, ex.boundary_capacity = lib, None, 1, 8
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_commit failed \(-1\)"):
        ex.map_commit(0)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_info failed \(-1\)"):
        ex.map_info()
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_info failed \(-1\)"):
        ex.download_map()

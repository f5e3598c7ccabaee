"""cape_map_maintain and the retired log's three calls: the declarations of the header, the layout of cape_map_maintain_result and the
constants of the binding against it, the twin's declaration, and the argument checks that need no device.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cape_map_maintain", "cape_map_retired_info", "cape_map_retired_download", "cape_map_retired_clear")
FLAGS = ("DONE", "NOTHING", "CAPACITY", "LOG_FULL")


class _MaintainResult(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("n_planes", C.c_int32), ("n_rings", C.c_int32), ("n_local", C.c_int32), ("n_vertices", C.c_int64),
                ("n_staged", C.c_int32), ("n_promoted", C.c_int32), ("n_promote_refused", C.c_int32), ("n_dropped", C.c_int32),
                ("n_lost", C.c_int32), ("n_retired", C.c_int32), ("n_retired_rings", C.c_int32), ("pad", C.c_uint32),
                ("n_retired_vertices", C.c_int64)]


def _code(name="cape_hip.h", where="include"):
    hdr = open(os.path.join(ROOT, where, name)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_the_entry_points_are_declared_exported_and_typed(hip_library):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code())
    assert "int cape_map_maintain(cape_handle h, uint32_t flags , cape_map_maintain_result* out, void* stream);" in flat
    assert "int cape_map_retired_info(cape_handle h, int32_t* n_planes, int32_t* n_rings, int64_t* n_vertices);" in flat
    assert ("int cape_map_retired_download(cape_handle h, cape_map_plane* planes, int32_t planes_capacity, cape_map_ring* rings, "
            "int32_t rings_capacity, double* vertices, int64_t vertices_capacity, cape_map_track* tracks );") in flat
    assert "int cape_map_retired_clear(cape_handle h);" in flat
    lib = cape_amd.load_library()
    assert set(NAMES) <= set(cape_amd.EXPORTED_SYMBOLS)
    for name in NAMES:
        getattr(lib, name)
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.cape_map_maintain.argtypes == [vp, C.c_uint32, vp, vp]
    assert lib.cape_map_retired_info.argtypes == [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_int64)]
    assert lib.cape_map_retired_download.argtypes == [vp, vp, i32, vp, i32, vp, C.c_int64, vp]
    assert lib.cape_map_retired_clear.argtypes == [vp]


def test_the_twin_is_declared_and_exported(host_binaries):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code("cape_host_map.h", os.path.join("rgb-d-slam_amd", "host")))
    assert ("int cape_host_map_maintain(const cape_host_map* map, cape_host_map* map_out, cape_host_map* retired_out, "
            "cape_map_maintain_result* result_out);") in flat
    assert cape_amd._host_library().cape_host_map_maintain
    assert callable(cape_amd.host_map_maintain)
    for name in ("map_maintain", "retired_info", "download_retired", "clear_retired"):
        assert callable(getattr(cape_amd.Extractor, name))


def test_the_result_mirrors_the_header(hip_library):
    import cape_amd

    body = re.search(r"typedef struct cape_map_maintain_result\s*\{(.*?)\}\s*cape_map_maintain_result;", _code(), re.S).group(1)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == [
        "uint32_t flags", "int32_t n_planes, n_rings", "int32_t n_local", "int64_t n_vertices", "int32_t n_staged",
        "int32_t n_promoted, n_promote_refused, n_dropped, n_lost", "int32_t n_retired, n_retired_rings", "uint32_t pad",
        "int64_t n_retired_vertices"]
    dt = cape_amd.MAP_MAINTAIN_RESULT_DTYPE
    assert dt.itemsize == C.sizeof(_MaintainResult) == 64
    assert dt.names == tuple(name for name, _ in _MaintainResult._fields_)
    for name, _ in _MaintainResult._fields_:
        assert dt.fields[name][1] == getattr(_MaintainResult, name).offset, name


def test_the_constants_mirror_the_header(hip_library):
    import cape_amd

    code = _code()
    for bit, name in enumerate(FLAGS):
        assert re.search(rf"CAPE_MAINTAIN_{name}\s*=\s*1u << {bit}\b", code), name
        assert getattr(cape_amd, f"MAINTAIN_{name}") == 1 << bit, name
    assert re.search(r"#define CAPE_MAP_RETIRED_MAX_PLANES 4096\b", code) and cape_amd.MAP_RETIRED_MAX_PLANES == 4096
    # the thresholds of the rules header are those the update's result bits are documented with
    rules = open(os.path.join(ROOT, "rgb-d-slam_amd", "csrc", "cape_map_maintain.h")).read()
    for name, value in (("kMaintainPromoteMatches", 4), ("kMaintainDropMisses", 2), ("kMaintainLostMisses", 10)):
        assert re.search(rf"{name} = {value};", rules), name


def test_the_argument_checks_run_before_the_device_probe(hip_library):
    """No handle can be created here: a NULL handle or result and a non-zero flag are refused with CAPE_ERR_INVALID_ARGUMENT before
    anything touches a device, and the binding turns that into CapeError."""
    import cape_amd

    lib = cape_amd.load_library()
    result = np.zeros(1, cape_amd.MAP_MAINTAIN_RESULT_DTYPE)
    out = result.ctypes.data_as(C.c_void_p)
    assert lib.cape_map_maintain(None, 0, out, None) == -1
    assert lib.cape_map_maintain(None, 1, out, None) == -1
    assert lib.cape_map_maintain(None, 0, None, None) == -1
    assert not result.view(np.uint8).any()
    assert lib.cape_map_retired_info(None, None, None, None) == -1
    assert lib.cape_map_retired_download(None, None, 0, None, 0, None, 0, None) == -1
    assert lib.cape_map_retired_clear(None) == -1
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h, ex.max_batch, ex.boundary_capacity = lib, None, 1, 8
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_maintain failed \(-1\)"):
        ex.map_maintain()
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_retired_info failed \(-1\)"):
        ex.retired_info()
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_retired_info failed \(-1\)"):
        ex.download_retired()
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_retired_clear failed \(-1\)"):
        ex.clear_retired()

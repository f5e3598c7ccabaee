"""cape_map_measure and its three companions: the declarations of the header, the layout of cape_plane_measurement and the flag
values of the binding against it, and the argument checks that need no device.  CPU only."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cape_map_measure", "cape_device_map_measurements", "cape_copy_map_measurements", "cape_copy_spill_measurements")
FLAGS = ("KEPT", "STAGEABLE", "FAIL_PLANE_COV", "FAIL_WORLD_COV", "FAIL_POLYGON", "RING_TOO_LONG", "BAD_POSE_COV")


class _PlaneMeasurement(C.Structure):
    _fields_ = [("normal", C.c_double * 3), ("d", C.c_double), ("staged_normal", C.c_double * 3), ("covariance", C.c_double * 16),
                ("x_axis", C.c_double * 3), ("y_axis", C.c_double * 3), ("center", C.c_double * 3), ("vertex_offset", C.c_uint32),
                ("vertex_count", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32)]


def _code():
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_the_four_entry_points_are_declared_exported_and_typed(hip_library):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code())
    assert ("int cape_map_measure(cape_handle h, int32_t n_frames, const double* camera_to_world, const double* pose_covariance, "
            "void* stream);") in flat
    assert "int cape_device_map_measurements(cape_handle h, cape_plane_measurement** rows, double** world_vertices);" in flat
    assert "int cape_copy_map_measurements(cape_handle h, int32_t n_frames, cape_plane_measurement* rows, double* world_vertices);" in flat
    assert ("int cape_copy_spill_measurements(cape_handle h, int32_t first, int32_t count, cape_plane_measurement* rows, "
            "double* world_vertices);") in flat
    lib = cape_amd.load_library()
    assert set(NAMES) <= set(cape_amd.EXPORTED_SYMBOLS)
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.cape_map_measure.argtypes == [vp, i32, vp, vp, vp]
    assert lib.cape_device_map_measurements.argtypes == [vp, C.POINTER(vp), C.POINTER(vp)]
    assert lib.cape_copy_map_measurements.argtypes == [vp, i32, vp, vp]
    assert lib.cape_copy_spill_measurements.argtypes == [vp, i32, i32, vp, vp]


def test_the_measurement_row_mirrors_the_header(hip_library):
    import cape_amd

    code = _code()
    body = re.search(r"typedef struct cape_plane_measurement\s*\{(.*?)\}\s*cape_plane_measurement;", code, re.S).group(1)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == [
        "double normal[3], d", "double staged_normal[3]", "double covariance[16]", "double x_axis[3], y_axis[3], center[3]",
        "uint32_t vertex_offset, vertex_count", "uint32_t flags, pad"]
    dt = cape_amd.PLANE_MEASUREMENT_DTYPE
    assert dt.itemsize == C.sizeof(_PlaneMeasurement) == 272
    assert dt.names == tuple(name for name, _ in _PlaneMeasurement._fields_)
    for name, _ in _PlaneMeasurement._fields_:
        assert dt.fields[name][1] == getattr(_PlaneMeasurement, name).offset, name
    assert dt["covariance"].shape == (4, 4) and dt["normal"].shape == (3,)


def test_the_flag_values_mirror_the_header(hip_library):
    import cape_amd

    code = _code()
    for bit, name in enumerate(FLAGS):
        assert re.search(rf"CAPE_MEASURE_{name}\s*=\s*1u << {bit}\b", code), name
        assert getattr(cape_amd, f"MEASURE_{name}") == 1 << bit, name
    for value, name in ((8, "COV_VALID"), (9, "PLANE_COV"), (10, "WORLD_PLANE_COV")):
        assert re.search(rf"CAPE_DEBUG_{name} = {value}\b", code), name
        assert cape_amd.DEBUG_OPS[name.lower()] == value


def test_the_argument_checks_run_before_the_device_probe(hip_library):
    """No handle can be created here: a NULL handle, a negative frame count and a missing pose covariance are refused with
    CAPE_ERR_INVALID_ARGUMENT before anything touches a device, and the binding turns that into CapeError."""
    import numpy as np

    import cape_amd

    lib = cape_amd.load_library()
    S = np.eye(3).reshape(1, 9).copy()
    assert lib.cape_map_measure(None, 1, None, S.ctypes.data_as(C.c_void_p), None) == -1
    assert lib.cape_map_measure(None, -1, None, S.ctypes.data_as(C.c_void_p), None) == -1
    assert lib.cape_map_measure(None, 1, None, None, None) == -1
    assert lib.cape_device_map_measurements(None, None, None) == -1
    assert lib.cape_copy_map_measurements(None, 1, None, None) == -1
    assert lib.cape_copy_spill_measurements(None, 0, 0, None, None) == -1
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h, ex.max_batch, ex.boundary_capacity = lib, None, 1, 8
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_measure failed \(-1\)"):
        ex.map_measure(1, None, np.eye(3)[None])
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_measure failed \(-1\)"):
        ex.map_measure(1, None, None)
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_map_measurements failed \(-1\)"):
        ex.measurement_rows(1)
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_spill_measurements failed \(-1\)"):
        ex.spill_measurement_rows(0, 1)

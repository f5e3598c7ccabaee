"""cape_map_step: the declaration of the header, the layout of cape_map_step_result (the commit's header, then the maintenance's) and
the binding's dtype against it, and the argument checks that need no device.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _CommitResult(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("frame", C.c_int32), ("n_planes", C.c_int32), ("n_rings", C.c_int32), ("n_vertices", C.c_int64),
                ("n_updated", C.c_int32), ("n_appended", C.c_int32), ("n_host_pairs", C.c_int32), ("n_fail_polygon", C.c_int32),
                ("next_id", C.c_uint64)]


class _MaintainResult(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("n_planes", C.c_int32), ("n_rings", C.c_int32), ("n_local", C.c_int32), ("n_vertices", C.c_int64),
                ("n_staged", C.c_int32), ("n_promoted", C.c_int32), ("n_promote_refused", C.c_int32), ("n_dropped", C.c_int32),
                ("n_lost", C.c_int32), ("n_retired", C.c_int32), ("n_retired_rings", C.c_int32), ("pad", C.c_uint32),
                ("n_retired_vertices", C.c_int64)]


class _StepResult(C.Structure):
    _fields_ = [("commit", _CommitResult), ("maintain", _MaintainResult)]


def _code():
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_the_entry_point_is_declared_exported_and_typed(hip_library):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code())
    assert ("int cape_map_step(cape_handle h, int32_t frame, const double* world_to_camera , const uint32_t* skip , uint32_t match_flags, "
            "uint32_t commit_flags, uint64_t* next_id, cape_map_step_result* out, void* stream);") in flat
    lib = cape_amd.load_library()
    assert lib.cape_abi_version() == cape_amd.CAPE_ABI_VERSION == 2  # additions only
    assert "cape_map_step" in cape_amd.EXPORTED_SYMBOLS
    vp = C.c_void_p
    assert lib.cape_map_step.argtypes == [vp, C.c_int32, vp, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), vp, vp]
    assert callable(cape_amd.Extractor.map_step)


def test_the_result_is_the_two_headers_side_by_side(hip_library):
    import cape_amd

    body = re.search(r"typedef struct cape_map_step_result\s*\{(.*?)\}\s*cape_map_step_result;", _code(), re.S).group(1)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == ["cape_map_commit_result commit",
                                                                                      "cape_map_maintain_result maintain"]
    assert C.sizeof(_CommitResult) == 48 and C.sizeof(_MaintainResult) == 64
    assert C.sizeof(_StepResult) == C.sizeof(_CommitResult) + C.sizeof(_MaintainResult) == 112
    assert (_StepResult.commit.offset, _StepResult.maintain.offset) == (0, 48)
    dt = cape_amd.MAP_STEP_RESULT_DTYPE
    assert dt.itemsize == 112 and dt.names == ("commit", "maintain")
    assert (dt.fields["commit"][1], dt.fields["maintain"][1]) == (0, 48)
    assert dt.fields["commit"][0] == cape_amd.MAP_COMMIT_RESULT_DTYPE and dt.fields["maintain"][0] == cape_amd.MAP_MAINTAIN_RESULT_DTYPE


def test_the_hand_off_rule_has_one_definition(hip_library):
    """the kernels' source and the host's bookkeeping compile step_map_after: the name is defined once, in cape_map_step.h, and used by
    the kernels' file and by the API's"""
    csrc = os.path.join(ROOT, "rgb-d-slam_amd", "csrc")
    rule = open(os.path.join(csrc, "cape_map_step.h")).read()
    assert len(re.findall(r"StepMapState step_map_after\(", rule)) == 1
    for name in ("cape_map_maintain.hip", "cape_api_map_update.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert "step_map_after(" in text and "StepMapState step_map_after(" not in text, name


def test_the_argument_checks_run_before_the_device_probe(hip_library):
    """No handle can be created here: a NULL handle, result, next_id or pose, a negative frame and the flags the call refuses come
    back as CAPE_ERR_INVALID_ARGUMENT before anything touches a device, and the binding turns that into CapeError."""
    import cape_amd

    lib = cape_amd.load_library()
    result = np.zeros(1, cape_amd.MAP_STEP_RESULT_DTYPE)
    out = result.ctypes.data_as(C.c_void_p)
    pose = np.eye(4).ravel()
    T = pose.ctypes.data_as(C.c_void_p)
    nid = C.c_uint64(7)
    fake = C.c_void_p(1)  # (never dereferenced: the checks below come first)
    assert lib.cape_map_step(None, 0, T, None, 0, 0, C.byref(nid), out, None) == -1
    assert lib.cape_map_step(fake, 0, T, None, 0, 0, C.byref(nid), None, None) == -1
    assert lib.cape_map_step(fake, 0, T, None, 0, 0, None, out, None) == -1
    assert lib.cape_map_step(fake, 0, None, None, 0, 0, C.byref(nid), out, None) == -1
    assert lib.cape_map_step(fake, -1, T, None, 0, 0, C.byref(nid), out, None) == -1
    for match_flags in (cape_amd.MATCH_MAP_AREAS, cape_amd.MATCH_MAP_DEVICE_SKIP, 1 << 30):
        assert lib.cape_map_step(fake, 0, T, None, match_flags, 0, C.byref(nid), out, None) == -1, match_flags
    assert lib.cape_map_step(fake, 0, T, None, 0, 2, C.byref(nid), out, None) == -1
    assert nid.value == 7 and not result.view(np.uint8).any()
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h, ex.max_batch, ex.boundary_capacity = lib, None, 1, 8
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_step failed \(-1\)"):
        ex.map_step(0, np.eye(4))

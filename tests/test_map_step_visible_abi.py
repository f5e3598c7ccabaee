"""cape_map_step_visible and cape_map_step_skip_words: the declarations of the header, the layout of cape_map_step_visible_result (the
step's result, then what the visibility counted) and the binding's dtype against it, and the argument checks that need no device.
cape_map_step itself still refuses CAPE_MATCH_MAP_DEVICE_SKIP.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_map_step_abi import _StepResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _StepVisibleResult(C.Structure):
    _fields_ = [("step", _StepResult), ("n_map", C.c_int32), ("n_moving", C.c_int32), ("n_listed", C.c_int32), ("pad", C.c_int32),
                ("n_undecided", C.c_int64)]


def _code():
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_the_entry_points_are_declared_exported_and_typed(hip_library):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code())
    assert ("int cape_map_step_visible(cape_handle h, int32_t frame, const double* world_to_camera , uint32_t match_flags, "
            "uint32_t commit_flags, uint64_t* next_id, cape_map_step_visible_result* out, void* stream);") in flat
    assert "int cape_map_step_skip_words(cape_handle h, uint32_t* words, int32_t words_capacity, int32_t* n_map);" in flat
    lib = cape_amd.load_library()
    assert lib.cape_abi_version() == cape_amd.CAPE_ABI_VERSION == 2  # additions only
    assert "cape_map_step_visible" in cape_amd.EXPORTED_SYMBOLS and "cape_map_step_skip_words" in cape_amd.EXPORTED_SYMBOLS
    vp = C.c_void_p
    assert lib.cape_map_step_visible.argtypes == [vp, C.c_int32, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), vp, vp]
    assert lib.cape_map_step_skip_words.argtypes == [vp, vp, C.c_int32, C.POINTER(C.c_int32)]
    assert callable(cape_amd.Extractor.map_step_visible) and callable(cape_amd.Extractor.map_step_skip_words)


def test_the_result_is_the_steps_result_and_the_counters(hip_library):
    import cape_amd

    body = re.search(r"typedef struct cape_map_step_visible_result\s*\{(.*?)\}\s*cape_map_step_visible_result;", _code(), re.S).group(1)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == [
        "cape_map_step_result step", "int32_t n_map", "int32_t n_moving", "int32_t n_listed", "int32_t pad", "int64_t n_undecided"]
    assert C.sizeof(_StepResult) == 112 and C.sizeof(_StepVisibleResult) == 112 + 24 == 136
    S = _StepVisibleResult
    assert (S.step.offset, S.n_map.offset, S.n_moving.offset, S.n_listed.offset, S.pad.offset, S.n_undecided.offset) == (0, 112, 116, 120, 124, 128)
    dt = cape_amd.MAP_STEP_VISIBLE_RESULT_DTYPE
    assert dt.itemsize == 136 and dt.names == ("step", "n_map", "n_moving", "n_listed", "pad", "n_undecided")
    assert [dt.fields[n][1] for n in dt.names] == [0, 112, 116, 120, 124, 128]
    assert dt.fields["step"][0] == cape_amd.MAP_STEP_RESULT_DTYPE
    assert [dt.fields[n][0] for n in dt.names[1:]] == [np.dtype("<i4")] * 4 + [np.dtype("<i8")]


def test_the_moving_bit_is_no_longer_informational():
    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    line = next(ln for ln in hdr.splitlines() if "CAPE_MAP_TRACK_MOVING = " in ln)
    assert "informational" not in line and "cape_map_step_visible" in line


def test_the_argument_checks_run_before_the_device_probe(hip_library):
    """No handle can be created here: a NULL handle, result, next_id or pose, a negative frame and the flags the call refuses come back
    as CAPE_ERR_INVALID_ARGUMENT before anything touches a device; so do the reader's NULL handle and negative capacity."""
    import cape_amd

    lib = cape_amd.load_library()
    result = np.zeros(1, cape_amd.MAP_STEP_VISIBLE_RESULT_DTYPE)
    out = result.ctypes.data_as(C.c_void_p)
    pose = np.eye(4).ravel()
    T = pose.ctypes.data_as(C.c_void_p)
    nid = C.c_uint64(7)
    fake = C.c_void_p(1)  # (never dereferenced: the checks below come first)
    step = lib.cape_map_step_visible
    assert step(None, 0, T, 0, 0, C.byref(nid), out, None) == -1
    assert step(fake, 0, T, 0, 0, C.byref(nid), None, None) == -1
    assert step(fake, 0, T, 0, 0, None, out, None) == -1
    assert step(fake, 0, None, 0, 0, C.byref(nid), out, None) == -1
    assert step(fake, -1, T, 0, 0, C.byref(nid), out, None) == -1
    for match_flags in (cape_amd.MATCH_MAP_AREAS, cape_amd.MATCH_MAP_DEVICE_SKIP, 1 << 30):
        assert step(fake, 0, T, match_flags, 0, C.byref(nid), out, None) == -1, match_flags
    assert step(fake, 0, T, 0, 2, C.byref(nid), out, None) == -1
    assert nid.value == 7 and not result.view(np.uint8).any()
    # the reader
    words = np.full(4, 0xFFFFFFFF, np.uint32)
    n_map = C.c_int32(-5)
    assert lib.cape_map_step_skip_words(None, words.ctypes.data_as(C.c_void_p), 4, C.byref(n_map)) == -1
    assert lib.cape_map_step_skip_words(fake, words.ctypes.data_as(C.c_void_p), -1, C.byref(n_map)) == -1
    assert n_map.value == -5 and np.all(words == 0xFFFFFFFF)
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h, ex.max_batch, ex.boundary_capacity = lib, None, 1, 8
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_step_visible failed \(-1\)"):
        ex.map_step_visible(0, np.eye(4))
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_step_skip_words failed \(-1\)"):
        ex.map_step_skip_words()


def test_cape_map_step_still_refuses_the_device_skip_flag(hip_library):
    import cape_amd

    lib = cape_amd.load_library()
    result = np.zeros(1, cape_amd.MAP_STEP_RESULT_DTYPE)
    pose = np.eye(4).ravel()
    nid = C.c_uint64(7)
    rc = lib.cape_map_step(C.c_void_p(1), 0, pose.ctypes.data_as(C.c_void_p), None, cape_amd.MATCH_MAP_DEVICE_SKIP, 0, C.byref(nid),
                           result.ctypes.data_as(C.c_void_p), None)
    assert rc == -1 and nid.value == 7 and not result.view(np.uint8).any()

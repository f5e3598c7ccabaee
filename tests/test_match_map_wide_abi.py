"""cape_match_map_wide / cape_copy_map_matches_wide: the declarations of the header, the layout of cape_frame_map_match_wide and the
constants of the binding against it, and the argument checks that need no device.  CPU only."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FrameMapMatchWide(C.Structure):
    _fields_ = [("n_map", C.c_int32), ("n_cur", C.c_int32), ("flags", C.c_uint32), ("n_matched", C.c_int32)]


def _header():
    return open(os.path.join(ROOT, "include", "cape_hip.h")).read()


def test_the_header_declares_both_functions_and_the_struct(hip_library):
    import cape_amd

    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert ("int cape_match_map_wide(cape_handle h, int32_t n_frames, const double* world_to_camera, const uint32_t* skip, "
            "uint32_t flags, void* stream);") in flat
    assert ("int cape_copy_map_matches_wide(cape_handle h, int32_t n_frames, cape_frame_map_match_wide* frames, int32_t* match, "
            "int32_t* seg_cur, int32_t* map_of, double* inter_area);") in flat
    body = re.search(r"typedef struct cape_frame_map_match_wide\s*\{(.*?)\}\s*cape_frame_map_match_wide;", code, re.S).group(1)
    assert re.findall(r"(u?int32_t)\s+([a-z_, ]+);", body) == [("int32_t", "n_map, n_cur"), ("uint32_t", "flags"), ("int32_t", "n_matched")]
    assert "#define CAPE_MATCH_MAP_WIDE_MAX_PLANES CAPE_MATCH_WIDE_MAX_PLANES\n" in hdr and "#define CAPE_MATCH_WIDE_MAX_PLANES 128\n" in hdr
    assert "#define CAPE_ABI_VERSION 2\n" in hdr
    lib = cape_amd.load_library()
    assert hasattr(lib, "cape_match_map_wide") and hasattr(lib, "cape_copy_map_matches_wide")
    assert {"cape_match_map_wide", "cape_copy_map_matches_wide"} <= set(cape_amd.EXPORTED_SYMBOLS)


def test_constants_and_struct_mirror_the_header(hip_library):
    import cape_amd

    assert cape_amd.MATCH_MAP_WIDE_MAX_PLANES == 128
    dt = cape_amd.FRAME_MAP_MATCH_WIDE_DTYPE
    assert dt.itemsize == C.sizeof(_FrameMapMatchWide) == 16
    for name, *_ in _FrameMapMatchWide._fields_:
        assert dt.fields[name][1] == getattr(_FrameMapMatchWide, name).offset, name


def test_without_a_device_the_calls_fail_with_the_shims_error(hip_library):
    """No handle can be created here: the entry points refuse a NULL one, and the methods of the binding turn that into CapeError
    (an AttributeError would mean the binding does not know them)."""
    import cape_amd

    lib = cape_amd.load_library()
    assert lib.cape_match_map_wide(None, 1, None, None, 0, None) == -1
    assert lib.cape_copy_map_matches_wide(None, 1, None, None, None, None, None) == -1
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h, ex.map_size = lib, None, 0
    with pytest.raises(cape_amd.CapeError, match=r"cape_match_map_wide failed \(-1\)"):
        ex.match_map_wide(1)
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_map_matches_wide failed \(-1\)"):
        ex.map_matches_wide(1, areas=True)

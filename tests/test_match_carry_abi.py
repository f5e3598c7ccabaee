"""cape_match_carry_save / _clear / _info and CAPE_MATCH_CARRY: the exports, the constant and the info struct of the binding against
the header, and the argument checks that need no device.  CPU only."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cape_match_carry_save", "cape_match_carry_clear", "cape_match_carry_info")


def test_the_three_symbols_are_exported(hip_library):
    import cape_amd

    lib = cape_amd.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert set(NAMES) <= set(cape_amd.EXPORTED_SYMBOLS)


def test_the_flag_and_the_info_struct_mirror_the_header(hip_library):
    import cape_amd

    hdr = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"CAPE_MATCH_CARRY\s*=\s*1u\s*<<\s*5\b", code)
    assert cape_amd.MATCH_CARRY == 1 << 5
    assert cape_amd.MATCH_CARRY not in (cape_amd.MATCH_ADVANCED, cape_amd.MATCH_ALLOW_INDEX0, cape_amd.MATCH_MAP_AREAS, cape_amd.MATCH_MAP_DEVICE_SKIP)
    body = re.search(r"typedef struct cape_match_carry_info_t\s*\{(.*?)\}\s*cape_match_carry_info_t;", code, re.S).group(1)
    assert re.findall(r"(u?int32_t)\s+([a-z_]+);", body) == [("int32_t", "valid"), ("int32_t", "n_kept"), ("uint32_t", "flags"), ("int32_t", "n_vertices")]
    assert [f[0] for f in cape_amd.cape_match_carry_info_t._fields_] == ["valid", "n_kept", "flags", "n_vertices"]
    assert C.sizeof(cape_amd.cape_match_carry_info_t) == 16
    assert "#define CAPE_ABI_VERSION 2\n" in hdr  # additive: no struct changed


def test_a_null_handle_is_refused_by_each_call(hip_library):
    """No handle can be created here: the entry points refuse a NULL one, and the methods of the binding turn that into CapeError."""
    import cape_amd

    lib = cape_amd.load_library()
    info = cape_amd.cape_match_carry_info_t()
    assert lib.cape_match_carry_save(None, 0, None) == -1
    assert lib.cape_match_carry_clear(None) == -1
    assert lib.cape_match_carry_info(None, C.byref(info)) == -1
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h = lib, None
    for call, name in ((lambda: ex.match_carry_save(0), NAMES[0]), (ex.match_carry_clear, NAMES[1]), (ex.match_carry_info, NAMES[2])):
        with pytest.raises(cape_amd.CapeError, match=name + r" failed \(-1\)"):
            call()

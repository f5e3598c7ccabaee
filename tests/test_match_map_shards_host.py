"""The host side of cape_match_map_shards that needs no GPU: the slot arithmetic of cape_amd.dist, the typed ctypes signatures of the
two entry points and the output flag CAPE_MATCH_EXACT_BAD_SHARD (tests/test_abi.py ties the header's declarations to EXPORTED_SYMBOLS)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_of_round_trips():
    from cape_amd.dist import packed_layout, shard_of, slot_of

    for frames_capacity in (1, 3, 8, 4096):
        layout = packed_layout(frames_capacity, 768, polygons=True)
        seen = []
        for shard in (0, 1, 5):
            for k in sorted({0, frames_capacity // 2, frames_capacity - 1}):
                s = slot_of(shard, k, layout)
                assert s == shard * frames_capacity + k and shard_of(s, layout) == (shard, k)
                seen.append(s)
        assert len(set(seen)) == len(seen)
        # the slots of consecutive shards are contiguous: n_shards x frames_capacity in all
        assert slot_of(1, 0, layout) == slot_of(0, frames_capacity - 1, layout) + 1
        for shard, k in ((0, frames_capacity), (0, -1), (-1, 0)):
            with pytest.raises(ValueError):
                slot_of(shard, k, layout)
    with pytest.raises(ValueError):
        shard_of(-1, layout)


def test_the_two_calls_are_typed(hip_library):
    import cape_amd

    L = cape_amd.load_library()
    vp = C.c_void_p
    assert L.cape_match_map_shards.argtypes == [vp, vp, C.c_int32, C.POINTER(cape_amd.cape_gather_layout),
                                                C.POINTER(cape_amd.cape_gather_polygon_layout), vp, vp, C.c_uint32, vp]
    assert L.cape_copy_shard_map_matches.argtypes == [vp, C.c_int32, vp, vp, vp]
    assert {"cape_match_map_shards", "cape_copy_shard_map_matches"} <= set(cape_amd.EXPORTED_SYMBOLS)
    # argument checks that come before any device work: no GPU needed
    lay, pl = cape_amd.cape_gather_layout(), cape_amd.cape_gather_polygon_layout()
    assert L.cape_match_map_shards(None, None, 1, C.byref(lay), C.byref(pl), None, None, 0, None) == -1
    assert L.cape_copy_shard_map_matches(None, 1, None, None, None) == -1


def test_bad_shard_flag_does_not_collide(hip_library):
    import cape_amd

    src = open(os.path.join(ROOT, "include", "cape_hip.h")).read()
    value = {name: 1 << int(shift) for name, shift in re.findall(r"\b(CAPE_MATCH_[A-Z0-9_]+) = 1u << (\d+)", src)}
    assert value["CAPE_MATCH_EXACT_BAD_SHARD"] == cape_amd.MATCH_EXACT_BAD_SHARD == 8
    assert value["CAPE_MATCH_EXACT_OVERFLOW"] == cape_amd.MATCH_EXACT_OVERFLOW and value["CAPE_MATCH_EXACT_HOST"] == cape_amd.MATCH_EXACT_HOST
    outputs = [value[k] for k in ("CAPE_MATCH_EXACT_OVERFLOW", "CAPE_MATCH_EXACT_HOST", "CAPE_MATCH_EXACT_BAD_SHARD")]
    assert len(set(outputs)) == 3 and all(v & (v - 1) == 0 for v in outputs)
    # ... nor with the input flags a caller might OR into the same word
    inputs = [value[k] for k in ("CAPE_MATCH_ADVANCED", "CAPE_MATCH_ALLOW_INDEX0", "CAPE_MATCH_MAP_AREAS")]
    assert cape_amd.MATCH_EXACT_BAD_SHARD not in inputs and cape_amd.MATCH_MAP_AREAS == value["CAPE_MATCH_MAP_AREAS"]

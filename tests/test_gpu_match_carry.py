"""The carried frame (cape_match_carry_save + CAPE_MATCH_CARRY): a stream cut into batches, or served one frame per call, gets from
cape_match_polygons_wide what the unsplit batch gets -- frame structs, matches, segment lists and every entry of the area table bit
for bit -- and what the host twin cape_host_match_planes computes from the kept planes of the two frames; a flagged carry flags the
frame behind it; the carry outlives every other call on the handle until the next save or a clear."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 128  # cape_amd.MATCH_WIDE_MAX_PLANES


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _handle(width, height, intr, max_batch):
    import torch
    from cape_amd import Extractor

    return Extractor(width, height, cylinders=False, max_batch=max_batch, **intr), torch.cuda.current_stream().cuda_stream


def _batch(ex, st, dev, first, n):
    """frames [first, first + n) of the device tensor `dev` become the handle's batch, polygons built"""
    ex.extract_device(dev[first:first + n].data_ptr(), n, st)
    ex.build_polygons(n, st)


def _matched(ex, st, n, T, flags):
    import cape_amd

    ex.match_polygons_wide(n, T, flags | cape_amd.MATCH_MAP_AREAS, st)
    return ex.polygon_matches_wide(n, areas=True)


def _assert_row(got, g, ref, r, what):
    """row g of one copied result equals row r of another: the frame struct, match, seg_prev, seg_cur, the area table bit for bit"""
    for name in ("n_prev", "n_cur", "flags", "n_matched"):
        assert got[0][g][name] == ref[0][r][name], f"{what}: {name} {got[0][g][name]} != {ref[0][r][name]}"
    for k, name in ((1, "match"), (2, "seg_prev"), (3, "seg_cur")):
        assert np.array_equal(got[k][g], ref[k][r]), f"{what}: {name}"
    bad = np.argwhere(_bits(got[4][g]) != _bits(ref[4][r]))
    assert len(bad) == 0, f"{what}: areas differ at {bad[:4].tolist()}"


def _assert_twin(got, g, prev_kept, cur_kept, T0, flags, what):
    """row g against cape_host_match_planes on the kept planes of the two frames: independent of the device's unsplit run"""
    import cape_amd

    (prev, prev_segs), (cur, cur_segs) = prev_kept, cur_kept
    fr, match, seg_prev, seg_cur, inter = got
    assert (fr[g]["n_prev"], fr[g]["n_cur"], fr[g]["flags"]) == (len(prev), len(cur), 0), what
    assert list(seg_prev[g, : len(prev)]) == prev_segs and list(seg_cur[g, : len(cur)]) == cur_segs, what
    m, ia = cape_amd.host_match_planes(prev, cur, T0, flags, areas=True)
    assert list(match[g, : len(prev)]) == list(m) and np.all(match[g, len(prev):] == -1), what
    bad = np.argwhere(_bits(inter[g, : len(prev), : len(cur)]) != _bits(ia))
    assert len(bad) == 0, f"{what}: areas differ from the host class at {bad[:4].tolist()}"


@functools.lru_cache(maxsize=None)
def _room():
    """four 640 x 480 room frames on the device and the relative poses of their trajectory"""
    from test_gpu_match_pose import _strided

    dev, T = _strided("room", 31, 40, 9, 4)
    return dev, np.ascontiguousarray(T, np.float64).reshape(4, 4, 4)


@functools.lru_cache(maxsize=None)
def _room_reference(flags):
    """the unsplit batch: one 4-frame call"""
    from cape_amd import synth

    dev, T = _room()
    ex, st = _handle(640, 480, synth.DEFAULT_INTRINSICS, 4)
    _batch(ex, st, dev, 0, 4)
    ref = _matched(ex, st, 4, T, flags)
    ex.close()
    assert np.all(ref[0]["flags"] == 0)
    # an empty comparison proves nothing
    assert int((ref[1][2] >= 0).sum()) >= 1 and np.count_nonzero(ref[4][2] > 0) >= 1, "row 2 of the reference holds no match / no area"
    return ref


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_a_split_batch_equals_the_whole_batch(flags):
    """2 + 2 frames on a max_batch = 2 handle, frame 1 carried over the cut: rows 0..1 of either call are rows 0..1 / 2..3 of the 4-frame
    call, and the row behind the cut is the host twin's."""
    import cape_amd
    from cape_amd import synth

    assert W == cape_amd.MATCH_WIDE_MAX_PLANES and (cape_amd.MATCH_ADVANCED, cape_amd.MATCH_ALLOW_INDEX0) == (1, 2)
    dev, T = _room()
    ref = _room_reference(flags)
    ex, st = _handle(640, 480, synth.DEFAULT_INTRINSICS, 2)
    _batch(ex, st, dev, 0, 2)
    first = _matched(ex, st, 2, T[:2], flags)
    for f in (0, 1):
        _assert_row(first, f, ref, f, f"first batch, frame {f}")
    prev_kept = ex.kept_planes(2)[1]  # (taken before the next extract)
    ex.match_carry_save(1, st)
    _batch(ex, st, dev, 2, 2)
    second = _matched(ex, st, 2, T[2:], flags | cape_amd.MATCH_CARRY)
    for f in (0, 1):
        _assert_row(second, f, ref, 2 + f, f"second batch, frame {f}")
    assert second[0][0]["n_prev"] == len(prev_kept[0]) > 0
    _assert_twin(second, 0, prev_kept, ex.kept_planes(2)[0], T[2], flags, "the row behind the cut")
    info = ex.match_carry_info()
    assert (info["valid"], info["n_kept"], info["flags"]) == (1, len(prev_kept[0]), 0)
    assert info["n_vertices"] == sum(len(p[5]) for p in prev_kept[0])
    ex.close()


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_one_frame_per_call(flags):
    """The reference's call pattern on a one-frame handle (records and polygons in pinned host memory, the carry in device memory): call
    f's single row is row f of the 4-frame call."""
    import cape_amd
    from cape_amd import synth

    dev, T = _room()
    ref = _room_reference(flags)
    ex, st = _handle(640, 480, synth.DEFAULT_INTRINSICS, 1)
    for f in range(4):
        _batch(ex, st, dev, f, 1)
        got = _matched(ex, st, 1, T[f:f + 1], flags | (cape_amd.MATCH_CARRY if f else 0))
        _assert_row(got, 0, ref, f, f"call {f}")
        ex.match_carry_save(0, st)
    ex.close()


def test_a_chained_predecessor():
    """[room, big | big, room] at 1280 x 960, `big` the checkerboard of 116 segments in two records: the carried frame holds planes of
    its spill record, and the row behind the cut is the unsplit batch's and the host twin's."""
    import torch
    import cape_amd
    from cape_amd import synth
    from test_gpu_map_match import _checker_frames
    from test_gpu_match_wide import _small_pose

    Wd, Ht = 1280, 960
    big, intr = _checker_frames(Wd, Ht, 100)
    room = synth.room(seed=1, frame=0, width=Wd, height=Ht, intr=intr)
    dev = torch.from_numpy(np.ascontiguousarray(np.stack([room, big, big, room]))).cuda()
    cases = [(None, 0), (None, cape_amd.MATCH_ALLOW_INDEX0), (_small_pose(4), cape_amd.MATCH_ADVANCED)]
    ex, st = _handle(Wd, Ht, intr, 4)
    _batch(ex, st, dev, 0, 4)
    assert len(ex.results(4).chain(1)) == 2
    refs = [_matched(ex, st, 4, T, flags) for T, flags in cases]
    ex.close()
    ex, st = _handle(Wd, Ht, intr, 2)
    for (T, flags), ref in zip(cases, refs):
        assert ref[0][2]["flags"] == 0 and ref[0][2]["n_prev"] > 64
        _batch(ex, st, dev, 0, 2)
        prev_kept = ex.kept_planes(2)[1]
        assert len(prev_kept[0]) > 64 and prev_kept[1][-1] >= 64, "the chain keeps planes of its second record"
        ex.match_carry_save(1, st)
        _batch(ex, st, dev, 2, 2)
        got = _matched(ex, st, 2, None if T is None else T[2:], flags | cape_amd.MATCH_CARRY)
        _assert_row(got, 0, ref, 2, f"flags {flags}: the row behind the cut")
        _assert_row(got, 1, ref, 3, f"flags {flags}: the row after it")
        assert got[0][0]["n_prev"] > 64 and int(got[2][0].max()) >= 64 and int(got[1][0].max()) >= 64
        _assert_twin(got, 0, prev_kept, ex.kept_planes(2)[0], None if T is None else T[2], flags, f"flags {flags}: the row behind the cut")
    ex.close()


def _flagged_carry(width, height, intr, flagged_frame, rooms):
    """[served, flagged | served, served] on a max_batch = 2 handle: the carry's description, then the two rows behind it"""
    import torch
    import cape_amd

    dev = torch.from_numpy(np.ascontiguousarray(np.stack([rooms[0], flagged_frame, rooms[1], rooms[2]]))).cuda()
    ex, st = _handle(width, height, intr, 2)
    _batch(ex, st, dev, 0, 2)
    kept = ex.kept_planes(2)[1]
    pol, _ = ex.polygons(2)
    ex.match_carry_save(1, st)
    info = ex.match_carry_info()
    _batch(ex, st, dev, 2, 2)
    got = _matched(ex, st, 2, None, cape_amd.MATCH_CARRY)
    ex.close()
    n_true = len(kept[0])
    assert info["valid"] == 1 and info["flags"] == cape_amd.MATCH_EXACT_OVERFLOW and info["n_kept"] == n_true
    fr, match, seg_prev, _, inter = got
    assert fr[0]["flags"] == cape_amd.MATCH_EXACT_OVERFLOW and fr[0]["n_prev"] == n_true
    assert np.all(match[0] == -1) and fr[0]["n_matched"] == 0 and np.all(inter[0] == -1.0)
    assert list(seg_prev[0, : min(n_true, W)]) == kept[1][:W] and np.all(seg_prev[0, n_true:] == -1)  # the first 128 positions
    assert fr[1]["flags"] == 0 and fr[1]["n_prev"] == fr[0]["n_cur"] > 0, "the frame after it is served"
    assert fr[1]["n_matched"] >= 1 and np.count_nonzero(inter[1] > 0) >= 1
    return n_true, pol


def test_a_carry_with_a_plane_left_to_the_host_class_flags_the_next_frame():
    import cape_amd
    from cape_amd import synth
    from test_gpu_match_wide import _perforated_wall

    Wd, Ht = 1280, 960
    intr = {k: v * 2.0 for k, v in synth.DEFAULT_INTRINSICS.items()}
    rooms = [synth.room(seed=1, frame=f, width=Wd, height=Ht, intr=intr) for f in (0, 3, 6)]
    _, pol = _flagged_carry(Wd, Ht, intr, _perforated_wall(Wd, Ht, intr), rooms)
    assert (pol[1]["flags"] & cape_amd.POLY_OVERFLOW).any()


def test_a_carry_of_more_than_128_kept_planes_flags_the_next_frame():
    from test_gpu_map_match import _checker_frames

    Wd, Ht = 1920, 1080
    big, intr = _checker_frames(Wd, Ht, 120)
    # the frames around it: the checkerboard of 60 facets (a room frame of this size holds a wall of more than 1 024 boundary points
    # and is flagged on its own account)
    small, _ = _checker_frames(Wd, Ht, 200)
    n_true, _ = _flagged_carry(Wd, Ht, intr, big, [small] * 3)
    assert n_true > W


def test_lifetime_and_arguments():
    import cape_amd
    from cape_amd import synth

    dev, T = _room()
    carry = cape_amd.MATCH_CARRY
    ex, st = _handle(640, 480, synth.DEFAULT_INTRINSICS, 2)
    assert ex.match_carry_info() == dict(valid=0, n_kept=0, flags=0, n_vertices=0)
    ex.extract_device(dev.data_ptr(), 2, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # no polygons of this batch yet
        ex.match_carry_save(0, st)
    ex.build_polygons(1, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # beyond the last build_polygons
        ex.match_carry_save(1, st)
    ex.build_polygons(2, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):
        ex.match_carry_save(2, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.match_carry_save(-1, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # nothing saved
        ex.match_polygons_wide(2, T[:2], carry, st)
    # the other matchers do not know the bit
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\): unknown match flag"):
        ex.match_polygons(2, carry, st)
    kept0, prev_kept = ex.kept_planes(2)
    ex.upload_map([(nn, d, x, y, c, ring, []) for nn, d, x, y, c, ring, _ in kept0[0][:2]])
    ex.match_map(2, None, None, 0, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\): unknown match flag"):
        ex.match_map(2, None, None, carry, st)
    ex.match_carry_save(1, st)
    _batch(ex, st, dev, 2, 2)
    row = _matched(ex, st, 2, T[2:], carry)
    assert int((row[1][0] >= 0).sum()) >= 1
    again = _matched(ex, st, 2, T[2:], carry)  # read, not consumed
    _assert_row(again, 0, row, 0, "two carried calls in a row")
    # another batch goes through the handle, flagless: the carry is still frame 1 of the first batch
    _batch(ex, st, dev, 0, 2)
    other = _matched(ex, st, 2, T[:2], 0)
    assert other[0][0]["n_prev"] == 0
    _batch(ex, st, dev, 2, 2)
    later = _matched(ex, st, 2, T[2:], carry)
    _assert_row(later, 0, row, 0, "after another batch")
    _assert_row(later, 1, row, 1, "after another batch, frame 1")
    # no poses: every entry, entry 0 included, is the identity -- the host twin without a pose bit for bit, and the decisions of
    # identity matrices (whose arithmetic re-normalises the normals: areas equal only to rounding, as for cape_match_polygons_pose)
    null = _matched(ex, st, 2, None, carry)
    eye = _matched(ex, st, 2, np.stack([np.eye(4)] * 2), carry)
    assert int((null[1][0] >= 0).sum()) >= 1
    _assert_twin(null, 0, prev_kept, ex.kept_planes(2)[0], None, 0, "NULL poses, the carried row")
    assert np.array_equal(null[1], eye[1]) and np.array_equal(null[2], eye[2]), "NULL poses against identity matrices"
    ex.match_carry_clear()
    assert ex.match_carry_info()["valid"] == 0
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):
        ex.match_polygons_wide(2, T[2:], carry, st)
    ex.match_polygons_wide(2, T[2:], 0, st)  # the flagless call is what it was
    assert ex.polygon_matches_wide(2)[0][0]["n_prev"] == 0
    ex.close()

"""The device's plane-count capacities, each visited at its last slot and one past it.

    16 kept planes    cape_match_polygons, cape_match_polygons_pose                           test_the_16_plane_matchers
    32 segments       the everyday grow kernels (kFastPlanes; segment 33 hands the frame on)  test_extraction_around_32_segments
    64 segments       a record (CAPE_MAX_PLANES; segment 65 opens a spill record)             test_extraction_around_64_segments,
                                                                                              test_polygons_across_the_chain
    64 kept planes    cape_match_map (first record), cape_match_map_shards, the second half   test_match_map_at_64, test_match_map_shards_at_64,
                      of the wide kernels' lanes ("a lane holds kept planes k and k + 64")    test_wide_matcher_around_64, test_lattice_*
    128 segments      two full records                                                        test_extraction_around_128_segments
    128 kept planes   cape_match_polygons_wide, cape_match_map_wide, the carried frame,       test_wide_matcher_around_128, test_carry_*,
                      the rows of cape_map_measure / cape_map_kalman                          test_match_map_wide_at_128, test_map_update_*

The frames come from tests/capacity_cases.py, whose counts tests/test_capacity_cases.py pins on the CPU: every facet / pane that
survives is a plane segment, an output plane and a kept plane.  Every comparison is with the oracle, the host twins or the host
polygon class at tolerance 0; the one exception is the BOUND of tests/test_gpu_map_measure.py for the covariances that pass through
pow, reused unchanged."""
import numpy as np
import pytest

import capacity_cases as K
from test_gpu_polygon import host_poly  # noqa: F401  (the fixture: the host polygon class through cape_host_polygon)

pytestmark = pytest.mark.gpu

W = 128  # cape_amd.MATCH_WIDE_MAX_PLANES
SMALL, MID, BIG = (640, 480, 80), (1280, 960, 100), (1920, 1080, 120)
LATTICE = (1280, 960, 4, 5)


@pytest.fixture(autouse=True)
def _host_twins(host_binaries):
    """the host twins (libcape_primitives.so) are built before cape_amd.host_* load them"""


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _checkers(counts, grid):
    """(frames stacked, intr) of the checkerboards with these plane counts"""
    made = [K.checker_with(c, *grid) for c in counts]
    return np.stack([m[0] for m in made]), made[0][1]


def _shared(prev, cur):
    """From the oracle's label grids of two frames of one generator (the same facets or panes, fewer or more of them zeroed): the
    0-based positions, in the current frame's segment list, of the segments the previous frame has too.  Under the identity -- or a
    pose that moves an outline by a few millimetres -- exactly these are matched: each by its own predecessor, the only candidate it
    overlaps; but position 0 unless MATCH_ALLOW_INDEX0 is set (the reference's `selectedIndex <= 0`)."""
    a, b = prev.plane_labels, cur.plane_labels
    return sorted(set((b[(a > 0) & (b > 0)] - 1).tolist()))


def _expected_matches(prev, cur, flags):
    import cape_amd

    shared = _shared(prev, cur)
    return len(shared) - (1 if 0 in shared and not flags & cape_amd.MATCH_ALLOW_INDEX0 else 0)


def _room(grid):
    from cape_amd import synth

    return synth.room(seed=1, frame=0, width=grid[0], height=grid[1], intr=K._intr(grid[0]))


def _kept_counts(kept):
    return [len(det) for det, _ in kept]


# ---- a. extraction and record chains ----------------------------------------------------------------------------------------------

def _extraction(oracle_mod, grid, counts, cyl, records, room=True):
    """The checkerboards with `counts` plane segments (and a room frame behind them) in one batch, twice on one handle: every
    observable of compare_frame equals the oracle's, and the records say what the counts demand -- `records[k]` records in frame k's
    chain, the last of which ends the chain, no capacity flag, as many spill records handed out as the chains need and as many
    frames through the general instance as have more than 64 segments."""
    from cape_amd import CAPE_MAX_PLANES, FRAME_PLANE_OVERFLOW, Extractor
    from test_gpu_parity import compare_frame

    Wd, Ht = grid[:2]
    frames, intr = _checkers(counts, grid)
    want = [K.checker_oracle(c, *grid, cyl) for c in counts]
    if room:
        frames = np.concatenate([frames, _room(grid)[None]])
        want.append(oracle_mod.Oracle(Wd, Ht, cylinders=cyl, **intr).run(frames[-1]))
    n = len(frames)
    ex = Extractor(Wd, Ht, cylinders=cyl, max_batch=n, **intr)
    lines = []
    ex.set_log_callback(lambda level, msg, frame: lines.append((level, msg, frame)))
    spilled = sum(r - 1 for r in records)
    for rep in range(2):
        assert ex.extract_host(frames) == n
        res = ex.results(n)
        hdr = res.records["header"]
        used, pool, general = ex.spill_info()
        assert (used, general) == (spilled, sum(1 for r in records if r > 1)) and pool >= spilled, (used, pool, general)
        for f, (count, recs) in enumerate(zip(counts, records)):
            assert int(hdr["n_plane_segments"][f]) == count
            assert len(res.segments(f)) == count and int(res.plane_labels[f].max()) == count
            chain = res.chain(f)
            assert len(chain) == recs, f"{count} segments: {len(chain)} records"
            for k, (rec, _) in enumerate(chain):
                h = rec["header"]
                assert not int(h["status"]) & FRAME_PLANE_OVERFLOW, f"{count} segments, record {k}: capacity flag"
                assert int(h["segment_base"]) == k * CAPE_MAX_PLANES
                # a chain ends AT a full record: no empty record behind 64 or 128 segments
                assert int(h["n_plane_segments"]) == count - k * CAPE_MAX_PLANES >= 1
                assert (int(h["next_record"]) >= n) == (k + 1 < recs), f"{count} segments, record {k}: next_record {int(h['next_record'])}"
        for f in range(n):
            assert not int(hdr["status"][f]) & FRAME_PLANE_OVERFLOW
            compare_frame(want[f], ex, res, f, check_cells=False)
    assert not [ln for ln in lines if "per-frame capacity exceeded" in ln[1]]
    ex.close()


@pytest.mark.parametrize("cyl", [False, True])
def test_extraction_around_32_segments(oracle_mod, cyl):
    """31 / 32 / 33 plane segments at 640 x 480: the everyday grow kernels hold 32 (kFastPlanes) and hand a frame to the 64-segment
    instance when segment 33 arrives (`nSeg >= MAXP` in front of the store, cape_grow.hip).  One record each, nothing spilled."""
    _extraction(oracle_mod, SMALL, [31, 32, 33], cyl, [1, 1, 1])


@pytest.mark.parametrize("cyl", [False, True])
def test_extraction_around_64_segments(oracle_mod, cyl):
    """63 / 64 / 65 plane segments at 1280 x 960.  The 64-segment instance hands a frame to the general instance when segment 65
    arrives, and the general instance takes ceil(segments / 64) records (recNeeded, cape_grow_general.hip): exactly 64 segments stay
    in the frame's own record with next_record = -1 -- the chain ends at a full record, there is no empty record behind it -- and 65
    put a single segment into a spill record."""
    _extraction(oracle_mod, MID, [63, 64, 65], cyl, [1, 1, 2])


@pytest.mark.parametrize("cyl", [False, True])
def test_extraction_around_128_segments(oracle_mod, cyl):
    """127 / 128 / 129 plane segments at 1920 x 1080: two records for 127 and for exactly 128 (the second one full, next_record = -1),
    three for 129, whose last record holds one segment.  Five spill records of the pool's eight."""
    _extraction(oracle_mod, BIG, [127, 128, 129], cyl, [2, 2, 3], room=False)


@pytest.mark.parametrize("count,records", [(64, 1), (65, 2)], ids=["64", "65"])
def test_one_frame_handle_at_64_segments(count, records):
    """On a max_batch = 1 handle the general instance is launched lazily, by the first reader that settles the results: results()
    here.  64 segments never arm it; 65 do, and come back whole."""
    from cape_amd import Extractor
    from test_gpu_parity import compare_frame

    depth, intr, want = K.checker_with(count, *MID)
    ex = Extractor(MID[0], MID[1], cylinders=False, max_batch=1, **intr)
    for rep in range(2):
        assert ex.extract_host(depth) == 1
        res = ex.results(1)
        assert len(res.chain(0)) == records and not int(res.records["header"]["status"][0]) & 1
        assert (int(res.records["header"]["next_record"][0]) >= 1) == (records > 1)
        assert ex.spill_info()[::2] == (records - 1, records - 1)
        compare_frame(want, ex, res, 0, check_cells=False)
    ex.close()


# ---- b. polygons across the chain ---------------------------------------------------------------------------------------------------

def _center(s):
    return np.asarray(s["normal"], np.float64) * (-np.float64(s["d"]))


@pytest.mark.parametrize("count,grid,records", [(65, MID, 2), (129, BIG, 3)], ids=["65", "129"])
def test_polygons_across_the_chain(host_poly, count, grid, records):  # noqa: F811
    """Every output plane of the 65- and of the 129-plane frame, the single plane of the last record included: the polygon
    cape_build_polygons made equals the host class on the same boundary candidates bit for bit.  The rows and vertex slabs of the
    spill records come through spill_polygons, record by record along next_record."""
    from cape_amd import POLY_VALID
    from test_gpu_match_wide import _extract
    from test_gpu_polygon import _same

    depth, intr, _ = K.checker_with(count, *grid)
    ex, st = _extract(np.stack([depth]), grid[0], grid[1], intr)
    res = ex.results(1)
    pol, ver = ex.polygons(1)
    used = ex.spill_info()[0]
    assert used == records - 1
    spol, sver = ex.spill_polygons(0, used)
    chain = res.chain(0)
    assert len(chain) == records
    per_record, rec_index = [], 0
    for part, (rec, slab) in enumerate(chain):
        k = rec_index - ex.max_batch
        prow, vslab = (pol[0], ver[0]) if part == 0 else (spol[k], sver[k])
        n_seg = min(64, int(rec["header"]["n_plane_segments"]))
        compared = 0
        for i in range(n_seg):
            s, p = rec["segments"][i], prow[i]
            assert s["is_output"], "every facet is an output plane"
            pts = slab[int(s["boundary_offset"]): int(s["boundary_offset"]) + int(s["boundary_count"])]
            o, c = int(p["vertex_offset"]), int(p["vertex_count"])
            _same(p, vslab[o:o + c], host_poly(pts, s["normal"], _center(s)), f"record {part} segment {i} ({len(pts)} points)")
            assert p["flags"] & POLY_VALID and c >= 3 and np.array_equal(_bits(p["center"]), _bits(_center(s)))
            compared += 1
        assert not prow[n_seg:]["flags"].any() and not prow[n_seg:]["vertex_count"].any(), f"record {part}: rows beyond its segments"
        per_record.append(compared)
        rec_index = int(rec["header"]["next_record"])
    assert per_record == [64] * (records - 1) + [1]
    ex.close()


# ---- c. the 16-plane matchers -------------------------------------------------------------------------------------------------------

def test_the_16_plane_matchers():
    """Frames that keep [16, 17, 16, 15, 16] planes.  cape_match_polygons and cape_match_polygons_pose flag exactly the two frames a
    17-plane frame takes part in; the 16-against-15 and the 15-against-16 frame are served and equal cape_host_match_planes in
    matches and in every bit of the area table; the wide call serves all five, equals the twin, and equals the narrow call on the
    frames both serve (as test_gpu_match_wide.test_narrow_frames_equal_the_16_plane_path has it)."""
    import cape_amd
    from test_gpu_match_wide import _compare_with_twin, _extract, _small_pose

    M, OVF = cape_amd.MATCH_MAX_PLANES, cape_amd.MATCH_EXACT_OVERFLOW
    counts = [16, 17, 16, 15, 16]
    frames, intr = _checkers(counts, SMALL)
    want = [K.checker_with(c, *SMALL)[2] for c in counts]
    n = len(counts)
    ex, st = _extract(frames, SMALL[0], SMALL[1], intr)
    kept = ex.kept_planes(n)
    assert M == 16 and _kept_counts(kept) == counts
    T = _small_pose(n)
    for flags in (0, cape_amd.MATCH_ALLOW_INDEX0):
        for pose in (None, T):
            if pose is None:
                ex.match_polygons(n, flags, st)
            else:
                ex.match_polygons_pose(n, pose, flags, st)
            narrow = ex.polygon_matches(n)
            assert [int(v) for v in narrow["flags"]] == [0, OVF, OVF, 0, 0]
            assert list(narrow["n_prev"]) == [0] + counts[:-1] and list(narrow["n_cur"]) == counts
            for f in (1, 2):  # a flagged frame reports nothing
                assert np.all(narrow[f]["match"] == -1) and np.all(narrow[f]["inter_area"] == -1.0)
            assert np.all(narrow[0]["match"] == -1) and np.all(narrow[0]["inter_area"] == -1.0)
            for f in (3, 4):
                (prev, prev_segs), (cur, cur_segs) = kept[f - 1], kept[f]
                g = narrow[f]
                assert list(g["seg_prev"][: len(prev)]) == prev_segs and np.all(g["seg_prev"][len(prev):] == -1)
                assert list(g["seg_cur"][: len(cur)]) == cur_segs and np.all(g["seg_cur"][len(cur):] == -1)
                m, ia = cape_amd.host_match_planes(prev, cur, None if pose is None else pose[f], flags, areas=True)
                assert list(g["match"][: len(prev)]) == list(m) and np.all(g["match"][len(prev):] == -1), f"frame {f}"
                bad = np.argwhere(_bits(g["inter_area"][: len(prev), : len(cur)]) != _bits(ia))
                assert len(bad) == 0, f"frame {f}: areas differ from the host class at {bad[:4].tolist()}"
                assert np.all(g["inter_area"][len(prev):] == -1.0) and np.all(g["inter_area"][:, len(cur):] == -1.0)
                # the 15 facets the two frames share find themselves (but index 0, unless asked for)
                assert sum(1 for v in m if v >= 0) == _expected_matches(want[f - 1], want[f], flags) >= 14, f"frame {f}: {list(m)}"
            assert 15 in _shared(want[3], want[4]) and int(narrow[4]["match"].max()) == 15, "the sixteenth plane of a full table is matched"
            ex.match_polygons_wide(n, pose, flags | cape_amd.MATCH_MAP_AREAS, st)
            fr, match, seg_prev, seg_cur, inter = _compare_with_twin(ex, n, pose, flags, kept)  # (asserts that no frame is flagged)
            for f in (3, 4):
                for name, wide in (("match", match), ("seg_prev", seg_prev), ("seg_cur", seg_cur)):
                    assert np.array_equal(wide[f, :M], narrow[f][name]) and np.all(wide[f, M:] == -1), (f, name)
                assert np.array_equal(_bits(inter[f, :M, :M]), _bits(narrow[f]["inter_area"])), f"frame {f}: the area tables differ"
            assert 16 in _shared(want[0], want[1]) and int(match[1].max()) == 16, "the wide call serves the 17-plane frames"
            assert [int(v) for v in fr["n_matched"][1:]] == [_expected_matches(want[f - 1], want[f], flags) for f in range(1, n)]
    ex.close()


# ---- d. the wide consecutive matcher ------------------------------------------------------------------------------------------------

def test_wide_matcher_around_64():
    """Kept counts [64, 65, 63, 64] at 1280 x 960: the second plane of a lane (kept planes k and k + 64) holds nothing, or exactly one
    plane, on either side of a pair.  Every frame is served; the twin bit for bit, the oracle's decisions."""
    import cape_amd
    from test_gpu_match_wide import _compare_with_twin, _extract, _small_pose

    counts = [64, 65, 63, 64]
    frames, intr = _checkers(counts, MID)
    want = [K.checker_with(c, *MID)[2] for c in counts]
    assert 64 in _shared(want[0], want[1]) and 64 in _shared(want[2], want[1]), "the plane of the spill record is a facet of every frame"
    ex, st = _extract(frames, MID[0], MID[1], intr)
    assert [len(ex.results(4).chain(f)) for f in range(4)] == [1, 2, 1, 1]
    kept = ex.kept_planes(4)
    assert _kept_counts(kept) == counts and kept[1][1][-1] == 64
    T = _small_pose(4)  # (shifted outlines: see test_gpu_map_match._oracle_decisions)
    for flags in (0, cape_amd.MATCH_ALLOW_INDEX0):
        ex.match_polygons_wide(4, T, flags | cape_amd.MATCH_MAP_AREAS, st)
        fr, match, seg_prev, seg_cur, inter = _compare_with_twin(ex, 4, T, flags, kept, oracle=True)
        assert seg_cur[1, 64] == 64 and seg_prev[2, 64] == 64 and int(seg_cur[[0, 2, 3]].max()) == 63
        assert 64 in match[1], "the kept plane of the spill record is matched"
        assert match[2, 64] >= 0, "... and finds its successor in the next frame"
        assert [int(v) for v in fr["n_matched"][1:]] == [_expected_matches(want[f - 1], want[f], flags) for f in (1, 2, 3)]
        assert min(fr["n_matched"][1:]) >= 62
    ex.close()


def _assert_flagged_wide(got, f, n_prev, n_cur, prev_segs, cur_segs):
    """a frame beyond the wide tables: its true counts, its first 128 segment positions, and nothing else"""
    import cape_amd

    fr, match, seg_prev, seg_cur, inter = got
    assert (fr[f]["flags"], fr[f]["n_prev"], fr[f]["n_cur"], fr[f]["n_matched"]) == (cape_amd.MATCH_EXACT_OVERFLOW, n_prev, n_cur, 0)
    assert np.all(match[f] == -1) and np.all(inter[f] == -1.0)
    assert list(seg_prev[f, : min(n_prev, W)]) == prev_segs[:W] and np.all(seg_prev[f, n_prev:] == -1)
    assert list(seg_cur[f, : min(n_cur, W)]) == cur_segs[:W] and np.all(seg_cur[f, n_cur:] == -1)


def test_wide_matcher_around_128():
    """Kept counts [128, 129, 128, 127] at 1920 x 1080: exactly the two frames the 129-plane frame takes part in are flagged, with
    their true counts and first 128 segment positions; the full table (frame 0) and 128 against 127 (frame 3) are served and equal
    the twin bit for bit, previous plane 127 with a decision."""
    import cape_amd
    from test_gpu_match_carry import _assert_twin, _matched
    from test_gpu_match_wide import _extract, _small_pose

    counts = [128, 129, 128, 127]
    frames, intr = _checkers(counts, BIG)
    want = [K.checker_with(c, *BIG)[2] for c in counts]
    assert len(_shared(want[3], want[2])) == 127 and 127 in _shared(want[3], want[2]), "segment 128 of frame 2 is a facet of frame 3"
    ex, st = _extract(frames, BIG[0], BIG[1], intr)
    kept = ex.kept_planes(4)
    assert _kept_counts(kept) == counts and W == cape_amd.MATCH_WIDE_MAX_PLANES
    for T, flags in ((None, 0), (_small_pose(4), cape_amd.MATCH_ALLOW_INDEX0)):
        got = _matched(ex, st, 4, T, flags)
        fr, match, seg_prev, seg_cur, inter = got
        assert [int(v) for v in fr["flags"]] == [0, cape_amd.MATCH_EXACT_OVERFLOW, cape_amd.MATCH_EXACT_OVERFLOW, 0]
        _assert_twin(got, 0, ([], []), kept[0], None if T is None else T[0], flags, "frame 0")
        assert seg_cur[0, 127] == 127 and np.all(match[0] == -1)
        _assert_flagged_wide(got, 1, 128, 129, kept[0][1], kept[1][1])
        _assert_flagged_wide(got, 2, 129, 128, kept[1][1], kept[2][1])
        _assert_twin(got, 3, kept[2], kept[3], None if T is None else T[3], flags, "128 against 127")
        assert np.all(seg_prev[3] == np.arange(W)) and seg_cur[3, 126] == 126 and seg_cur[3, 127] == -1
        assert match[3, 127] >= 0, "previous plane 127 has a decision"
        assert fr[3]["n_matched"] == _expected_matches(want[2], want[3], flags) >= 126 and np.all(inter[3, :, 127] == -1.0)
    ex.close()


@pytest.mark.parametrize("shifted", [False, True])
def test_lattice_fills_the_second_half_of_the_select_kernel(shifted):
    """The wall behind the lattice with 64, 65 and 103 panes: coplanar planes, so EVERY pair passes both gates and a previous plane's
    run of candidates is n_cur long -- 65 and 103, beyond the 64 first candidates of the select kernel's lanes.  Under the identity a
    plane's only overlapping candidate is itself (position j of its run: the second half for j >= 64); under a shift of one pane
    pitch it is its neighbour.  Matches and areas equal the twin bit for bit."""
    import cape_amd
    from test_gpu_match_wide import _compare_with_twin, _extract

    counts = [64, 65, 103]
    made = [K.lattice_with(c, *LATTICE) for c in counts]
    ex, st = _extract(np.stack([m[0] for m in made]), LATTICE[0], LATTICE[1], made[0][1])
    kept = ex.kept_planes(3)
    assert _kept_counts(kept) == counts
    want = [m[2] for m in made]
    assert max(_shared(want[1], want[2])) >= 64, "a pane of frame 1 sits beyond position 63 of frame 2's list"
    T = None
    if shifted:
        T = np.stack([np.eye(4)] * 3)
        T[:, 0, 3] = K.pane_pitch_mm(LATTICE[0], LATTICE[2])
    for flags in (0, cape_amd.MATCH_ALLOW_INDEX0):
        ex.match_polygons_wide(3, T, flags | cape_amd.MATCH_MAP_AREAS, st)
        fr, match, _, _, inter = _compare_with_twin(ex, 3, T, flags, kept)
        for f in (1, 2):
            n_prev, n_cur = counts[f - 1], counts[f]
            assert not (inter[f, :n_prev, :n_cur] == -1.0).any(), f"frame {f}: a pair did not pass the gates"
            assert np.count_nonzero(inter[f, :n_prev, :n_cur] > 0) >= n_prev // 2
        if not shifted:
            # every pane finds itself: the 64 / 65 panes of the previous frame, those beyond position 63 included
            for f in (1, 2):
                assert fr[f]["n_matched"] == _expected_matches(want[f - 1], want[f], flags) >= counts[f - 1] - 1, f"frame {f}"
            assert int(match[2].max()) == max(_shared(want[1], want[2]))
        else:
            assert min(fr[1]["n_matched"], fr[2]["n_matched"]) >= 32, "the shifted panes land on their neighbours"
    ex.close()


# ---- e. the carried frame -----------------------------------------------------------------------------------------------------------

def test_carry_of_128_and_of_129_kept_planes():
    """[127, 128 | 127, 129 | 127, 128] at 1920 x 1080 on a max_batch = 2 handle.  The carried 128-plane frame fills the carry's
    tables (n_kept 128, no flag) and gives the next batch's frame 0 the bits of the in-batch pair and of the twin; the carried
    129-plane frame is kept as flagged, with its true count, and flags the frame behind it."""
    import torch
    import cape_amd
    from test_gpu_match_carry import _assert_row, _assert_twin, _batch, _handle, _matched
    from test_gpu_match_wide import _small_pose

    OVF, CARRY = cape_amd.MATCH_EXACT_OVERFLOW, cape_amd.MATCH_CARRY
    frames, intr = _checkers([127, 128, 127, 129], BIG)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    T, flags = _small_pose(4), cape_amd.MATCH_ALLOW_INDEX0
    ex, st = _handle(BIG[0], BIG[1], intr, 4)
    _batch(ex, st, dev, 0, 4)
    ref = _matched(ex, st, 4, T, flags)
    ex.close()
    assert [int(v) for v in ref[0]["flags"]] == [0, 0, 0, OVF] and (ref[0][2]["n_prev"], ref[0][2]["n_cur"]) == (128, 127)
    assert ref[1][2, 127] >= 0, "the in-batch pair matches previous plane 127"

    ex, st = _handle(BIG[0], BIG[1], intr, 2)
    _batch(ex, st, dev, 0, 2)
    prev_kept = ex.kept_planes(2)[1]
    assert len(prev_kept[0]) == 128
    ex.match_carry_save(1, st)
    info = ex.match_carry_info()
    assert (info["valid"], info["n_kept"], info["flags"]) == (1, 128, 0)
    assert info["n_vertices"] == sum(len(p[5]) for p in prev_kept[0])
    _batch(ex, st, dev, 2, 2)
    got = _matched(ex, st, 2, T[2:], flags | CARRY)
    _assert_row(got, 0, ref, 2, "the row behind the cut")
    _assert_row(got, 1, ref, 3, "the row after it")
    cur_kept = ex.kept_planes(2)
    _assert_twin(got, 0, prev_kept, cur_kept[0], T[2], flags, "the row behind the cut")
    assert got[1][0, 127] >= 0 and got[2][0, 127] == 127
    # the 129-plane frame: carried as flagged
    ex.match_carry_save(1, st)
    info = ex.match_carry_info()
    assert (info["valid"], info["n_kept"], info["flags"]) == (1, 129, OVF)
    _batch(ex, st, dev, 0, 2)
    after = _matched(ex, st, 2, T[:2], flags | CARRY)
    fr, match, seg_prev, seg_cur, inter = after
    assert (fr[0]["flags"], fr[0]["n_prev"], fr[0]["n_cur"], fr[0]["n_matched"]) == (OVF, 129, 127, 0)
    assert np.all(match[0] == -1) and np.all(inter[0] == -1.0)
    assert list(seg_prev[0]) == cur_kept[1][1][:W], "the first 128 positions of the carried frame"
    assert fr[1]["flags"] == 0 and (fr[1]["n_prev"], fr[1]["n_cur"]) == (127, 128), "the frame after it is served"
    ex.close()


# ---- f. the map matchers ------------------------------------------------------------------------------------------------------------

EYE = (np.eye(3), np.zeros(3))


def _own_map(det):
    """kept planes as map planes under the identity, rings shifted (see test_gpu_map_match._oracle_decisions)"""
    from test_gpu_map_match import _lift

    return [_lift(k, *EYE, ring=k[5] + [7.0, 5.0]) for k in det]


def _mid_batch():
    """[64 planes, 65 planes, room] at 1280 x 960, polygons built, and the map of the 65-plane frame's and the room's own planes"""
    from test_gpu_match_wide import _extract

    frames, intr = _checkers([64, 65], MID)
    ex, st = _extract(np.concatenate([frames, _room(MID)[None]]), MID[0], MID[1], intr)
    kept = ex.kept_planes(3)
    assert _kept_counts(kept)[:2] == [64, 65] and 0 < len(kept[2][0]) <= 64
    assert [len(ex.results(3).chain(f)) for f in range(3)] == [1, 2, 1], "the 65-plane frame continues in a spill record"
    planes = _own_map(kept[1][0] + kept[2][0])
    ex.upload_map(planes)
    return ex, st, kept, planes


def test_match_map_at_64():
    """cape_match_map serves the kept planes of a frame's first record: 64 of them fill seg_cur / map_of and the 64 columns of the
    area table; the 65-plane frame is flagged; the room frame behind it is served."""
    import cape_amd
    from test_gpu_map_match import _compare_with_twin

    ex, st, kept, planes = _mid_batch()
    pairs = [[(s, d) for d, s in zip(det, segs)] for det, segs in kept]  # (as test_gpu_map_match._kept lists them)
    T = np.stack([np.eye(4)] * 3)
    for flags in (cape_amd.MATCH_ALLOW_INDEX0, 0):
        ex.match_map(3, T, None, flags | cape_amd.MATCH_MAP_AREAS, st)
        assert _compare_with_twin(ex, 3, pairs, planes, T, None, flags, oracle=True) == 2
        fr, match, inter = ex.map_matches(3, areas=True)
        assert [int(v) for v in fr["flags"]] == [0, cape_amd.MATCH_EXACT_OVERFLOW, 0]
        assert fr[0]["n_cur"] == 64 and fr[0]["seg_cur"][63] == 63 and fr[0]["map_of"][63] >= 0 and 63 in match[0]
        assert fr[0]["n_matched"] == 64 - (0 if flags else 1) and np.count_nonzero(inter[0][:, 63] > 0) >= 1
        assert np.all(match[1] == -1) and np.all(fr[1]["map_of"] == -1) and fr[1]["n_matched"] == 0 and np.all(inter[1] == -1.0)
        assert fr[2]["n_matched"] >= 1
    ex.close()


def test_match_map_shards_at_64():
    """The shard matcher's 64 kept planes per slot, and the packer's capacity (per shard: frames_capacity x planes_per_frame).  The
    64-plane frame alone in a shard of capacity 64 fits exactly -- served, equal to cape_match_map, nothing dropped --; in a shard of
    capacity 63 its last plane is dropped and the slot flagged; in a shard that holds the whole batch the 65-plane frame's slot is
    flagged beside two served ones."""
    import cape_amd
    from test_gpu_match_map_shards import _assert_flagged, _assert_same, _header_view

    ex, st, kept, planes = _mid_batch()
    flags = cape_amd.MATCH_ALLOW_INDEX0
    ex.match_map(3, None, None, flags | cape_amd.MATCH_MAP_AREAS, st)
    want = ex.map_matches(3, areas=True)
    assert [int(v) for v in want[0]["flags"]] == [0, cape_amd.MATCH_EXACT_OVERFLOW, 0] and want[0][0]["n_matched"] == 64

    def shard(n, per_frame, vertices):
        layout = ex.gather_configure(n, planes_per_frame=per_frame, polygons=True, vertices_per_frame=vertices)
        ptr = ex.pack(n, 0, st)
        overflow = int(_header_view(ex.packed_host())["overflow"][0])
        ex.match_map_shards(ptr, 1, layout, None, None, flags | cape_amd.MATCH_MAP_AREAS, st)
        return overflow, ex.shard_map_matches(n, areas=True)

    overflow, got = shard(1, 64, ex.boundary_capacity)
    assert overflow == 0, "64 planes fit a capacity of 64"
    _assert_same(got, want, slice(0, 1))
    assert got[0][0]["flags"] == 0 and got[0][0]["n_cur"] == 64 and got[0][0]["map_of"][63] >= 0
    overflow, got = shard(1, 63, ex.boundary_capacity)
    assert overflow == cape_amd.PACKED_PLANES_DROPPED
    _assert_flagged(got, 0, cape_amd.MATCH_EXACT_OVERFLOW)
    overflow, got = shard(3, 64, 2 * ex.boundary_capacity)  # (a budget the chain cannot exceed: boundary_capacity per record)
    assert overflow == 0, "the batch's planes fit 3 x 64"
    _assert_same(got, want, np.array([0, 2]))
    _assert_flagged(got, 1, cape_amd.MATCH_EXACT_OVERFLOW)
    ex.close()


def test_match_map_wide_at_128():
    """cape_match_map_wide at 1920 x 1080 against the map of the 129-plane frame's own planes: 127 and 128 kept planes are served and
    equal the twin, the kept plane at index 127 matched; 129 are flagged with their true count, beside the same two served frames."""
    import cape_amd
    from test_gpu_match_map_wide import _compare_with_twin
    from test_gpu_match_wide import _extract, _small_pose

    OVF = cape_amd.MATCH_EXACT_OVERFLOW
    frames, intr = _checkers([127, 128, 129], BIG)
    ex, st = _extract(frames, BIG[0], BIG[1], intr)
    kept = ex.kept_planes(3)
    assert _kept_counts(kept) == [127, 128, 129]
    planes = _own_map(kept[2][0])
    assert len(planes) == 129 <= cape_amd.MAP_MAX_PLANES
    ex.upload_map(planes)
    T = _small_pose(3)
    for flags in (cape_amd.MATCH_ALLOW_INDEX0, 0):
        ex.match_map_wide(2, T[:2], None, flags | cape_amd.MATCH_MAP_AREAS, st)
        fr, match, seg_cur, map_of, inter = _compare_with_twin(ex, 2, kept, planes, T, flags)
        assert seg_cur[1, 127] == 127 and map_of[1, 127] >= 0 and 127 in match[1], "the kept plane at index 127 is matched"
        assert seg_cur[0, 126] == 126 and seg_cur[0, 127] == -1 and map_of[0, 126] >= 0
        assert list(fr["n_matched"]) == [127 - (0 if flags else 1), 128 - (0 if flags else 1)]
        assert np.count_nonzero(inter[1][:, 127] > 0) >= 1
        ex.match_map_wide(3, T, None, flags | cape_amd.MATCH_MAP_AREAS, st)
        fr3, match3, seg_cur3, map_of3, inter3 = ex.map_matches_wide(3, areas=True)
        assert [int(v) for v in fr3["flags"]] == [0, 0, OVF] and (fr3[2]["n_cur"], fr3[2]["n_map"], fr3[2]["n_matched"]) == (129, 129, 0)
        assert np.all(match3[2] == -1) and np.all(map_of3[2] == -1) and np.all(inter3[2] == -1.0)
        assert list(seg_cur3[2]) == kept[2][1][:W]  # the first 128 positions
        for a, b in ((fr3, fr), (match3, match), (seg_cur3, seg_cur), (map_of3, map_of)):
            assert np.array_equal(a[:2], b), "the served frames beside the flagged one"
        assert np.array_equal(_bits(inter3[:2]), _bits(inter))
    ex.close()


# ---- g. the map update's 128-row tables -----------------------------------------------------------------------------------------------

def _map_update(frames, grid, intr, source):
    """match_map_wide, map_measure and map_kalman of a batch against the map of frame `source`'s own stageable measurements, each
    compared with its twin through the helpers of its own test file; returns (measurements, fusion rows, results)"""
    import cape_amd
    from test_gpu_map_kalman import _compare_with_twin, _tracks
    from test_gpu_map_match import _w2c
    from test_gpu_map_measure import _compare_frame, _detected, _pose_covariances
    from test_gpu_match_wide import _extract
    from test_map_update_host import _pose

    n = len(frames)
    ex, st = _extract(frames, grid[0], grid[1], intr)
    rng = np.random.default_rng(33)
    T, S = np.stack([_pose(rng)] * n), _pose_covariances(rng, n)  # (one camera pose: every frame sees the source frame's planes)
    W2C = np.stack([_w2c(T[f][:3, :3], T[f][:3, 3]) for f in range(n)])
    ex.map_measure(n, T, S, st)
    meas, det = ex.map_measurements(n), _detected(ex, n)
    stats = dict(rel=0.0, bits=0, n=0)
    compared = [_compare_frame(meas[f], det[f][0], det[f][1], T[f], S[f], stats) for f in range(n)]
    assert compared[source] == len(det[source][0]), "a kept plane of the source frame was not compared"
    print(f"\nmeasurements: largest _rel {stats['rel']:.3g} over {stats['n']} kept planes, {stats['bits']} covariances differ in a bit")
    map_meas = [m for m in meas[source] if m["flags"] & cape_amd.MEASURE_STAGEABLE]
    assert len(map_meas) == len(meas[source])
    arrays, tracks = cape_amd.pack_map([m["plane"] for m in map_meas]), _tracks(map_meas)
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, cape_amd.MATCH_ALLOW_INDEX0, st)
    ex.map_kalman(n, st)
    fr, rows, results, _, meas = _compare_with_twin(ex, n, arrays, tracks)
    ex.close()
    return meas, fr, rows, results


def test_map_update_rows_at_127_and_128():
    """cape_map_measure and cape_map_kalman keep 128 rows per frame: a [127, 128] pair fills them to the last row but one and to the
    last row.  Row 127 is measured (in a spill record: segment 127), matched, fused, and equal to the twins."""
    import cape_amd

    frames, intr = _checkers([127, 128], BIG)
    meas, fr, rows, results = _map_update(frames, BIG, intr, source=1)
    assert [len(m) for m in meas] == [127, 128] and list(fr["n_cur"]) == [127, 128]
    assert meas[1][127]["segment"] == 127 and meas[1][127]["flags"] & cape_amd.MEASURE_STAGEABLE and meas[1][127]["covariance"].any()
    assert meas[1][64]["segment"] == 64 and meas[1][64]["covariance"].any(), "the first plane of the spill record"
    for i in (64, 127):
        assert rows[1, i]["flags"] & cape_amd.FUSION_STATE and rows[1, i]["map_plane"] == i, f"row {i}: {rows[1, i]['flags']}, {rows[1, i]['map_plane']}"
    assert fr[1]["n_updated"] == 128 and fr[0]["n_updated"] == 127
    assert rows[0, 126]["flags"] & cape_amd.FUSION_STATE and not rows[0, 127:].view(np.uint8).any()
    updated = np.flatnonzero(results[1]["result"] & cape_amd.MAP_RESULT_UPDATED)
    assert len(updated) == 128 and sorted(results[1]["kept_plane"][updated]) == list(range(128))


def test_map_update_rows_of_a_65_plane_frame():
    """The same for the frame with ONE plane in its spill record: row 64 -- the record's only segment -- is measured, matched and
    fused; the room frame beside it is untouched by the chain."""
    import cape_amd

    frames, intr = _checkers([65], MID)
    meas, fr, rows, results = _map_update(np.concatenate([frames, _room(MID)[None]]), MID, intr, source=0)
    assert len(meas[0]) == 65 and fr[0]["n_cur"] == 65 and 0 < len(meas[1]) < 64
    assert meas[0][64]["segment"] == 64 and meas[0][64]["flags"] & cape_amd.MEASURE_STAGEABLE and meas[0][64]["covariance"].any()
    assert rows[0, 64]["flags"] & cape_amd.FUSION_STATE and rows[0, 64]["map_plane"] == 64
    assert fr[0]["n_updated"] == 65 and not rows[0, 65:].view(np.uint8).any()

"""cape_match_map_wide: MapPlane::find_matches against the persistent map for frames of up to 128 kept planes, record chains included.
Pinned to cape_match_map on the frames both serve (equal decisions, bit-identical areas), checked bit for bit against the host twin
cape_host_match_map -- which has no limit on the detected planes -- and in its decisions against the oracle of the reference's algorithm
on frames of 17..64 and of more than 64 kept planes, a map plane with a hole over a plane of a spill record included, and for its flags,
argument checks and determinism."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 128  # cape_amd.MATCH_MAP_WIDE_MAX_PLANES (asserted below)
EYE = (np.eye(3), np.zeros(3))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _extract(frames, width, height, intr, build=None):
    import torch
    from cape_amd import Extractor

    n = len(frames)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    ex = Extractor(width, height, cylinders=False, max_batch=n, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n if build is None else build, st)
    return ex, st


def _compare_with_twin(ex, n, kept, planes, T, flags, oracle=False):
    """every frame of the last match_map_wide against cape_host_match_map on the kept planes of the whole chains (none may be flagged);
    returns the copied results"""
    import cape_amd

    arrays = cape_amd.pack_map(planes)
    frames, match, seg_cur, map_of, inter = ex.map_matches_wide(n, areas=True)
    assert match.shape == (n, len(planes)) and inter.shape == (n, len(planes), W)
    for f in range(n):
        det, segs = kept[f]
        g = frames[f]
        assert (g["n_map"], g["n_cur"]) == (len(planes), len(det)), f"frame {f}: counts"
        assert g["flags"] == 0, f"frame {f} is flagged"
        assert list(seg_cur[f, : len(det)]) == segs and np.all(seg_cur[f, len(det):] == -1)
        m, mo, ia = cape_amd.host_match_map(arrays, det, T[f], None, flags, areas=True)
        assert list(match[f]) == list(m), f"frame {f}"
        assert list(map_of[f, : len(det)]) == list(mo) and np.all(map_of[f, len(det):] == -1)
        assert g["n_matched"] == sum(1 for v in m if v >= 0)
        bad = np.argwhere(_bits(inter[f][:, : len(det)]) != _bits(ia))
        assert len(bad) == 0, f"frame {f}: areas differ from the host class at {bad[:4].tolist()}"
        assert np.all(inter[f][:, len(det):] == -1.0)
        if oracle:
            from test_gpu_map_match import _oracle_decisions

            assert list(match[f]) == _oracle_decisions(det, planes, T[f], None, flags), f"frame {f}: decisions differ from the reference's algorithm"
    return frames, match, seg_cur, map_of, inter


def test_narrow_frames_equal_match_map():
    """Eight room frames with the poses of their trajectory and a map lifted from two of them: what cape_match_map serves, the wide call
    serves alike -- counts, segment lists, matches, and every entry of the area table bit for bit -- with host skip words under each
    flag, and with the skip words of cape_map_visibility."""
    import cape_amd
    from test_gpu_map_match import _kept, _map_from, _stream, _w2c

    assert W == cape_amd.MATCH_MAP_WIDE_MAX_PLANES == cape_amd.MATCH_WIDE_MAX_PLANES
    n, M = 8, 64
    ex, st, c2w = _stream("room", 11, 20, 5, n)
    rng = np.random.default_rng(7)
    planes = _map_from(_kept(ex, n), c2w, (0, 5), rng)
    ex.upload_map(planes)
    T = np.stack([_w2c(*c2w[f]) for f in range(n)])
    words = (len(planes) + 31) // 32
    for flags, device_skip in ((0, False), (cape_amd.MATCH_ADVANCED, False), (cape_amd.MATCH_ALLOW_INDEX0, False), (0, True)):
        skip = None
        if device_skip:
            ex.map_visibility(n, T)
            flags |= cape_amd.MATCH_MAP_DEVICE_SKIP
        else:
            skip = rng.integers(0, 2**32, (n, words), dtype=np.uint64).astype(np.uint32) & np.uint32(0x11111111)
        ex.match_map(n, T, skip, flags | cape_amd.MATCH_MAP_AREAS, st)
        ex.match_map_wide(n, T, skip, flags | cape_amd.MATCH_MAP_AREAS, st)
        narrow, nmatch, ninter = ex.map_matches(n, areas=True)
        frames, match, seg_cur, map_of, inter = ex.map_matches_wide(n, areas=True)
        assert np.array_equal(frames["flags"], narrow["flags"])
        assert int((nmatch >= 0).sum()) > 0 and np.count_nonzero(ninter > 0) > n, "the comparison would pass on empty results"
        for name in ("n_map", "n_cur", "n_matched"):
            assert np.array_equal(frames[name], narrow[name]), name
        assert np.array_equal(match, nmatch)
        assert np.array_equal(seg_cur[:, :M], narrow["seg_cur"]) and np.array_equal(map_of[:, :M], narrow["map_of"])
        assert np.all(seg_cur[:, M:] == -1) and np.all(map_of[:, M:] == -1)
        assert np.array_equal(_bits(inter[:, :, :M]), _bits(ninter)), "the area tables differ"
        assert np.all(inter[:, :, M:] == -1.0)
        # without the table the decisions are the same, and the table is refused
        ex.match_map_wide(n, T, skip, flags, st)
        again = ex.map_matches_wide(n)
        assert np.array_equal(again[0], frames) and all(np.array_equal(a, b) for a, b in zip(again[1:], (match, seg_cur, map_of)))
        with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
            ex.map_matches_wide(n, areas=True)
    ex.close()


def test_17_to_64_kept_planes():
    """The checkerboard of facets against a map of its own kept planes, seen through a camera that moved a few millimetres: bit for
    bit like the host twin and with the decisions of the reference's algorithm, kept-plane indices beyond 15 included."""
    import cape_amd
    from cape_amd import synth
    from test_gpu_map_match import _checker_frames, _lift
    from test_gpu_match_wide import _small_pose

    big, intr = _checker_frames(640, 480, 80)
    ex, st = _extract(np.stack([big, synth.room(seed=2, frame=5, width=640, height=480, intr=intr)]), 640, 480, intr)
    kept = ex.kept_planes(2)
    assert 16 < len(kept[0][0]) <= 64
    planes = [_lift(k, *EYE) for k in kept[0][0]]
    ex.upload_map(planes)
    T = _small_pose(2)  # (shifted outlines: see test_gpu_map_match._oracle_decisions)
    for flags in (0, cape_amd.MATCH_ADVANCED, cape_amd.MATCH_ALLOW_INDEX0):
        ex.match_map_wide(2, T, None, flags | cape_amd.MATCH_MAP_AREAS, st)
        fr, match, _, _, inter = _compare_with_twin(ex, 2, kept, planes, T, flags, oracle=True)
        assert int(match[0].max()) >= 16, "kept planes beyond the first 16 are matched"
        assert np.count_nonzero(inter[0] > 0) >= fr[0]["n_cur"] - 1
    ex.close()


def _circle(c, r, k):
    a = np.linspace(0, 2 * math.pi, k, endpoint=False)
    return np.stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)], 1)


@functools.lru_cache(maxsize=None)
def _chained_input():
    from cape_amd import synth
    from test_gpu_map_match import _checker_frames

    Wd, Ht = 1280, 960
    big, intr = _checker_frames(Wd, Ht, 100)
    room = synth.room(seed=1, frame=0, width=Wd, height=Ht, intr=intr)
    return np.stack([room, big, room]), Wd, Ht, intr


def _chained_frame():
    """[room, checkerboard of 116 plane segments in two records, room] at 1280 x 960, and the map of the checkerboard's own kept planes:
    more than 64 map planes, one of the first record and the last one of the spill record with a hole inside its detected counterpart.
    Returns (ex, st, kept, planes, planes without the holes, the holed map planes)."""
    from test_gpu_map_match import _lift

    frames, Wd, Ht, intr = _chained_input()
    ex, st = _extract(frames, Wd, Ht, intr)
    res = ex.results(3)
    assert len(res.segments(1)) == 116 and len(res.chain(1)) == 2
    kept = ex.kept_planes(3)
    det, segs = kept[1]
    assert len(det) > 64 and segs[-1] >= 64, "the chain keeps planes of its second record"
    plain = [_lift(k, *EYE) for k in det]
    holed = (5, len(det) - 1)
    assert segs[holed[1]] >= 64
    planes = list(plain)
    for h in holed:
        k = det[h]
        planes[h] = _lift(k, *EYE, holes=[_circle(k[5].mean(0), 0.15 * math.sqrt(k[6] / math.pi), 6)])
    return ex, st, kept, planes, plain, holed


def test_a_chained_frame():
    """A frame of 116 plane segments lives in two records.  It is served against a map of more than 64 planes: kept planes counted over
    the whole chain, those of the spill record reached through the kept-plane table -- by the hole loop as well -- results bit for bit
    the twin's.  cape_match_map still flags the frame, and its results are not disturbed."""
    import cape_amd
    from test_gpu_match_wide import _small_pose

    ex, st, kept, planes, plain, holed = _chained_frame()
    n_big = len(kept[1][0])
    assert len(planes) == n_big > 64
    ex.upload_map(planes)
    T = _small_pose(3)
    ex.match_map(3, T, None, cape_amd.MATCH_MAP_AREAS, st)
    before = ex.map_matches(3, areas=True)
    assert before[0][1]["flags"] & cape_amd.MATCH_EXACT_OVERFLOW and not before[0][0]["flags"] and np.all(before[1][1] == -1)
    for flags in (0, cape_amd.MATCH_ADVANCED, cape_amd.MATCH_ALLOW_INDEX0):
        ex.match_map_wide(3, T, None, flags | cape_amd.MATCH_MAP_AREAS, st)
        fr, match, _, map_of, inter = _compare_with_twin(ex, 3, kept, planes, T, flags)
        assert fr[1]["n_cur"] == n_big and int(match[1].max()) >= 64 and int(map_of[1, 64:n_big].max()) >= 0
        assert fr[1]["n_matched"] > 64, "the frame finds its own planes, in both records"
        # the hole takes its share of the intersection, in the spill record too
        _, _, whole = cape_amd.host_match_map(cape_amd.pack_map(plain), kept[1][0], T[1], None, flags, areas=True)
        for h in holed:
            assert 0.0 < inter[1, h, h] < whole[h, h], f"map plane {h}"
        others = [j for j in range(n_big) if j not in holed]
        assert np.array_equal(_bits(inter[1][others][:, :n_big]), _bits(whole[others]))
    after = ex.map_matches(3, areas=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)), "cape_match_map's results were disturbed"
    ex.close()


def test_flags_and_arguments():
    """More than 128 kept planes and a plane left to the host class flag their frame, and nothing else; the argument checks."""
    import cape_amd
    from cape_amd import synth
    from test_gpu_map_match import _checker_frames, _lift
    from test_gpu_match_wide import _perforated_wall

    # a checkerboard of 139 facets at 1920 x 1080 (three records): beyond the wide tables, the twin answers
    Wd, Ht = 1920, 1080
    big, intr = _checker_frames(Wd, Ht, 120)
    ex, st = _extract(np.stack([big, big]), Wd, Ht, intr)
    (det, segs), _ = ex.kept_planes(2)
    assert len(det) == 139 and len(ex.results(2).chain(0)) == 3
    planes = [_lift(k, *EYE, ring=k[5] + [7.0, 5.0]) for k in det[::7]]
    ex.upload_map(planes)
    ex.match_map_wide(1, None, None, cape_amd.MATCH_MAP_AREAS, st)
    fr, match, seg_cur, map_of, inter = ex.map_matches_wide(1, areas=True)
    assert fr[0]["flags"] == cape_amd.MATCH_EXACT_OVERFLOW and fr[0]["n_cur"] == 139 and fr[0]["n_map"] == len(planes)
    assert np.all(match == -1) and np.all(map_of == -1) and fr[0]["n_matched"] == 0 and np.all(inter == -1.0)
    assert list(seg_cur[0]) == segs[:W]  # the first 128 positions
    m, _ = cape_amd.host_match_map(cape_amd.pack_map(planes), det, None, None, 0)
    assert sum(1 for v in m if v >= 0) > len(planes) // 2, "the twin gives the frame's answer: its own planes are found"
    ex.close()

    # a plane of more boundary candidates than the device hull takes: CAPE_POLY_OVERFLOW flags its frame only
    Wd, Ht = 1280, 960
    intr = {k: v * 2.0 for k, v in synth.DEFAULT_INTRINSICS.items()}
    rooms = [synth.room(seed=1, frame=f, width=Wd, height=Ht, intr=intr) for f in (0, 3)]
    ex, st = _extract(np.stack([rooms[0], _perforated_wall(Wd, Ht, intr), rooms[1]]), Wd, Ht, intr, build=2)
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):  # no map uploaded
        ex.match_map_wide(2, None, None, 0, st)
    kept = ex.kept_planes(2)
    planes = [_lift(k, *EYE, ring=k[5] + [7.0, 5.0]) for k in kept[0][0]]
    assert len(planes) >= 3
    ex.upload_map(planes)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # frame 2 has no polygons yet
        ex.match_map_wide(3, None, None, 0, st)
    ex.build_polygons(3, st)
    pol, _ = ex.polygons(3)
    assert (pol[1]["flags"] & cape_amd.POLY_OVERFLOW).any() and not (pol[[0, 2]]["flags"] & cape_amd.POLY_OVERFLOW).any()
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.match_map_wide(3, None, None, 1 << 7, st)
    words = np.zeros((3, 1), np.uint32)
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.match_map_wide(3, None, words, cape_amd.MATCH_MAP_DEVICE_SKIP, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # no cape_map_visibility since the upload
        ex.match_map_wide(3, None, None, cape_amd.MATCH_MAP_DEVICE_SKIP, st)
    ex.match_map_wide(3, None, None, cape_amd.MATCH_MAP_AREAS | cape_amd.MATCH_ALLOW_INDEX0, st)
    fr, match, _, map_of, inter = ex.map_matches_wide(3, areas=True)
    assert [int(f) for f in fr["flags"]] == [0, cape_amd.MATCH_EXACT_OVERFLOW, 0]
    assert np.all(match[1] == -1) and np.all(map_of[1] == -1) and fr[1]["n_matched"] == 0 and np.all(inter[1] == -1.0)
    assert fr[0]["n_matched"] > 0 and np.count_nonzero(inter[2] > 0) > 0, "the frames around the wall are served"
    # the copy: no more frames than the call covered; n_map is that of the call, whatever is uploaded later
    ex.match_map_wide(2, None, None, cape_amd.MATCH_ALLOW_INDEX0, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):
        ex.map_matches_wide(3)
    n_map = len(planes)
    ex.upload_map(planes[:2])
    fr2, match2, _, _ = ex.map_matches_wide(2)
    assert match2.shape == (2, n_map) and np.all(fr2["n_map"] == n_map) and np.array_equal(match2, match[:2])
    ex.match_map_wide(2, None, None, 0, st)
    assert ex.map_matches_wide(2)[1].shape == (2, 2)
    # an empty map: nothing matched
    ex.upload_map([])
    ex.match_map_wide(3, None, None, 0, st)
    fr, match, seg_cur, map_of = ex.map_matches_wide(3)
    assert match.shape == (3, 0) and np.all(map_of == -1) and np.all(fr["n_matched"] == 0) and np.all(fr["n_map"] == 0)
    assert fr[0]["n_cur"] == len(kept[0][0]) and list(seg_cur[0, : fr[0]["n_cur"]]) == kept[0][1]
    ex.close()


def test_determinism():
    """The chained frame's call twice on one handle and once on a fresh one: all five arrays byte for byte."""
    import cape_amd
    from test_gpu_match_wide import _small_pose

    T = _small_pose(3)
    runs = []
    for handle in range(2):
        ex, st, kept, planes, _, _ = _chained_frame()
        ex.upload_map(planes)
        for _ in range(2 - handle):
            ex.match_map_wide(3, T, None, cape_amd.MATCH_MAP_AREAS, st)
            runs.append(ex.map_matches_wide(3, areas=True))
        ex.close()
    assert len(runs) == 3 and int(runs[0][0]["n_matched"].sum()) > 64 and np.all(runs[0][0]["flags"] == 0)
    for other in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], other))


def test_outlines_beyond_128_vertices_equal_match_map():
    """The stream of test_polygon_matches_1280x960_outlines_beyond_128_vertices (64 tumlike frames of 1280 x 960, cylinders on) against
    a map lifted from the kept planes of the frame with the longest outline (more than 128 vertices): both intersection kernels hand
    pairs on up to the last tier, and the wide call serves what cape_match_map serves -- counts, segment lists, matches, and every
    entry of the area table bit for bit; no frame flagged."""
    import torch
    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu
    from test_gpu_map_match import _lift
    from test_gpu_match_wide import _small_pose

    n, M = 64, 64
    intr = {k: v * 2.0 for k, v in synth.TUM_FR1_INTRINSICS.items()}
    dev = synth_gpu.stream("tumlike", 17, n, width=1280, height=960, start=256, device="cuda", chunk=4)
    ex = Extractor(1280, 960, cylinders=True, max_batch=n, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    kept = ex.kept_planes(n)
    longest = [max((len(k[5]) for k in det), default=0) for det, _ in kept]
    source = int(np.argmax(longest))
    assert longest[source] > 128, "the stream must show an outline the 128-vertex tiers cannot hold"
    planes = [_lift(k, *EYE) for k in kept[source][0]]
    ex.upload_map(planes)
    T = _small_pose(n)
    ex.match_map(n, T, None, cape_amd.MATCH_MAP_AREAS, st)
    assert ex.map_match_lists()["tiers"][2] > 0, "no pair reached the last tier"
    ex.match_map_wide(n, T, None, cape_amd.MATCH_MAP_AREAS, st)
    assert ex.map_match_lists()["tiers"][2] > 0, "no pair reached the last tier"
    narrow, nmatch, ninter = ex.map_matches(n, areas=True)
    frames, match, seg_cur, map_of, inter = ex.map_matches_wide(n, areas=True)
    assert not narrow["flags"].any() and not frames["flags"].any(), "a frame is flagged"
    assert int((nmatch >= 0).sum()) > 0 and np.count_nonzero(ninter > 0) > n, "the comparison would pass on empty results"
    for name in ("n_map", "n_cur", "n_matched"):
        assert np.array_equal(frames[name], narrow[name]), name
    assert np.array_equal(match, nmatch)
    assert np.array_equal(seg_cur[:, :M], narrow["seg_cur"]) and np.array_equal(map_of[:, :M], narrow["map_of"])
    assert np.all(seg_cur[:, M:] == -1) and np.all(map_of[:, M:] == -1)
    assert np.array_equal(_bits(inter[:, :, :M]), _bits(ninter)), "the area tables differ"
    assert np.all(inter[:, :, M:] == -1.0)
    ex.close()

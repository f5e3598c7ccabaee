"""cape_match_polygons_wide: MapPlane::find_matches between consecutive frames of up to 128 kept planes, record chains included.
Pinned to the shipped 16-plane path on frames both serve (equal matches, bit-identical areas), checked bit for bit against the host
twin cape_host_match_planes and in its decisions against the oracle of the reference's algorithm on frames of 17..64 and of more than
64 kept planes, and for its flags and argument checks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 128  # cape_amd.MATCH_WIDE_MAX_PLANES (asserted below)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _extract(frames, width, height, intr, build=None, **kw):
    import torch
    from cape_amd import Extractor

    n = len(frames)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    ex = Extractor(width, height, cylinders=False, max_batch=n, **intr, **kw)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n if build is None else build, st)
    return ex, st


def _small_pose(n):
    """a camera that moves a few millimetres and a fraction of a degree between the frames: every plane still passes the gates, no
    outline coincides with its predecessor's"""
    a = 0.004
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [7.0, 5.0, 3.0]
    return np.stack([T] * n)


def _compare_with_twin(ex, n, T, flags, kept, oracle=False):
    """every frame of the last match_polygons_wide against cape_host_match_planes on the kept planes of the whole chains; returns the
    copied results"""
    import cape_amd

    frames, match, seg_prev, seg_cur, inter = ex.polygon_matches_wide(n, areas=True)
    for f in range(n):
        (prev, prev_segs), (cur, cur_segs) = (kept[f - 1] if f else ([], [])), kept[f]
        g = frames[f]
        assert (g["n_prev"], g["n_cur"]) == (len(prev), len(cur)), f"frame {f}: plane counts"
        assert g["flags"] == 0, f"frame {f} is flagged"
        assert list(seg_prev[f, : len(prev)]) == prev_segs and np.all(seg_prev[f, len(prev):] == -1)
        assert list(seg_cur[f, : len(cur)]) == cur_segs and np.all(seg_cur[f, len(cur):] == -1)
        m, ia = cape_amd.host_match_planes(prev, cur, None if T is None else T[f], flags, areas=True)
        assert list(match[f, : len(prev)]) == list(m), f"frame {f}"
        assert np.all(match[f, len(prev):] == -1) and g["n_matched"] == sum(1 for v in m if v >= 0)
        bad = np.argwhere(_bits(inter[f, : len(prev), : len(cur)]) != _bits(ia))
        assert len(bad) == 0, f"frame {f}: areas differ from the host class at {bad[:4].tolist()}"
        assert np.all(inter[f, len(prev):] == -1.0) and np.all(inter[f, :, len(cur):] == -1.0)
        if oracle and f:
            from test_gpu_map_match import _oracle_decisions

            planes = [(nn, d, x, y, c, ring, []) for nn, d, x, y, c, ring, _ in prev]
            want = _oracle_decisions(cur, planes, np.eye(4) if T is None else T[f], None, flags)
            assert list(match[f, : len(prev)]) == want, f"frame {f}: decisions differ from the reference's algorithm"
    return frames, match, seg_prev, seg_cur, inter


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_narrow_frames_equal_the_16_plane_path(flags):
    """Eight room frames with the relative poses of their trajectory: what cape_match_polygons_pose serves, the wide call serves
    alike -- counts, segment lists, matches, and every entry of the area table bit for bit."""
    import torch
    import cape_amd
    from cape_amd import Extractor, synth
    from test_gpu_match_pose import _strided

    assert W == cape_amd.MATCH_WIDE_MAX_PLANES
    n, M = 8, cape_amd.MATCH_MAX_PLANES
    dev, T = _strided("room", 31, 40, 9, n)
    assert not np.allclose(T[1], np.eye(4))
    ex = Extractor(640, 480, cylinders=False, max_batch=n, **synth.DEFAULT_INTRINSICS)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    ex.match_polygons_pose(n, T, flags, st)
    ex.match_polygons_wide(n, T, flags | cape_amd.MATCH_MAP_AREAS, st)
    narrow = ex.polygon_matches(n)
    frames, match, seg_prev, seg_cur, inter = ex.polygon_matches_wide(n, areas=True)
    assert np.all(narrow["flags"] == 0) and np.all(frames["flags"] == 0)
    assert np.array_equal(frames["n_prev"], narrow["n_prev"]) and np.array_equal(frames["n_cur"], narrow["n_cur"])
    assert int((narrow["match"] >= 0).sum()) > 0 and np.count_nonzero(narrow["inter_area"] > 0) > n
    for name, wide in (("match", match), ("seg_prev", seg_prev), ("seg_cur", seg_cur)):
        assert np.array_equal(wide[:, :M], narrow[name]), name
        assert np.all(wide[:, M:] == -1), name
    assert np.array_equal(frames["n_matched"], (narrow["match"] >= 0).sum(1))
    assert np.array_equal(_bits(inter[:, :M, :M]), _bits(narrow["inter_area"])), "the area tables differ"
    assert np.all(inter[:, M:] == -1.0) and np.all(inter[:, :, M:] == -1.0)
    # without the table the decisions are the same, and the table is refused
    ex.match_polygons_wide(n, T, flags, st)
    assert np.array_equal(ex.polygon_matches_wide(n)[1], match)
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.polygon_matches_wide(n, areas=True)
    ex.close()


def test_17_to_64_kept_planes():
    """The checkerboard of facets that cape_match_polygons flags (more than 16 kept planes), twice, then a room frame: served here,
    bit for bit like the host twin and with the decisions of the reference's algorithm, kept-plane indices beyond 15 included."""
    import cape_amd
    from cape_amd import synth
    from test_gpu_map_match import _checker_frames

    big, intr = _checker_frames(640, 480, 80)
    frames = np.stack([big, big, synth.room(seed=2, frame=5, width=640, height=480, intr=intr)])
    ex, st = _extract(frames, 640, 480, intr)
    kept = ex.kept_planes(3)
    T = _small_pose(3)  # (shifted outlines: see test_gpu_map_match._oracle_decisions)
    for flags in (0, cape_amd.MATCH_ALLOW_INDEX0):
        ex.match_polygons_wide(3, T, flags | cape_amd.MATCH_MAP_AREAS, st)
        fr, match, _, _, inter = _compare_with_twin(ex, 3, T, flags, kept, oracle=True)
        assert 16 < fr[1]["n_cur"] <= 64 and fr[1]["n_cur"] == len(kept[1][0])
        assert int(match[1].max()) >= 16, "kept planes beyond the first 16 are matched"
        assert np.count_nonzero(inter[1] > 0) >= fr[1]["n_cur"] - 1
    ex.match_polygons(3, 0, st)
    narrow = ex.polygon_matches(3)
    assert narrow[1]["flags"] & cape_amd.MATCH_EXACT_OVERFLOW and narrow[2]["flags"] & cape_amd.MATCH_EXACT_OVERFLOW
    ex.close()


def test_a_chained_frame():
    """A frame of 116 plane segments lives in two records.  Every frame around it is served: kept planes counted over the whole chain,
    those of the spill record reached through the kept-plane table, results bit for bit the twin's."""
    import cape_amd
    from cape_amd import synth
    from test_gpu_map_match import _checker_frames

    Wd, Ht = 1280, 960
    big, intr = _checker_frames(Wd, Ht, 100)
    room = synth.room(seed=1, frame=0, width=Wd, height=Ht, intr=intr)
    ex, st = _extract(np.stack([room, big, big, room]), Wd, Ht, intr)
    res = ex.results(4)
    assert len(res.segments(1)) == 116 and len(res.chain(1)) == 2
    kept = ex.kept_planes(4)
    assert len(kept[1][0]) > 64 and kept[1][1][-1] >= 64, "the chain keeps planes of its second record"
    for flags in (0, cape_amd.MATCH_ALLOW_INDEX0):
        ex.match_polygons_wide(4, None, flags | cape_amd.MATCH_MAP_AREAS, st)
        fr, match, _, _, _ = _compare_with_twin(ex, 4, None, flags, kept)
        n_big = len(kept[1][0])
        assert fr[1]["n_cur"] == n_big and fr[2]["n_prev"] == n_big and n_big > 64
        # the frame against itself: every plane finds itself, but plane 0 (the `selectedIndex <= 0` quirk) unless asked for
        want = np.arange(n_big)
        if not flags:
            want[0] = -1
        assert np.array_equal(match[2, :n_big], want)
        assert int(match[2].max()) >= 64
    T = _small_pose(4)
    ex.match_polygons_wide(4, T, cape_amd.MATCH_ADVANCED | cape_amd.MATCH_MAP_AREAS, st)
    _, match, _, _, _ = _compare_with_twin(ex, 4, T, cape_amd.MATCH_ADVANCED, kept)
    assert int(match[2].max()) >= 64
    ex.match_polygons(4, 0, st)
    narrow = ex.polygon_matches(4)
    assert all(narrow[f]["flags"] & cape_amd.MATCH_EXACT_OVERFLOW for f in (1, 2, 3))
    ex.close()


def _perforated_wall(width, height, intr):
    """A wall with every other cell of every other cell row missing: ONE plane whose region touches a hole almost everywhere, so that
    it has more boundary candidates (1 565 at 1280 x 960) than the device hull takes: CAPE_POLY_OVERFLOW."""
    z = np.round(2000.0 + np.random.default_rng(5).normal(0, 0.6, (height, width))).astype(np.float32)
    for r in range(1, height // 20, 2):
        for c in range(1, width // 20, 2):
            z[r * 20:(r + 1) * 20, c * 20:(c + 1) * 20] = 0
    return z


def test_flags_and_arguments():
    """A plane left to the host class flags its frame and the next one; the argument checks.  (No input of the existing polygon tests
    is certain to hold a plane of more than 1 024 boundary candidates: the perforated wall is made for it.)"""
    import cape_amd
    from cape_amd import synth

    Wd, Ht = 1280, 960
    intr = {k: v * 2.0 for k, v in synth.DEFAULT_INTRINSICS.items()}
    rooms = [synth.room(seed=1, frame=f, width=Wd, height=Ht, intr=intr) for f in (0, 3, 6)]
    ex, st = _extract(np.stack([rooms[0], rooms[1], _perforated_wall(Wd, Ht, intr), rooms[2]]), Wd, Ht, intr, build=3)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # frame 3 has no polygons yet
        ex.match_polygons_wide(4, None, 0, st)
    ex.build_polygons(4, st)
    pol, _ = ex.polygons(4)
    assert (pol[2]["flags"] & cape_amd.POLY_OVERFLOW).any() and not (pol[[0, 1, 3]]["flags"] & cape_amd.POLY_OVERFLOW).any()
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.match_polygons_wide(4, None, 1 << 7, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-1\)"):
        ex.match_polygons_wide(4, None, cape_amd.MATCH_MAP_DEVICE_SKIP, st)
    ex.match_polygons_wide(4, None, cape_amd.MATCH_MAP_AREAS, st)
    fr, match, _, _, inter = ex.polygon_matches_wide(4, areas=True)
    assert [int(f) for f in fr["flags"]] == [0, 0, cape_amd.MATCH_EXACT_OVERFLOW, cape_amd.MATCH_EXACT_OVERFLOW]
    assert np.all(match[2:] == -1) and np.all(fr["n_matched"][2:] == 0) and np.all(inter[2:] == -1.0)
    assert np.count_nonzero(inter[1] > 0) > 0, "the frames in front of the wall are served"
    ex.match_polygons_wide(2, None, 0, st)
    with pytest.raises(cape_amd.CapeError, match=r"\(-4\)"):  # more frames than the last call covered
        ex.polygon_matches_wide(3)
    assert ex.polygon_matches_wide(2)[0]["n_matched"][1] == fr[1]["n_matched"]
    ex.close()


def test_more_than_128_kept_planes_are_flagged_and_the_twin_answers():
    """A checkerboard of 139 facets at 1920 x 1080 (three records): beyond the wide tables, so both frames are flagged with their
    true counts, and cape_host_match_planes -- no limit -- gives the answer from the kept planes of the chains."""
    import cape_amd
    from test_gpu_map_match import _checker_frames

    Wd, Ht = 1920, 1080
    big, intr = _checker_frames(Wd, Ht, 120)
    ex, st = _extract(np.stack([big, big]), Wd, Ht, intr)
    kept = ex.kept_planes(2)
    n_big = len(kept[0][0])
    assert n_big > W and len(ex.results(2).chain(1)) == 3
    ex.match_polygons_wide(2, None, cape_amd.MATCH_MAP_AREAS, st)
    fr, match, seg_prev, seg_cur, inter = ex.polygon_matches_wide(2, areas=True)
    assert [int(f) for f in fr["flags"]] == [cape_amd.MATCH_EXACT_OVERFLOW] * 2
    assert list(fr["n_cur"]) == [n_big, n_big] and list(fr["n_prev"]) == [0, n_big]
    assert np.all(match == -1) and np.all(fr["n_matched"] == 0) and np.all(inter == -1.0)
    assert list(seg_cur[1]) == kept[1][1][:W] and list(seg_prev[1]) == kept[0][1][:W]  # the first 128 positions
    m = cape_amd.host_match_planes(kept[0][0], kept[1][0], None, 0)
    assert list(m) == [-1] + list(range(1, n_big))
    ex.close()


def test_outlines_beyond_128_vertices_equal_the_16_plane_path():
    """The stream of test_polygon_matches_1280x960_outlines_beyond_128_vertices (64 tumlike frames of 1280 x 960, cylinders on): a
    gated pair with an outline of more than 128 vertices is handed from tier to tier up to the last one by the wide intersection
    kernel as by the 16-plane one -- counts, matches, segment lists, and every entry of the area table bit for bit; no frame flagged."""
    import torch
    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu

    n, M = 64, cape_amd.MATCH_MAX_PLANES
    intr = {k: v * 2.0 for k, v in synth.TUM_FR1_INTRINSICS.items()}
    dev = synth_gpu.stream("tumlike", 17, n, width=1280, height=960, start=256, device="cuda", chunk=4)
    ex = Extractor(1280, 960, cylinders=True, max_batch=n, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), n, st)
    ex.build_polygons(n, st)
    ex.match_polygons(n, 0, st)
    ex.match_polygons_wide(n, None, cape_amd.MATCH_MAP_AREAS, st)
    narrow = ex.polygon_matches(n)
    frames, match, seg_prev, seg_cur, inter = ex.polygon_matches_wide(n, areas=True)
    assert not narrow["flags"].any() and not frames["flags"].any(), "a frame is flagged"
    # a pair of the last tier: a kept outline of more than 128 vertices that passes the gates against a plane of the next frame
    pol, _ = ex.polygons(n)
    long_pairs = 0
    for f in range(1, n):
        for j in range(int(frames[f]["n_prev"])):
            if pol[f - 1, seg_prev[f, j]]["vertex_count"] > 128:
                long_pairs += int(np.count_nonzero(inter[f, j] != -1.0))
    assert long_pairs > 0, "the stream must show a gated pair the 128-vertex tiers cannot hold"
    assert np.array_equal(frames["n_prev"], narrow["n_prev"]) and np.array_equal(frames["n_cur"], narrow["n_cur"])
    assert int((narrow["match"] >= 0).sum()) > 0 and np.count_nonzero(narrow["inter_area"] > 0) > n
    for name, wide in (("match", match), ("seg_prev", seg_prev), ("seg_cur", seg_cur)):
        assert np.array_equal(wide[:, :M], narrow[name]), name
        assert np.all(wide[:, M:] == -1), name
    assert np.array_equal(frames["n_matched"], (narrow["match"] >= 0).sum(1))
    assert np.array_equal(_bits(inter[:, :M, :M]), _bits(narrow["inter_area"])), "the area tables differ"
    assert np.all(inter[:, M:] == -1.0) and np.all(inter[:, :, M:] == -1.0)
    ex.close()

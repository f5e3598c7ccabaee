"""cape_map_pose_score on the device against its host twin cape_host_pose_score, which compiles the same rules header.

What must agree, per (frame, hypothesis, pair):
  * the feature rows, n_pairs, n_invalid, the flags, reduced[3], signed[3] (the distance part) and sum_sq: BIT FOR BIT;
  * the three angle parts of signed, atan2(sin(x), cos(x)) through ocml on the device and through the C library on the host: a bound in
    units in the last place.  MEASURED on the MI355X over the sets of this file: at most ANGLE_ULPS_MEASURED = 1 ulp from the twin
    in every set (room frames, the six hypothesis counts, the five map sizes, the chained frame, the flagged batch, the straddle cases:
    1 ulp each); asserted: twice that, 2 ulp -- the sets only sample, so the margin is one factor of two.  Where the twin's value is exactly 0 the device's must be 0;
  * inlier_words, n_inliers and score: EQUAL wherever no angle part of the twin lies within NEAR = 1e-12 of its threshold (three orders
    above a few ulp at 0.2).  The share left out for nearness is computed from the twin's values alone, before the device's results are
    looked at, and must be 0 on every set (the straddle cases sit 2e-10 from the threshold, and are decided exactly).

Every test prints its figures before it asserts (`pytest -s`)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 128
ANGLE_ULPS_MEASURED = 1
ANGLE_ULPS = 2 * ANGLE_ULPS_MEASURED
NEAR = 1e-12
EYE = (np.eye(3), np.zeros(3))


def _det_planes(det):
    """(n_cur, 4): the kept planes' (normal, d) as the twin takes them -- out_normal and d of their segments"""
    return np.array([[*k[0], k[1]] for k in det], np.float64).reshape(-1, 4)


def _hypotheses(rng, base, n_hyp, angle=math.radians(3.0), shift=100.0):
    """(n, n_hyp, 4, 4): per frame its pose (hypothesis 0) and perturbed ones -- a rotation of up to a few degrees, a translation of up
    to about 100 mm in front of it: the angle parts stay inliers, the distance part does not always"""
    from test_pose_score_host import _pose

    out = np.empty((len(base), n_hyp, 4, 4))
    for f, T in enumerate(base):
        for h in range(n_hyp):
            out[f, h] = T if h == 0 else _pose(rng, angle, shift if h % 4 else 8.0) @ T
    return out


def _tracks_for(rng, n):
    """tracks of a map of n planes: a valid covariance each, ids of their own"""
    import cape_amd
    from test_map_update_host import _spd

    tracks = np.zeros(n, cape_amd.MAP_TRACK_DTYPE)
    for j in range(n):
        tracks[j]["covariance"] = _spd(rng, 4, 10.0 ** rng.uniform(-4, 0))
        tracks[j]["flags"] = cape_amd.MAP_TRACK_STAGED if j % 3 == 0 else 0
        tracks[j]["id"] = 500 + 3 * j
    return tracks


class Stats:
    def __init__(self):
        self.worst = self.pairs = self.inliers = self.outliers = self.near = self.rows = 0

    def __str__(self):
        return (f"{self.rows} (frame, hypothesis) rows, {self.pairs} scored pairs: {self.inliers} inliers, {self.outliers} outliers, "
                f"{self.near} within {NEAR:g} of a threshold; angle parts at most {self.worst} ulp from the twin (bound {ANGLE_ULPS})")


def _compare_with_twin(ex, n, arrays, tracks, kept, poses, residuals=True, stats=None):
    """every frame of the last map_pose_score against cape_host_pose_score on the device's own match; returns (scores, features,
    residuals or None, stats)"""
    import cape_amd
    from test_pose_score_host import THR_ANGLE, _bits, _bits_nan, _ulps

    stats = stats or Stats()
    mframes, match, _, _ = ex.map_matches_wide(n)
    scores, res = ex.pose_scores(n, residuals=True) if residuals else (ex.pose_scores(n), None)
    features = ex.pose_features(n)
    n_hyp = poses.shape[1]
    assert scores.shape == (n, n_hyp) and features.shape == (n, W)
    for f in range(n):
        det = _det_planes(kept[f][0])
        flagged = int(mframes[f]["flags"]) & cape_amd.MATCH_EXACT_OVERFLOW
        m = match[f] if match.shape[1] else np.zeros(0, np.int32)
        ts, tf, tr = cape_amd.host_pose_score(arrays, tracks, np.full(len(m), -1, np.int32) if flagged else m, det[:W] if flagged else det, poses[f],
                                              frame_flags=flagged)
        k = int(ts[0]["n_pairs"])
        # ---- the twin's own values decide what may be compared: nothing of the device's is read here
        near = np.abs(np.abs(tr[:, :k, :3]) - THR_ANGLE) <= NEAR
        stats.near += int(near.sum())
        stats.rows += n_hyp
        stats.pairs += n_hyp * k
        stats.inliers += int(ts["n_inliers"].sum())
        stats.outliers += n_hyp * k - int(ts["n_inliers"].sum())
        assert not near.any(), f"frame {f}: {int(near.sum())} angle parts within {NEAR:g} of the threshold"
        # ---- bit for bit
        assert features[f].tobytes() == tf.tobytes(), f"frame {f}: feature rows"
        for name in ("n_pairs", "n_invalid", "flags"):
            assert np.array_equal(scores[f][name], ts[name]), f"frame {f}: {name} {scores[f][name][:4]} != {ts[name][:4]}"
        assert np.array_equal(_bits_nan(scores[f]["sum_sq"]), _bits_nan(ts["sum_sq"])), f"frame {f}: sum_sq"
        if res is not None:
            got = res[f]
            assert np.array_equal(_bits_nan(got[:, :, 3:]), _bits_nan(tr[:, :, 3:])), f"frame {f}: signed[3] / reduced"
            assert not got[:, k:].any(), f"frame {f}: residual rows beyond n_pairs"
            a, b = got[:, :k, :3], tr[:, :k, :3]
            assert np.array_equal(np.isnan(a), np.isnan(b))
            fin = np.isfinite(b)
            assert np.all(a[fin & (b == 0)] == 0), f"frame {f}: the twin's 0 is not 0 on the device"
            if fin.any():
                u = _ulps(a[fin], b[fin])
                stats.worst = max(stats.worst, int(u.max()))
        # ---- equal decisions (no pair of this frame is near a threshold)
        for name in ("n_inliers", "inlier_words"):
            assert np.array_equal(scores[f][name], ts[name]), f"frame {f}: {name}"
        assert np.array_equal(_bits(scores[f]["score"]), _bits(ts["score"])), f"frame {f}: score"
    return scores, features, res, stats


# ---- the eight room frames against their own map -------------------------------------------------------------------------------
class _Room:
    pass


@pytest.fixture(scope="module")
def room():
    import cape_amd
    from test_gpu_map_kalman import _c2w, _tracks
    from test_gpu_map_match import _stream, _w2c
    from test_gpu_map_measure import _pose_covariances

    r = _Room()
    r.n = 8
    r.ex, r.st, r.c2w = _stream("room", 11, 20, 5, r.n)
    r.T = np.stack([_c2w(*r.c2w[f]) for f in range(r.n)])
    r.W2C = np.stack([_w2c(*r.c2w[f]) for f in range(r.n)])
    r.S = _pose_covariances(np.random.default_rng(21), r.n)
    r.flags = cape_amd.MATCH_ALLOW_INDEX0
    r.ex.map_measure(r.n, r.T, r.S, r.st)
    meas = r.ex.map_measurements(r.n)
    # their own map: the stageable measurements of the first two frames with several planes, LAST FIRST -- the map's order is not the
    # kept planes'
    sources = [f for f in range(r.n) if len(meas[f]) > 1][:2]
    r.map_meas = [m for f in sources for m in meas[f] if m["flags"] & cape_amd.MEASURE_STAGEABLE][::-1]
    assert len(r.map_meas) > 3
    r.arrays = cape_amd.pack_map([m["plane"] for m in r.map_meas])
    r.tracks = _tracks(r.map_meas)
    r.kept = r.ex.kept_planes(r.n)
    r.poses = _hypotheses(np.random.default_rng(51), r.W2C, 24)
    r.restore = lambda: _restore(r)
    r.restore()
    yield r
    r.ex.close()


def _restore(r):
    r.ex.upload_map(r.arrays)
    r.ex.upload_tracks(r.tracks)
    r.ex.match_map_wide(r.n, r.W2C, None, r.flags, r.st)


def test_room_frames_equal_the_twin(room):
    import cape_amd

    ex, n, st = room.ex, room.n, room.st
    ex.map_pose_score(n, room.poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    scores, features, res, stats = _compare_with_twin(ex, n, room.arrays, room.tracks, room.kept, room.poses)
    print(f"\nroom frames against a map of {len(room.arrays[0])} planes: {stats}; pairs per frame {scores[:, 0]['n_pairs'].tolist()}")
    assert stats.inliers >= 1 and stats.outliers >= 1 and stats.near == 0
    assert stats.worst <= ANGLE_ULPS
    assert int(scores[:, 0]["n_pairs"].max()) >= 2 and not scores["flags"].any() and not scores["n_invalid"].any()
    # under its own pose a frame of the map's sources scores every pair as an inlier
    own = scores[:, 0]
    assert any(own[f]["n_inliers"] == own[f]["n_pairs"] > 1 for f in range(n))
    # the pair order is the map's: ascending map planes, kept planes not ascending somewhere
    orders = [features[f, : own[f]["n_pairs"]] for f in range(n)]
    assert all(np.all(np.diff(o["map_index"]) > 0) for o in orders) and any(np.any(np.diff(o["kept_plane"]) < 0) for o in orders)
    # without the per-pair table the scores are the same bytes, and the table is refused
    ex.map_pose_score(n, room.poses, 0, stream=st)
    assert ex.pose_scores(n).tobytes() == scores.tobytes() and ex.pose_features(n).tobytes() == features.tobytes()
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_pose_scores failed \(-1\)"):
        ex.pose_scores(n, residuals=True)
    # fewer frames may be copied, more may not
    assert ex.pose_scores(3).tobytes() == scores[:3].tobytes()
    ex.map_pose_score(4, room.poses[:4], 0, stream=st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_pose_scores failed \(-4\)"):
        ex.pose_scores(5)
    assert ex.pose_scores(4).tobytes() == scores[:4].tobytes()


def test_device_poses_equal_the_host_route(room):
    import torch

    import cape_amd

    ex, n, st = room.ex, room.n, room.st
    ex.map_pose_score(n, room.poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    host_route = (ex.pose_scores(n, residuals=True), ex.pose_features(n))
    dev = torch.from_numpy(np.ascontiguousarray(room.poses)).cuda()
    torch.cuda.current_stream().synchronize()
    ex.map_pose_score(n, dev.data_ptr(), cape_amd.POSE_SCORE_DEVICE_POSES | cape_amd.POSE_SCORE_RESIDUALS, n_hypotheses=room.poses.shape[1], stream=st)
    (scores, res), features = ex.pose_scores(n, residuals=True), ex.pose_features(n)
    assert scores.tobytes() == host_route[0][0].tobytes() and res.tobytes() == host_route[0][1].tobytes()
    assert features.tobytes() == host_route[1].tobytes() and int(scores["n_pairs"].sum()) > 0
    # the device pointers
    ps, pf = C.c_void_p(), C.c_void_p()
    assert ex.L.cape_pose_score_device(ex.h, C.byref(ps), C.byref(pf)) == 0 and ps.value and pf.value


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 256, 257])
def test_hypothesis_counts_at_the_lane_wave_and_workgroup_edges(room, n_hyp):
    import cape_amd

    ex, st = room.ex, room.st
    f = int(np.argmax([len(k[0]) for k in room.kept[:4]]))
    poses = _hypotheses(np.random.default_rng(60 + n_hyp), room.W2C[: f + 1], n_hyp)
    ex.map_pose_score(f + 1, poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    scores, _, _, stats = _compare_with_twin(ex, f + 1, room.arrays, room.tracks, room.kept, poses)
    print(f"\n{n_hyp} hypotheses per frame: {stats}")
    assert stats.pairs >= n_hyp and stats.worst <= ANGLE_ULPS and stats.near == 0


def test_a_hypothesis_alone_gives_the_bytes_it_gives_among_256_others(room):
    import cape_amd

    ex, st = room.ex, room.st
    f = int(np.argmax([len(k[0]) for k in room.kept[:4]]))  # (the frame of the hypothesis counts above)
    n = f + 1
    poses = _hypotheses(np.random.default_rng(71), room.W2C[:n], 257)
    ex.map_pose_score(n, poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    scores, res = ex.pose_scores(n, residuals=True)
    assert scores[f, 0]["n_pairs"] > 0 and len({s.tobytes() for s in scores[f]}) > 128, "the hypotheses give different rows"
    for h in (0, 1, 63, 64, 200, 255, 256):
        ex.map_pose_score(n, poses[:, h: h + 1], cape_amd.POSE_SCORE_RESIDUALS, stream=st)
        alone, alone_res = ex.pose_scores(n, residuals=True)
        assert alone[f, 0].tobytes() == scores[f, h].tobytes(), f"hypothesis {h}: the row depends on its company"
        assert alone_res[f, 0].tobytes() == res[f, h].tobytes(), f"hypothesis {h}: the residuals depend on its company"


def _rotation_onto(a, b):
    """the rotation that takes unit vector a onto unit vector b"""
    v, c = np.cross(a, b), float(a @ b)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + K + K @ K / (1 + c)


def test_thresholds_straddled_on_the_device(room):
    """Hypotheses made so that one part of one pair's signed distance is thr (1 -+ 1e-9), thr being the float threshold widened to
    double: below is an inlier of that part, above an outlier, on the device as on the twin -- decided exactly, 2e-10 (1e-8 mm) away."""
    import cape_amd
    from test_pose_score_host import THR_ANGLE, THR_DISTANCE

    ex, st = room.ex, room.st
    _, match, _, _ = ex.map_matches_wide(room.n)
    f = int(np.argmax((match >= 0).sum(axis=1)))
    det = _det_planes(room.kept[f][0])
    P = room.arrays[0]
    poses, want = [], []
    for j in np.flatnonzero(match[f] >= 0):
        i = int(match[f, j])
        cn, cd, nm, dm = det[i, :3], det[i, 3], P[j]["normal"], float(P[j]["d"])
        for part in range(4):
            thr = THR_DISTANCE if part == 3 else THR_ANGLE
            for sign in (1.0, -1.0):
                for side in (-1e-9, 1e-9):
                    T = np.eye(4)
                    if part < 3:
                        # the map normal rotated onto q: q[part] = cn[part] - sign thr (1 + side), the two other components those of
                        # cn, scaled to a unit vector
                        rest = [c for c in range(3) if c != part]
                        q = cn.copy()
                        q[part] = cn[part] - sign * thr * (1 + side)
                        if abs(q[part]) >= 1 or float(cn[rest] @ cn[rest]) < 1e-3:
                            continue
                        q[rest] *= math.sqrt((1 - q[part] ** 2) / float(cn[rest] @ cn[rest]))
                        T[:3, :3] = _rotation_onto(nm / np.linalg.norm(nm), q)
                        T[:3, 3] = T[:3, :3] @ nm * (dm - cd)  # qd = cd: the distance part is (about) 0
                    else:
                        T[:3, :3] = room.W2C[f][:3, :3]
                        T[:3, 3] = T[:3, :3] @ nm * (dm - (cd - sign * thr * (1 + side)))
                    poses.append(T)
                    want.append((int(j), i, part, sign, side))
    assert len(want) >= 12
    poses = np.stack(poses)[None]
    ex.map_pose_score(f + 1, np.concatenate([np.tile(np.eye(4), (f, len(want), 1, 1)), poses]) if f else poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    scores, res = ex.pose_scores(f + 1, residuals=True)
    features = ex.pose_features(f + 1)
    slot = {int(F["map_index"]): k for k, F in enumerate(features[f, : scores[f, 0]["n_pairs"]])}
    ts, _, tr = cape_amd.host_pose_score(room.arrays, room.tracks, match[f], det, poses[0])
    decided = [0, 0]
    worst = 0
    for h, (j, i, part, sign, side) in enumerate(want):
        k = slot[j]
        thr = THR_DISTANCE if part == 3 else THR_ANGLE
        for name, r in (("twin", tr), ("device", res[f])):
            value = r[h, k, part]
            assert abs(abs(value) / thr - (1 + side)) < 1e-10 and np.sign(value) == sign, f"{name}: part {part} is {value!r}"
        others_in = all(abs(tr[h, k, c]) <= (THR_DISTANCE if c == 3 else THR_ANGLE) for c in range(4) if c != part)
        inlier = side < 0 and others_in
        for name, s in (("twin", ts[h]), ("device", scores[f, h])):
            bit = bool(s["inlier_words"][i >> 5] >> (i & 31) & 1)
            assert bit == inlier, f"{name}: pair ({j}, {i}) part {part} at thr (1 {side:+g}), sign {sign:+g}: inlier bit {bit}"
        decided[part == 3] += int(others_in)
        assert scores[f, h]["inlier_words"].tolist() == ts[h]["inlier_words"].tolist() and scores[f, h]["n_inliers"] == ts[h]["n_inliers"]
        worst = max(worst, int(np.max(np.abs(res[f][h, k, :3].view(np.int64) - tr[h, k, :3].view(np.int64)))))
    print(f"\nstraddle: frame {f}, {len(slot)} pairs, {len(want)} hypotheses, {decided[0]} angle and {decided[1]} distance cases decided by the "
          f"straddled part alone; the straddled pairs' angle parts at most {worst} ulp from the twin")
    assert decided[0] >= 4 and decided[1] >= 4 and worst <= ANGLE_ULPS


# ---- maps of every size at which the pairs kernel takes another path ---------------------------------------------------------------
@pytest.fixture(scope="module")
def stream8():
    from test_gpu_map_match import _kept, _stream, _w2c

    ex, st, c2w = _stream("room", 11, 20, 5, 8)
    s = _Room()
    s.ex, s.st, s.c2w, s.n = ex, st, c2w, 8
    s.W2C = np.stack([_w2c(*c2w[f]) for f in range(8)])
    s.lifted = _kept(ex, 8)
    s.kept = ex.kept_planes(8)
    yield s
    ex.close()


@pytest.mark.parametrize("size", [1, 33, 64, 65, 1024])
def test_map_sizes_at_the_chunk_edges(stream8, size):
    import cape_amd
    from test_gpu_map_match import _map_from

    s = stream8
    rng = np.random.default_rng(100 + size)
    # the kept planes of frames 4 and 5 lifted to the world, LAST in the map; in front of them perturbed copies moved 5 m along their
    # normals, which pass no gate: the pairs lie in the map's last chunk of 64
    true = _map_from(s.lifted, s.c2w, (4, 5), rng, 0)
    fillers = [(p[0], p[1] + 5000.0, *p[2:]) for p in _map_from(s.lifted, s.c2w, (4, 5), rng, size)[: max(size - len(true), 0)]]
    planes = (fillers + true)[-size:] if size > len(true) else true[:size]
    assert len(planes) == size and 1 < len(true) < 33
    arrays, tracks = cape_amd.pack_map(planes), _tracks_for(rng, size)
    s.ex.upload_map(arrays)
    s.ex.upload_tracks(tracks)
    s.ex.match_map_wide(s.n, s.W2C, None, cape_amd.MATCH_ALLOW_INDEX0, s.st)
    poses = _hypotheses(rng, s.W2C, 5)
    s.ex.map_pose_score(s.n, poses, cape_amd.POSE_SCORE_RESIDUALS, stream=s.st)
    scores, features, _, stats = _compare_with_twin(s.ex, s.n, arrays, tracks, s.kept, poses)
    last = max((int(features[f, scores[f, 0]["n_pairs"] - 1]["map_index"]) for f in range(s.n) if scores[f, 0]["n_pairs"]), default=-1)
    print(f"\nmap of {size} planes: {stats}; pairs per frame {scores[:, 0]['n_pairs'].tolist()}, the last pair's map plane {last}")
    assert stats.worst <= ANGLE_ULPS and stats.near == 0
    if size > 1:
        assert stats.pairs > 0 and stats.inliers >= 1 and last >= size - len(true)
    if size > 64:
        assert last >= 64, "a pair of the second chunk of map planes"


# ---- a chained frame of more than 64 kept planes ----------------------------------------------------------------------------------
def test_a_chained_frame_of_65_to_128_pairs():
    import cape_amd
    from test_gpu_map_match import _lift
    from test_gpu_match_map_wide import _chained_input, _extract
    from test_gpu_match_wide import _small_pose

    frames, Wd, Ht, intr = _chained_input()
    ex, st = _extract(frames, Wd, Ht, intr)
    n = len(frames)
    kept = ex.kept_planes(n)
    det = kept[1][0]
    assert 64 < len(det) <= W
    # the map: the chained frame's own kept planes, LAST FIRST -- pair k is kept plane n_cur - 1 - k or so, the spill record's first
    planes = [_lift(k, *EYE) for k in det][::-1]
    rng = np.random.default_rng(81)
    arrays, tracks = cape_amd.pack_map(planes), _tracks_for(rng, len(planes))
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    T = _small_pose(n)
    ex.match_map_wide(n, T, None, cape_amd.MATCH_ALLOW_INDEX0, st)
    poses = _hypotheses(rng, T, 9, angle=math.radians(1.0), shift=60.0)
    ex.map_pose_score(n, poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    scores, features, _, stats = _compare_with_twin(ex, n, arrays, tracks, kept, poses)
    k = int(scores[1, 0]["n_pairs"])
    rows = features[1, :k]
    print(f"\nchained frame: {len(det)} kept planes, {k} pairs; {stats}; kept planes of the first pairs {rows['kept_plane'][:4].tolist()}")
    assert 65 <= k <= W and stats.worst <= ANGLE_ULPS and stats.near == 0
    assert int((rows["kept_plane"] >= 64).sum()) >= 1 and rows["kept_plane"][0] > rows["kept_plane"][k - 1]
    assert stats.inliers >= 1 and stats.outliers >= 1
    # bits 64 .. 127 of the inlier words are used
    assert scores[1]["inlier_words"][:, 2:].any()
    ex.close()


# ---- a frame without pairs, a flagged frame, an empty map -----------------------------------------------------------------------------
def test_no_pairs_a_flagged_frame_and_an_empty_map():
    import cape_amd
    from cape_amd import synth
    from test_gpu_map_match import _lift
    from test_gpu_match_map_wide import _extract
    from test_gpu_match_wide import _perforated_wall

    Wd, Ht = 1280, 960
    intr = {k: v * 2.0 for k, v in synth.DEFAULT_INTRINSICS.items()}
    rooms = [synth.room(seed=1, frame=f, width=Wd, height=Ht, intr=intr) for f in (0, 3)]
    ex, st = _extract(np.stack([rooms[0], _perforated_wall(Wd, Ht, intr), rooms[1]]), Wd, Ht, intr)
    kept = ex.kept_planes(3)
    planes = [_lift(k, *EYE, ring=k[5] + [7.0, 5.0]) for k in kept[0][0]]
    rng = np.random.default_rng(91)
    arrays, tracks = cape_amd.pack_map(planes), _tracks_for(rng, len(planes))
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    # frame 2 sees the map from 50 m away: no pair passes the gates
    base = np.stack([np.eye(4)] * 3)
    base[2, :3, 3] = [50000.0, -50000.0, 50000.0]
    ex.match_map_wide(3, base, None, cape_amd.MATCH_ALLOW_INDEX0, st)
    fr, match, _, _ = ex.map_matches_wide(3)
    assert [int(v) for v in fr["flags"]] == [0, cape_amd.MATCH_EXACT_OVERFLOW, 0] and fr[0]["n_matched"] > 0 and fr[2]["n_matched"] == 0
    poses = _hypotheses(rng, base, 7)
    ex.map_pose_score(3, poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    scores, features, res, stats = _compare_with_twin(ex, 3, arrays, tracks, kept, poses)
    print(f"\nflagged / empty: {stats}; flags {scores[:, 0]['flags'].tolist()}, pairs {scores[:, 0]['n_pairs'].tolist()}")
    assert scores[0, 0]["n_pairs"] == fr[0]["n_matched"] > 0
    for f, flag in ((1, cape_amd.MATCH_EXACT_OVERFLOW), (2, 0)):
        assert np.all(scores[f]["flags"] == flag) and not features[f].view(np.uint8).any() and not res[f].any()
        for name in ("n_pairs", "n_inliers", "n_invalid", "score", "sum_sq", "inlier_words"):
            assert not np.any(scores[f][name]), (f, name)
    # an empty map succeeds with headers only
    ex.upload_map(cape_amd.pack_map([]))
    ex.upload_tracks(np.zeros(0, cape_amd.MAP_TRACK_DTYPE))
    ex.match_map_wide(3, base, None, 0, st)
    ex.map_pose_score(3, poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    scores, features, res, _ = _compare_with_twin(ex, 3, cape_amd.pack_map([]), np.zeros(0, cape_amd.MAP_TRACK_DTYPE), kept, poses)
    assert [int(v) for v in scores[:, 0]["flags"]] == [0, cape_amd.MATCH_EXACT_OVERFLOW, 0]
    assert not scores["n_pairs"].any() and not scores["score"].any() and not features.view(np.uint8).any() and not res.any()
    ex.close()


def test_an_invalid_track_flags_the_frame_and_is_still_scored(room):
    import cape_amd

    ex, n, st = room.ex, room.n, room.st
    _, match, _, _ = ex.map_matches_wide(n)
    j = int(np.flatnonzero((match >= 0).sum(axis=0) >= 2)[0])
    ex.map_pose_score(n, room.poses, 0, stream=st)
    valid = ex.pose_scores(n)
    bad = room.tracks.copy()
    bad[j]["covariance"][2, 2] = -1e-6  # (its square root is a NaN: is_valid fails; cape_map_kalman would report FAIL_STATE)
    ex.upload_tracks(bad)
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_pose_score(n, room.poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    scores, features, _, stats = _compare_with_twin(ex, n, room.arrays, bad, room.kept, room.poses)
    hit = match[:, j] >= 0
    assert hit.any()
    assert np.all(scores[hit]["n_invalid"] == 1) and np.all(scores[hit]["flags"] == cape_amd.POSE_SCORE_INVALID_FEATURE)
    assert not scores[~hit]["n_invalid"].any() and not scores[~hit]["flags"].any()
    for name in ("n_pairs", "n_inliers", "score", "sum_sq", "inlier_words"):  # the standard deviations enter no distance
        assert np.array_equal(scores[name], valid[name]), name
    print(f"\ninvalid track of map plane {j}: frames {np.flatnonzero(hit).tolist()} carry INVALID_FEATURE; {stats}")
    room.restore()


# ---- bookkeeping ----------------------------------------------------------------------------------------------------------------------
def test_bookkeeping(room):
    import torch

    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu

    ex, n, st = room.ex, room.n, room.st
    CAP = r"cape_copy_pose_scores failed \(-4\)"

    def downloads():
        out = list(ex.map_matches_wide(n)) + list(ex.map_kalman_rows(n)) + list(ex.map_union_rows(n)) + list(ex.measurement_rows(n))
        (P, R, V), T = ex.download_map()
        return [np.ascontiguousarray(a).view(np.uint8).copy() for a in out + [P, R, V, T]]

    # the call writes nothing but its own results: match, Kalman, union, measurements, map and tracks are the bytes they were
    room.restore()
    ex.map_measure(n, room.T, room.S, st)
    ex.map_kalman(n, st)
    ex.map_union(n, st)
    before = downloads()
    ex.map_pose_score(n, room.poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    first = ex.pose_scores(n, residuals=True)
    ex.map_pose_score(n, room.poses, cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    second = ex.pose_scores(n, residuals=True)
    after = downloads()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and len(before) == 15
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)) and int(first[0]["n_pairs"].sum()) > 0
    # the argument checks behind the handle
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_score failed \(-1\)"):
        ex.map_pose_score(n, room.poses, 1 << 5, stream=st)
    assert ex.L.cape_map_pose_score(ex.h, n, 0, room.poses.ctypes.data_as(C.c_void_p), 0, C.c_void_p(st)) == -1
    assert ex.L.cape_map_pose_score(ex.h, n, 1, None, 0, C.c_void_p(st)) == -1
    assert ex.L.cape_map_pose_score(ex.h, -1, 1, room.poses.ctypes.data_as(C.c_void_p), 0, C.c_void_p(st)) == -1
    # the per-pair table beyond 1 GiB is refused before anything is allocated: 8 frames x 18 725 hypotheses x 128 x 7 x 8 bytes
    assert ex.L.cape_map_pose_score(ex.h, n, 18725, room.poses.ctypes.data_as(C.c_void_p), cape_amd.POSE_SCORE_RESIDUALS, C.c_void_p(st)) == -4
    # (a refused call leaves no results)
    with pytest.raises(cape_amd.CapeError, match=CAP):
        ex.pose_scores(1)
    # more frames than the wide match covered
    ex.match_map_wide(4, room.W2C[:4], None, room.flags, st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_score failed \(-4\)"):
        ex.map_pose_score(5, room.poses[:5], 0, stream=st)
    room.restore()

    # ---- what invalidates cape_map_kalman's results invalidates these: on a second handle, whose depth is at hand
    dev = torch.cat([synth_gpu.stream("room", 11, 1, start=20 + 5 * i, device="cuda", chunk=1) for i in range(4)]).contiguous()
    ex2 = Extractor(640, 480, cylinders=False, max_batch=4, **synth.DEFAULT_INTRINSICS)
    poses = room.poses[:4]

    def prepare(extract=True):
        if extract:
            ex2.extract_device(dev.data_ptr(), 4, st)
            ex2.build_polygons(4, st)
        ex2.upload_map(room.arrays)
        ex2.upload_tracks(room.tracks)
        ex2.match_map_wide(4, room.W2C[:4], None, room.flags, st)
        ex2.map_measure(4, room.T[:4], room.S[:4], st)
        ex2.map_pose_score(4, poses, 0, stream=st)
        return ex2.pose_scores(4)

    want = prepare()
    assert want.tobytes() == first[0][:4].tobytes(), "a second handle gives the first one's bytes"
    invalidators = {
        "cape_extract": lambda: ex2.extract_device(dev.data_ptr(), 4, st),
        "cape_build_polygons": lambda: ex2.build_polygons(4, st),
        "cape_map_upload": lambda: ex2.upload_map(room.arrays),
        "cape_map_upload_tracks": lambda: ex2.upload_tracks(room.tracks),
        "cape_match_map_wide": lambda: ex2.match_map_wide(4, room.W2C[:4], None, room.flags, st),
        "cape_map_measure": lambda: ex2.map_measure(4, room.T[:4], room.S[:4], st),
    }
    ps = C.c_void_p()
    for name, call in invalidators.items():
        assert ex2.pose_scores(4).tobytes() == want.tobytes()
        call()
        with pytest.raises(cape_amd.CapeError, match=CAP):
            ex2.pose_scores(1)
        assert ex2.L.cape_pose_score_device(ex2.h, C.byref(ps), None) == -4, name
        assert prepare().tobytes() == want.tobytes(), name
    # a step that changes the map
    result, _ = ex2.map_step(1, room.W2C[1], None, room.flags, cape_amd.COMMIT_ADD_STAGED, 900, st)
    assert result["commit"]["flags"] & cape_amd.COMMIT_DONE and (result["commit"]["n_updated"] > 0 or result["commit"]["n_appended"] > 0)
    with pytest.raises(cape_amd.CapeError, match=CAP):
        ex2.pose_scores(1)
    # ... and scoring needs a wide match against the map as it stands now
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_score failed \(-4\)"):
        ex2.map_pose_score(4, poses, 0, stream=st)
    ex2.match_map_wide(4, room.W2C[:4], None, room.flags, st)
    ex2.map_pose_score(4, poses, 0, stream=st)
    assert ex2.pose_scores(4).shape == (4, poses.shape[1])
    # without tracks, without a wide match
    ex2.upload_map(room.arrays)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_score failed \(-4\)"):
        ex2.map_pose_score(4, poses, 0, stream=st)  # no tracks
    ex2.upload_tracks(room.tracks)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_score failed \(-4\)"):
        ex2.map_pose_score(4, poses, 0, stream=st)  # tracks, but no wide match since the upload
    ex2.close()

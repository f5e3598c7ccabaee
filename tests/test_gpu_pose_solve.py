"""cape_map_pose_solve and cape_map_pose_select on the device against their host twins cape_host_pose_solve / cape_host_pose_select,
which compile the same rules header (csrc/cape_pose_solve.h).  The minimiser is + - x / sqrt in one order, no transcendental function:
solution rows, the pose buffer and the selection rows must equal the twin's BIT FOR BIT, on the device's own match.  The score rows in
the middle of the chain are cape_map_pose_score's and are held to what tests/test_gpu_pose_score.py holds them to.

Every test prints its figures before it asserts (`pytest -s`)."""
import ctypes as C
import math

import numpy as np
import pytest
from test_gpu_pose_score import _compare_with_twin, _det_planes, _hypotheses, _tracks_for
from test_pose_solve_host import pose_of

pytestmark = pytest.mark.gpu

W = 128
EYE = (np.eye(3), np.zeros(3))


def _x_of(w2c):
    """x[6] of a world-to-camera matrix under the identity camera basis: the position, then the coefficients (w, x, y) / (1 + z) of
    get_optimization_coefficients_from_quaternion"""
    R = w2c[:3, :3].T
    p = -(R @ w2c[:3, 3])
    w = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return np.concatenate([p, q[:3] / max(1.0 + q[3], 0.001)])


def _words(kept_planes):
    w = [0, 0, 0, 0]
    for i in kept_planes:
        w[int(i) >> 5] |= 1 << (int(i) & 31)
    return w


def _starts(rng, base, n_hyp, shift=40.0, turn=0.03):
    """(n, n_hyp, 6): per frame its own x perturbed by tens of mm and a few degrees (0.03 in a coefficient is about 3.4 degrees)"""
    out = np.empty((len(base), n_hyp, 6))
    for f, T in enumerate(base):
        x = _x_of(T)
        for h in range(n_hyp):
            out[f, h] = x + np.concatenate([rng.uniform(-shift, shift, 3), rng.uniform(-turn, turn, 3)])
    return out


def _subsets(rng, match, n_hyp, size):
    """(n, n_hyp, 4) words: per frame and hypothesis `size` of the frame's matched kept planes (all of them where it has fewer, or
    with size None)"""
    out = np.zeros((len(match), n_hyp, 4), np.uint32)
    for f, row in enumerate(match):
        paired = row[row >= 0]
        for h in range(n_hyp):
            pick = paired if size is None or len(paired) <= size else rng.choice(paired, size, replace=False)
            out[f, h] = _words(pick)
    return out


def _twin(ex, n, arrays, tracks, kept, x0=None, subsets=None, params=None, selection=None):
    """the twin's (solutions, poses) of every frame on the device's own match"""
    import cape_amd

    mframes, match, _, _ = ex.map_matches_wide(n)
    rows, poses = [], []
    for f in range(n):
        det = _det_planes(kept[f][0])
        flagged = int(mframes[f]["flags"]) & cape_amd.MATCH_EXACT_OVERFLOW
        m = match[f] if match.shape[1] else np.zeros(0, np.int32)
        r, p, _ = cape_amd.host_pose_solve(arrays, tracks, np.full(len(m), -1, np.int32) if flagged else m, det[:W] if flagged else det,
                                           None if x0 is None else x0[f], None if subsets is None else subsets[f], params=params,
                                           frame_flags=flagged, selection=None if selection is None else selection[f])
        rows.append(r)
        poses.append(p)
    return np.stack(rows), np.stack(poses)


def _solve_and_compare(ex, n, st, arrays, tracks, kept, x0, subsets, params=None):
    ex.map_pose_solve(n, x0, subsets, params=params, stream=st)
    rows, poses = ex.pose_solutions(n)
    want_rows, want_poses = _twin(ex, n, arrays, tracks, kept, x0, subsets, params)
    assert rows.shape == want_rows.shape == x0.shape[:2]
    for f in range(n):
        assert rows[f].tobytes() == want_rows[f].tobytes(), (f"frame {f}: solution rows; statuses {rows[f]['status'][:8].tolist()} != "
                                                             f"{want_rows[f]['status'][:8].tolist()}")
        assert poses[f].tobytes() == want_poses[f].tobytes(), f"frame {f}: poses"
    return rows, poses


def _summary(rows):
    s = rows["status"].reshape(-1)
    ran = rows["nfev"].reshape(-1)[s > 0]
    return (f"{len(s)} problems: statuses {dict(zip(*[v.tolist() for v in np.unique(s, return_counts=True)]))}, "
            f"nfev {int(ran.min()) if len(ran) else 0}..{int(ran.max()) if len(ran) else 0}")



class _Set:
    pass


@pytest.fixture(scope="module")
def rooms():
    """the eight room frames of the score test against a map of their own: every frame's kept planes lifted to the world (the room
    shows two or three planes per frame, so at most a frame or two reach the three pairs a problem needs; the others are refused)"""
    import cape_amd
    from test_gpu_map_kalman import _c2w
    from test_gpu_map_match import _kept, _map_from, _stream, _w2c
    from test_gpu_map_measure import _pose_covariances

    r = _Set()
    r.n = 8
    r.ex, r.st, r.c2w = _stream("room", 11, 20, 5, r.n)
    r.T = np.stack([_c2w(*r.c2w[f]) for f in range(r.n)])
    r.W2C = np.stack([_w2c(*r.c2w[f]) for f in range(r.n)])
    r.S = _pose_covariances(np.random.default_rng(21), r.n)
    r.flags = cape_amd.MATCH_ALLOW_INDEX0
    rng = np.random.default_rng(300)
    planes = _map_from(_kept(r.ex, r.n), r.c2w, range(r.n), rng, 0)
    r.arrays, r.tracks = cape_amd.pack_map(planes), _tracks_for(rng, len(planes))
    r.kept = r.ex.kept_planes(r.n)
    r.poses = _hypotheses(np.random.default_rng(51), r.W2C, 5)
    r.restore = lambda: _restore(r)
    r.restore()
    _, r.match, _, _ = r.ex.map_matches_wide(r.n)
    yield r
    r.ex.close()


def _restore(r):
    r.ex.upload_map(r.arrays)
    r.ex.upload_tracks(r.tracks)
    r.ex.match_map_wide(r.n, r.W2C, None, r.flags, r.st)


@pytest.fixture(scope="module")
def checker():
    """[room, checkerboard of 116 facets in four orientations, room] at 1280 x 960 against the checkerboard's own kept planes, last
    first: frame 1 has 65 .. 128 pairs, kept planes beyond 63 among them; the room frames have none"""
    import cape_amd
    from test_gpu_map_match import _lift
    from test_gpu_match_map_wide import _chained_input, _extract
    from test_gpu_match_wide import _small_pose

    frames, Wd, Ht, intr = _chained_input()
    c = _Set()
    c.ex, c.st = _extract(frames, Wd, Ht, intr)
    c.n = len(frames)
    c.kept = c.ex.kept_planes(c.n)
    det = c.kept[1][0]
    assert 64 < len(det) <= W
    rng = np.random.default_rng(360)
    c.arrays, c.tracks = cape_amd.pack_map([_lift(k, *EYE) for k in det][::-1]), _tracks_for(rng, len(det))
    c.W2C = _small_pose(c.n)
    c.flags = cape_amd.MATCH_ALLOW_INDEX0
    c.restore = lambda: _restore(c)
    c.restore()
    _, c.match, _, _ = c.ex.map_matches_wide(c.n)
    assert 65 <= int((c.match[1] >= 0).sum()) <= W
    yield c
    c.ex.close()


def _chain(s, n_hyp, seed):
    """solve -> score (the solve's poses in place) -> select -> refit, every stage against the twin; returns (rows, sel, refit, final)"""
    import cape_amd

    ex, n, st = s.ex, s.n, s.st
    rng = np.random.default_rng(seed)
    x0, subsets = _starts(rng, s.W2C, n_hyp), _subsets(rng, s.match, n_hyp, 3)
    rows, poses = _solve_and_compare(ex, n, st, s.arrays, s.tracks, s.kept, x0, subsets)
    print(f"\nsolve: {_summary(rows)}; pairs used {rows[:, 0]['n_pairs_used'].tolist()}")
    ran = rows["status"] > 0
    moved = np.abs(rows["x"][..., :3] - x0[..., :3]).max(axis=-1)
    assert ran.any() and moved[ran].max() > 1.0 and not moved[~ran].any(), "the minimiser moved, a refused problem did not"
    _, pose_ptr = ex.pose_solve_device()
    ex.map_pose_score(n, pose_ptr, cape_amd.POSE_SCORE_DEVICE_POSES, n_hypotheses=n_hyp, stream=st)
    scores, _, _, stats = _compare_with_twin(ex, n, s.arrays, s.tracks, s.kept, poses, residuals=False)
    print(f"score: {stats}")
    ex.map_pose_select(n, st)
    sel = ex.pose_selection(n)
    want = np.array([cape_amd.host_pose_select(scores[f], rows[f]) for f in range(n)])
    print(f"select: best {sel['best'].tolist()}, scanned {sel['n_scanned'].tolist()}, inliers {sel['n_inliers'].tolist()}, flags {sel['flags'].tolist()}")
    assert sel.tobytes() == want.tobytes() and (sel["best"] >= 0).any()
    ex.map_pose_solve(n, flags=cape_amd.POSE_SOLVE_FROM_SELECTION, stream=st)
    refit, refit_poses = ex.pose_solutions(n)
    want_rows, want_poses = _twin(ex, n, s.arrays, s.tracks, s.kept, selection=sel)
    print(f"refit: {_summary(refit)}; pairs used {refit[:, 0]['n_pairs_used'].tolist()}")
    assert refit.shape == (n, 1) and refit.tobytes() == want_rows.tobytes() and refit_poses.tobytes() == want_poses.tobytes()
    assert np.all((refit[:, 0]["status"] == cape_amd.POSE_SOLVE_NO_SELECTION) == (sel["best"] < 0))
    # (the selection is still there, and a select over the refit's single row is refused: the hypothesis counts differ)
    assert ex.pose_selection(n).tobytes() == sel.tobytes()
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_select failed \(-4\)"):
        ex.map_pose_select(n, st)
    _, pose_ptr = ex.pose_solve_device()
    ex.map_pose_score(n, pose_ptr, cape_amd.POSE_SCORE_DEVICE_POSES, n_hypotheses=1, stream=st)
    final = ex.pose_scores(n)[:, 0]
    print(f"final: inliers {final['n_inliers'].tolist()} of pairs {final['n_pairs'].tolist()}")
    # under its final pose at least one frame makes every pair an inlier
    assert any(refit[f, 0]["status"] > 0 and final[f]["n_inliers"] == final[f]["n_pairs"] >= 3 for f in range(n))
    return rows, sel, refit, final


def test_the_chain_on_the_room_frames(rooms):
    _chain(rooms, 24, 301)


def test_the_chain_on_the_chained_frame(checker):
    rows, sel, refit, final = _chain(checker, 24, 302)
    assert refit[1, 0]["n_pairs_used"] == sel[1]["n_inliers"] >= 3 and refit[1, 0]["status"] in (1, 2, 3)


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 256, 257])
def test_hypothesis_counts_at_the_lane_wave_and_workgroup_edges(checker, n_hyp):
    c = checker
    rng = np.random.default_rng(310 + n_hyp)
    x0, subsets = _starts(rng, c.W2C[:2], n_hyp), _subsets(rng, c.match[:2], n_hyp, 3)
    rows, _ = _solve_and_compare(c.ex, 2, c.st, c.arrays, c.tracks, c.kept, x0, subsets)
    print(f"\n{n_hyp} hypotheses per frame: {_summary(rows[1])}")
    assert (rows[1]["status"] > 0).all() and (rows[1]["n_pairs_used"] == 3).all()


def test_a_problem_alone_gives_the_bytes_it_gives_among_256_others(checker):
    c = checker
    rng = np.random.default_rng(320)
    x0, subsets = _starts(rng, c.W2C[:2], 257), _subsets(rng, c.match[:2], 257, 3)
    c.ex.map_pose_solve(2, x0, subsets, stream=c.st)
    rows, poses = c.ex.pose_solutions(2)
    assert len({r.tobytes() for r in rows[1]}) > 128, "the problems give different rows"
    for h in (0, 63, 64, 255, 256):
        c.ex.map_pose_solve(2, x0[:, h: h + 1], subsets[:, h: h + 1], stream=c.st)
        alone, alone_poses = c.ex.pose_solutions(2)
        assert alone[1, 0].tobytes() == rows[1, h].tobytes(), f"problem {h}: the row depends on its company"
        assert alone_poses[1, 0].tobytes() == poses[1, h].tobytes(), f"problem {h}: the pose depends on its company"


def test_subset_sizes_and_bits_of_unmatched_kept_planes(checker, rooms):
    c = checker
    rng = np.random.default_rng(330)
    x0 = _starts(rng, c.W2C, 7, shift=30.0, turn=0.01)
    subsets = np.concatenate([_subsets(rng, c.match, 2, 3), _subsets(rng, c.match, 2, 4), _subsets(rng, c.match, 1, 39),
                              _subsets(rng, c.match, 2, None)], axis=1)
    rows, _ = _solve_and_compare(c.ex, c.n, c.st, c.arrays, c.tracks, c.kept, x0, subsets)
    used = rows[1]["n_pairs_used"].tolist()
    print(f"\nchained frame, {len(c.kept[1][0])} kept planes: {_summary(rows[1])}; pairs used {used}")
    assert used[:5] == [3, 3, 4, 4, 39] and 65 <= used[5] == used[6] <= W and (rows[1]["status"] > 0).all()
    assert np.isin(rows[1, 4:]["status"], (1, 2, 3)).all(), "39 pairs and every pair of the frame: well conditioned"
    assert subsets[1, :, 2:].any(), "bits 64 .. 127 of the subset words are in use"
    # the room frames beside it have kept planes and no pair: every bit names an unmatched kept plane and is ignored
    assert all(len(c.kept[f][0]) > 0 for f in (0, 2)) and not rows[[0, 2]]["n_pairs_used"].any()
    # a subset that also names every unmatched kept plane solves the same problem: every pair of a room frame, and of the chained frame
    r = rooms
    x0r = _starts(rng, r.W2C, 2)
    exact, _ = _solve_and_compare(r.ex, r.n, r.st, r.arrays, r.tracks, r.kept, x0r, _subsets(rng, r.match, 2, None))
    r.ex.map_pose_solve(r.n, x0r, np.full((r.n, 2, 4), 0xFFFFFFFF, np.uint32), stream=r.st)
    everything, _ = r.ex.pose_solutions(r.n)
    print(f"room frames, every pair: {_summary(exact)}; pairs used {exact[:, 0]['n_pairs_used'].tolist()} of kept planes {[len(k[0]) for k in r.kept]}")
    assert everything.tobytes() == exact.tobytes()
    c.ex.map_pose_solve(c.n, x0[:, 5:], np.full((c.n, 2, 4), 0xFFFFFFFF, np.uint32), stream=c.st)
    assert c.ex.pose_solutions(c.n)[0].tobytes() == rows[:, 5:].tobytes()


def test_one_wave_mixes_refused_converged_and_maxfev_ended_lanes(checker):
    import cape_amd

    c = checker
    rng = np.random.default_rng(340)
    x0, subsets = _starts(rng, c.W2C[:2], 64, shift=60.0), _subsets(rng, c.match[:2], 64, 5)
    c.ex.map_pose_solve(2, x0, subsets, stream=c.st)
    done, _ = c.ex.pose_solutions(2)
    # lanes 3 k + 1 restart from where they ended: they end again at once; lanes 3 k + 2 are refused: no pairs, or a NaN in the start
    x0[:, 1::3] = done["x"][:, 1::3]
    subsets[:, 2::6] = 0
    x0[:, 5::6, 4] = np.nan
    params = cape_amd.pose_solve_params(maxfev=16)
    rows, poses = _solve_and_compare(c.ex, 2, c.st, c.arrays, c.tracks, c.kept, x0, subsets, params)
    status = rows[1]["status"]
    print(f"\none wave: {_summary(rows[1])}; by lane {status.tolist()}; nfev {rows[1]['nfev'].tolist()}")
    assert (status[2::6] == cape_amd.POSE_SOLVE_TOO_FEW_PAIRS).all() and (status[5::6] == cape_amd.POSE_SOLVE_BAD_START).all()
    assert np.isin(status[1::3], (1, 2, 3)).any() and (status[0::3] == 5).any()
    # the refused lanes' poses are the start's
    for h in range(2, 64, 6):
        assert np.array_equal(rows[1, h]["x"], x0[1, h]) and np.array_equal(poses[1, h], pose_of(x0[1, h]))
    assert np.isnan(poses[1, 5, :3, :3]).any()


def test_host_and_device_inputs_give_the_same_bytes(checker):
    import torch

    import cape_amd

    c = checker
    rng = np.random.default_rng(350)
    x0, subsets = _starts(rng, c.W2C, 9), _subsets(rng, c.match, 9, 3)
    c.ex.map_pose_solve(c.n, x0, subsets, stream=c.st)
    host_route = c.ex.pose_solutions(c.n)
    dx = torch.from_numpy(np.ascontiguousarray(x0)).cuda()
    ds = torch.from_numpy(np.ascontiguousarray(subsets).view(np.int32)).cuda()
    torch.cuda.current_stream().synchronize()
    c.ex.map_pose_solve(c.n, dx.data_ptr(), ds.data_ptr(), flags=cape_amd.POSE_SOLVE_DEVICE_INPUT, n_hypotheses=9, stream=c.st)
    rows, poses = c.ex.pose_solutions(c.n)
    assert rows.tobytes() == host_route[0].tobytes() and poses.tobytes() == host_route[1].tobytes() and (rows["status"] > 0).any()
    a, b = c.ex.pose_solve_device()
    assert a and b


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
    rng = np.random.default_rng(370)
    arrays, tracks = cape_amd.pack_map(planes), _tracks_for(rng, len(planes))
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    base = np.stack([np.eye(4)] * 3)
    base[2, :3, 3] = [50000.0, -50000.0, 50000.0]  # frame 2 sees the map from 50 m away: no pair passes the gates
    ex.match_map_wide(3, base, None, cape_amd.MATCH_ALLOW_INDEX0, st)
    fr, match, _, _ = ex.map_matches_wide(3)
    assert [int(v) for v in fr["flags"]] == [0, cape_amd.MATCH_EXACT_OVERFLOW, 0] and fr[0]["n_matched"] > 0 and fr[2]["n_matched"] == 0
    x0 = _starts(rng, base, 4)
    subsets = np.full((3, 4, 4), 0xFFFFFFFF, np.uint32)
    rows, _ = _solve_and_compare(ex, 3, st, arrays, tracks, kept, x0, subsets)
    print(f"\nflagged / no pairs: statuses {rows['status'].tolist()}, pairs used {rows[:, 0]['n_pairs_used'].tolist()}")
    assert (rows[1]["status"] == cape_amd.POSE_SOLVE_OVERFLOW).all() and (rows[1]["flags"] == cape_amd.MATCH_EXACT_OVERFLOW).all()
    assert (rows[2]["status"] == cape_amd.POSE_SOLVE_TOO_FEW_PAIRS).all() and not rows[1:]["n_pairs_used"].any()
    assert rows[0, 0]["n_pairs_used"] == fr[0]["n_matched"]
    # the selection over refused frames finds no consensus, and the refit says so
    ex.map_pose_score(3, ex.pose_solve_device()[1], cape_amd.POSE_SCORE_DEVICE_POSES, n_hypotheses=4, stream=st)
    ex.map_pose_select(3, st)
    sel = ex.pose_selection(3)
    assert list(sel[1:]["best"]) == [-1, -1] and (sel[1:]["flags"] == cape_amd.POSE_SELECT_NO_CONSENSUS).all()
    ex.map_pose_solve(3, flags=cape_amd.POSE_SOLVE_FROM_SELECTION, stream=st)
    refit, _ = ex.pose_solutions(3)
    want, _ = _twin(ex, 3, arrays, tracks, kept, selection=sel)
    assert refit.tobytes() == want.tobytes() and list(refit[1:, 0]["status"]) == [cape_amd.POSE_SOLVE_NO_SELECTION] * 2
    # an empty map succeeds: every problem is refused for its pairs
    empty, no_tracks = cape_amd.pack_map([]), np.zeros(0, cape_amd.MAP_TRACK_DTYPE)
    ex.upload_map(empty)
    ex.upload_tracks(no_tracks)
    ex.match_map_wide(3, base, None, 0, st)
    rows, _ = _solve_and_compare(ex, 3, st, empty, no_tracks, kept, x0, subsets)
    assert list(rows[:, 0]["status"]) == [cape_amd.POSE_SOLVE_TOO_FEW_PAIRS, cape_amd.POSE_SOLVE_OVERFLOW, cape_amd.POSE_SOLVE_TOO_FEW_PAIRS]
    ex.close()


def test_an_invalid_track_refuses_its_frame(checker):
    import cape_amd

    c = checker
    j = int(np.flatnonzero(c.match[1] >= 0)[3])
    bad = c.tracks.copy()
    bad[j]["covariance"][2, 2] = -1e-6  # (its square root is a NaN: is_valid fails)
    c.ex.upload_tracks(bad)
    c.ex.match_map_wide(c.n, c.W2C, None, c.flags, c.st)
    rng = np.random.default_rng(380)
    x0, subsets = _starts(rng, c.W2C, 3), _subsets(rng, c.match, 3, 3)
    rows, _ = _solve_and_compare(c.ex, c.n, c.st, c.arrays, bad, c.kept, x0, subsets)
    assert (rows[1]["status"] == cape_amd.POSE_SOLVE_INVALID_FEATURE).all() and (rows[1]["flags"] == cape_amd.POSE_SCORE_INVALID_FEATURE).all()
    assert (rows[[0, 2]]["status"] == cape_amd.POSE_SOLVE_TOO_FEW_PAIRS).all() and not rows[[0, 2]]["flags"].any()
    c.restore()


def test_bookkeeping(rooms):
    room = rooms
    import torch

    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu

    ex, n, st = room.ex, room.n, room.st
    CAP = r"cape_copy_pose_solutions failed \(-4\)"
    rng = np.random.default_rng(390)
    x0, subsets = _starts(rng, room.W2C, 5), _subsets(rng, room.match, 5, 3)

    def downloads():
        out = list(ex.map_matches_wide(n)) + list(ex.map_kalman_rows(n)) + list(ex.map_union_rows(n)) + list(ex.measurement_rows(n))
        out += list(ex.pose_scores(n, residuals=True)) + [ex.pose_features(n)]
        (P, R, V), T = ex.download_map()
        return [np.ascontiguousarray(a).view(np.uint8).copy() for a in out + [P, R, V, T]]

    # the calls write nothing but their own results: map, tracks, matches, Kalman, union, measurements and score results stay
    room.restore()
    ex.map_measure(n, room.T, room.S, st)
    ex.map_kalman(n, st)
    ex.map_union(n, st)
    ex.map_pose_score(n, room.poses[:, :5], cape_amd.POSE_SCORE_RESIDUALS, stream=st)
    before = downloads()
    ex.map_pose_solve(n, x0, subsets, stream=st)
    first = ex.pose_solutions(n)
    ex.map_pose_select(n, st)
    sel = ex.pose_selection(n)
    ex.map_pose_solve(n, flags=cape_amd.POSE_SOLVE_FROM_SELECTION, stream=st)
    ex.map_pose_solve(n, x0, subsets, stream=st)
    second = ex.pose_solutions(n)
    after = downloads()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and len(before) == 18
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)) and int(first[0]["n_pairs_used"].sum()) > 0
    # (a new solve over hypotheses ends the selection made over the rows it replaced)
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_pose_selection failed \(-4\)"):
        ex.pose_selection(1)
    # the argument checks behind the handle
    xp, sp = x0.ctypes.data_as(C.c_void_p), subsets.ctypes.data_as(C.c_void_p)
    assert ex.L.cape_map_pose_solve(ex.h, n, 5, xp, sp, None, 1 << 5, C.c_void_p(st)) == -1
    assert ex.L.cape_map_pose_solve(ex.h, n, 0, xp, sp, None, 0, C.c_void_p(st)) == -1
    assert ex.L.cape_map_pose_solve(ex.h, n, 5, None, sp, None, 0, C.c_void_p(st)) == -1
    assert ex.L.cape_map_pose_solve(ex.h, n, 5, xp, None, None, 0, C.c_void_p(st)) == -1
    assert ex.L.cape_map_pose_solve(ex.h, -1, 5, xp, sp, None, 0, C.c_void_p(st)) == -1
    assert ex.L.cape_map_pose_solve(ex.h, n, 2, None, None, None, cape_amd.POSE_SOLVE_FROM_SELECTION, C.c_void_p(st)) == -1
    bad = cape_amd.pose_solve_params(xtol=float("nan"))
    assert ex.L.cape_map_pose_solve(ex.h, n, 5, xp, sp, bad.ctypes.data_as(C.c_void_p), 0, C.c_void_p(st)) == -1
    # (an argument error leaves the last results alone; a refusal for capacity leaves none)
    assert ex.pose_solutions(n)[0].tobytes() == first[0].tobytes()
    # a refit without a current selection; select with a different hypothesis count, and without a current score or solve
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_solve failed \(-4\)"):
        ex.map_pose_solve(n, flags=cape_amd.POSE_SOLVE_FROM_SELECTION, stream=st)
    with pytest.raises(cape_amd.CapeError, match=CAP):
        ex.pose_solutions(1)
    ex.map_pose_solve(n, x0[:, :4], subsets[:, :4], stream=st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_select failed \(-4\)"):
        ex.map_pose_select(n, st)  # 4 solutions, 5 scores per frame
    ex.map_pose_solve(n, x0, subsets, stream=st)
    ex.map_pose_select(n, st)
    assert ex.pose_selection(n).tobytes() == sel.tobytes()
    ex.match_map_wide(n, room.W2C, None, room.flags, st)  # (ends the score and the solve)
    ex.map_pose_solve(n, x0, subsets, stream=st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_select failed \(-4\)"):
        ex.map_pose_select(n, st)  # no current score
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_pose_score(n, room.poses[:, :5], 0, stream=st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_select failed \(-4\)"):
        ex.map_pose_select(n, st)  # no current solve
    # more frames than the wide match covered
    ex.match_map_wide(4, room.W2C[:4], None, room.flags, st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_solve failed \(-4\)"):
        ex.map_pose_solve(5, x0[:5], subsets[:5], stream=st)
    ex.map_pose_solve(4, x0[:4], subsets[:4], stream=st)
    assert ex.pose_solutions(4)[0].tobytes() == first[0][:4].tobytes()
    with pytest.raises(cape_amd.CapeError, match=CAP):
        ex.pose_solutions(5)
    room.restore()

    # ---- what invalidates cape_map_pose_score's results invalidates these: on a second handle, whose depth is at hand
    dev = torch.cat([synth_gpu.stream("room", 11, 1, start=20 + 5 * i, device="cuda", chunk=1) for i in range(4)]).contiguous()
    ex2 = Extractor(640, 480, cylinders=False, max_batch=4, **synth.DEFAULT_INTRINSICS)

    def prepare(extract=True):
        if extract:
            ex2.extract_device(dev.data_ptr(), 4, st)
            ex2.build_polygons(4, st)
        ex2.upload_map(room.arrays)
        ex2.upload_tracks(room.tracks)
        ex2.match_map_wide(4, room.W2C[:4], None, room.flags, st)
        ex2.map_measure(4, room.T[:4], room.S[:4], st)
        ex2.map_pose_solve(4, x0[:4], subsets[:4], stream=st)
        ex2.map_pose_score(4, room.poses[:4, :5], 0, stream=st)
        ex2.map_pose_select(4, st)
        return ex2.pose_solutions(4)[0], ex2.pose_selection(4)

    want, want_sel = prepare()
    assert want.tobytes() == first[0][:4].tobytes() and want_sel.tobytes() == sel[:4].tobytes(), "a second handle gives the first one's bytes"
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
        assert ex2.pose_solutions(4)[0].tobytes() == want.tobytes()
        call()
        with pytest.raises(cape_amd.CapeError, match=CAP):
            ex2.pose_solutions(1)
        with pytest.raises(cape_amd.CapeError, match=r"cape_copy_pose_selection failed \(-4\)"):
            ex2.pose_selection(1)
        assert ex2.L.cape_pose_solve_device(ex2.h, C.byref(ps), None) == -4, name
        assert ex2.L.cape_map_pose_select(ex2.h, 4, C.c_void_p(st)) == -4, name
        got, got_sel = prepare()
        assert got.tobytes() == want.tobytes() and got_sel.tobytes() == want_sel.tobytes(), name
    # a step that changes the map
    result, _ = ex2.map_step(1, room.W2C[1], None, room.flags, cape_amd.COMMIT_ADD_STAGED, 900, st)
    assert result["commit"]["flags"] & cape_amd.COMMIT_DONE
    with pytest.raises(cape_amd.CapeError, match=CAP):
        ex2.pose_solutions(1)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_solve failed \(-4\)"):
        ex2.map_pose_solve(4, x0[:4], subsets[:4], stream=st)  # no wide match against the map as it stands now
    ex2.close()

"""cape_map_pose_solve and cape_map_pose_select on the device against their host twins cape_host_pose_solve / cape_host_pose_select,
which compile the same rules header (csrc/cape_pose_solve.h).  The minimiser is + - x / sqrt in one order, no transcendental function:
solution rows, the pose buffer and the selection rows must equal the twin's BIT FOR BIT, on the device's own match.  The score rows in
the middle of the chain are cape_map_pose_score's and are held to what tests/test_gpu_pose_score.py holds them to.  The same holds off
the default path: the parameter sets and camera bases of tests/test_pose_solve_host.py, a lane that takes the pivoted rank-deficient
branch among lanes that do not, and a lane whose first evaluation overflows.

Every test prints its figures before it asserts (`pytest -s`)."""
import ctypes as C
import math

import numpy as np
import pytest
from test_gpu_pose_score import _compare_with_twin, _det_planes, _hypotheses, _tracks_for
from test_pose_solve_host import BASES, CONVERGED, PARAMETER_SETS, STATUSES, pose_of

pytestmark = pytest.mark.gpu

W = 128
EYE = (np.eye(3), np.zeros(3))


def _x_of(w2c, C=np.eye(3)):
    """x[6] of a world-to-camera matrix under the camera basis C (world-to-camera rotation M^T with M = C R, position pw = C p): the
    position p, then the coefficients (w, x, y) / (1 + z) of get_optimization_coefficients_from_quaternion for R"""
    M = w2c[:3, :3].T
    R = C.T @ M
    p = C.T @ -(M @ w2c[:3, 3])
    w = math.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return np.concatenate([p, q[:3] / max(1.0 + q[3], 0.001)])


def _words(kept_planes):
    w = [0, 0, 0, 0]
    for i in kept_planes:
        w[int(i) >> 5] |= 1 << (int(i) & 31)
    return w


def _starts(rng, base, n_hyp, shift=40.0, turn=0.03, C=np.eye(3)):
    """(n, n_hyp, 6): per frame its own x under the basis C perturbed by tens of mm and a few degrees (0.03 in a coefficient is about
    3.4 degrees)"""
    out = np.empty((len(base), n_hyp, 6))
    for f, T in enumerate(base):
        x = _x_of(T, C)
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


# ---- off the default path: the camera basis and the parameter sets of tests/test_pose_solve_host.py -------------------------------
def _orientation_subsets(rng, det, match_row, sizes):
    """(len(sizes), 4) words: subsets of the frame's matched kept planes of the given sizes, each holding three planes whose normals
    are pairwise more than acos(0.9) apart (the checkerboard's four orientations: any three of them are independent), so that every
    problem has a minimum the stop codes of the table can be asserted at"""
    paired = match_row[match_row >= 0]
    normals = np.array([det[i][0] for i in paired])
    out = np.zeros((len(sizes), 4), np.uint32)
    for h, size in enumerate(sizes):
        order = rng.permutation(len(paired))
        apart = []
        for k in order:
            if len(apart) < 3 and all(abs(float(normals[k] @ normals[j])) < 0.9 for j in apart):
                apart.append(k)
        assert len(apart) == 3
        rest = [k for k in order if k not in apart][: max(0, min(size, len(paired)) - 3)]
        out[h] = _words(paired[apart + rest])
    return out


OFF_SIZES = (3,) * 6 + (5,) * 5 + (39,) * 5  # 16 problems per frame


def _noisy_map(det, seed=405):
    """The checkerboard's own kept planes as a map that a solver has something to do on: lifted by a camera pose that is not the
    identity (a turn of 0.05 about (1, 2, 3), 150 mm away), normals disturbed by 1e-3 and distances by 2 mm as make_frame of the
    host test disturbs them.  Returns (map planes, the world-to-camera matrix they were lifted by).
    (The fixture's own map is the exact lift under the identity pose: residuals that go to exactly 0 at x = 0, where gnorm, scaled
    by fnorm, never falls below gtol and xnorm makes xtol unreachable -- MINPACK's stop codes of the host table do not occur on it.)"""
    from test_gpu_map_match import _lift, _w2c

    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    R, o = np.eye(3) + math.sin(0.05) * K + (1.0 - math.cos(0.05)) * (K @ K), np.array([120.0, -80.0, 45.0])
    rng = np.random.default_rng(seed)
    planes = []
    for k in det:
        n, d, x, y, c, ring, holes = _lift(k, R, o)
        n = n + rng.normal(scale=1e-3, size=3)
        planes.append((n / np.linalg.norm(n), d + float(rng.normal(scale=2.0)), x, y, c, ring, holes))
    return planes, _w2c(R, o)


@pytest.mark.parametrize("name", list(PARAMETER_SETS))
def test_parameter_sets_under_three_camera_bases(checker, name):
    """one call per basis: the starts describe, under that basis, the pose the match was made under (perturbed), so the problems
    converge to the same camera; rows and poses are the twin's bytes, the statuses those the reference has on the host"""
    import cape_amd

    c = checker
    planes, w2c = _noisy_map(c.kept[1][0])
    arrays, W2C = cape_amd.pack_map(planes[::-1]), np.stack([w2c] * 2)
    try:
        c.ex.upload_map(arrays)
        c.ex.upload_tracks(c.tracks)
        c.ex.match_map_wide(2, W2C, None, c.flags, c.st)
        _, match, _, _ = c.ex.map_matches_wide(2)
        assert 65 <= int((match[1] >= 0).sum()) <= W
        rows_of = {}
        for basis, Cb in BASES.items():
            rng = np.random.default_rng(400)  # (the same subsets and the same perturbations under every basis)
            assert np.abs(pose_of(_x_of(w2c, Cb), Cb) - w2c).max() < 1e-9, "the start's coefficients describe the match's pose"
            x0 = _starts(rng, W2C, len(OFF_SIZES), C=Cb)
            subsets = np.stack([np.zeros((len(OFF_SIZES), 4), np.uint32), _orientation_subsets(rng, c.kept[1][0], match[1], OFF_SIZES)])
            params = cape_amd.pose_solve_params(camera_basis=Cb, **PARAMETER_SETS[name])
            rows, poses = _solve_and_compare(c.ex, 2, c.st, arrays, c.tracks, c.kept, x0, subsets, params)
            print(f"\n{name}, {basis}: {_summary(rows[1])}; flags {sorted(set(rows[1]['flags'].tolist()))}")
            assert rows[1]["n_pairs_used"].tolist() == list(OFF_SIZES) and not rows[1]["flags"].any()
            status = rows[1]["status"]
            if name == "ftol=xtol=0":
                assert np.isin(status, (6, 7, 8)).all() and (rows[1]["nfev"] < 400).all()
            else:
                assert np.isin(status, sorted(STATUSES[name])).all(), status.tolist()
            for h in range(len(OFF_SIZES)):
                assert np.array_equal(poses[1, h], pose_of(rows[1, h]["x"], Cb))
            rows_of[basis] = (rows, poses)
        # the basis is read: the same problems under another basis are other rows and other poses, bit for bit ...
        for basis in ("permutation", "rotated"):
            assert all(rows_of[basis][0][1, h].tobytes() != rows_of["identity"][0][1, h].tobytes() for h in range(len(OFF_SIZES)))
            assert all(rows_of[basis][1][1, h].tobytes() != rows_of["identity"][1][1, h].tobytes() for h in range(len(OFF_SIZES)))
        # ... of the same camera: where the iteration runs to its end the poses agree to what the tolerances leave
        if STATUSES.get(name) == CONVERGED or name == "ftol=xtol=0":
            apart = max(float(np.abs(rows_of[basis][1][1] - rows_of["identity"][1][1]).max()) for basis in ("permutation", "rotated"))
            print(f"{name}: poses under the three bases at most {apart:.3e} apart")
            assert apart < 1.0, "a millimetre: a transposed or mis-strided basis ends at another camera, metres away"
    finally:
        c.restore()


# ---- the rank-deficient branch and NOT_FINITE on the device -------------------------------------------------------------------
def _slabs_and_facets(width=640, height=480):
    """a depth frame of six planes: in the upper half three fronto-parallel slabs side by side, constant depths near 800, 1500 and
    2600 mm; in the lower half three tilted facets of the checkerboard's kind whose normals are independent.  With the noise of
    test_gpu_match_wide._perforated_wall."""
    from cape_amd import synth

    intr = synth.DEFAULT_INTRINSICS
    X, Y = np.meshgrid((np.arange(width) - intr["cx"]) / intr["fx"], (np.arange(height) - intr["cy"]) / intr["fy"])
    z = np.zeros((height, width))
    edges = [0, width // 3, 2 * width // 3, width]
    for k, (d, (nx, ny)) in enumerate(zip((800.0, 1500.0, 2600.0), ((0.5, 0.0), (-0.5, 0.0), (0.0, 0.5)))):
        cols = slice(edges[k], edges[k + 1])
        z[: height // 2, cols] = d
        z[height // 2:, cols] = (2000.0 + 240.0 * k) / (1.0 + nx * X[height // 2:, cols] + ny * Y[height // 2:, cols])
    return np.round(z + np.random.default_rng(5).normal(0, 0.6, (height, width))).astype(np.float32)


def _snap(v):
    """the signed unit vector of v's largest component"""
    out = np.zeros(3)
    k = int(np.argmax(np.abs(v)))
    out[k] = 1.0 if v[k] > 0 else -1.0
    return out


def _slab_pose():
    """camera to world (R, o): a turn of 0.004 about (1, 2, 3) and a few millimetres.  Not the identity: at a minimum whose position or
    whose last two coefficients are 0 the forward differences' steps sqrt(eps) |x_j| underflow against the residuals, the columns come
    out exactly 0 and a full-rank problem takes the pivoted branch in its last iterations (as it does in MINPACK's fdjac2):
    tests/test_pose_solve_host.py::test_the_slab_frame_of_the_device_test_on_the_host measures both on the twin."""
    a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(0.004) * K + (1.0 - math.cos(0.004)) * (K @ K), np.array([7.0, 5.0, 3.0])


def _slab_map(det, pose=None):
    """the map of a frame's own kept planes lifted by _slab_pose (or by `pose`), the fronto-parallel ones with normal and in-plane axes
    snapped to exact unit vectors and d = -(n . c), which leaves their detections tilted by about 0.003 against them: returns (map
    planes, the kept planes that are slabs)"""
    from test_gpu_map_match import _lift

    planes, slabs = [], []
    for i, k in enumerate(det):
        n, d, x, y, c, ring, holes = _lift(k, *(_slab_pose() if pose is None else pose))
        if abs(n[2]) > 0.999:
            n, x, y = _snap(n), _snap(x), _snap(y)
            d = float(-(n @ c))
            slabs.append(i)
        planes.append((n, d, x, y, c, ring, holes))
    return planes, slabs


DEGENERATE_START = np.array([10.0, -20.0, 0.0, 1.0, 0.0, 0.0])


@pytest.fixture(scope="module")
def slabs():
    """one 640 x 480 frame of three fronto-parallel slabs and three tilted facets against the map of its own kept planes, matched
    under the pose the map was lifted by.  A problem over the three slabs alone has map normals (0, 0, +-1) exactly: the columns of
    x and y are exactly 0 whatever the rotation, and from a start with the identity rotation the first coefficient's too -- the
    pivoted qrfac, the nsing < 6 arms of lmpar and qrsolv and a pivot vector that is not the identity; its minimum is not at the
    start's rotation.  The facets make the other problems of the same wave full rank.  (The slabs alone would not: with three
    parallel planes every start is rank deficient.)"""
    import cape_amd
    from cape_amd import synth
    from test_gpu_map_match import _w2c
    from test_gpu_match_map_wide import _extract

    s = _Set()
    s.n = 1
    s.ex, s.st = _extract(_slabs_and_facets()[None], 640, 480, synth.DEFAULT_INTRINSICS)
    s.kept = s.ex.kept_planes(1)
    det = s.kept[0][0]
    planes, s.slabs = _slab_map(det)
    assert len(det) == 6 and len(s.slabs) == 3
    s.facets = [i for i in range(6) if i not in s.slabs]
    s.arrays, s.tracks = cape_amd.pack_map(planes), _tracks_for(np.random.default_rng(410), len(planes))
    s.W2C = _w2c(*_slab_pose())[None]
    s.ex.upload_map(s.arrays)
    s.ex.upload_tracks(s.tracks)
    s.ex.match_map_wide(1, s.W2C, None, cape_amd.MATCH_ALLOW_INDEX0, s.st)
    _, s.match, _, _ = s.ex.map_matches_wide(1)
    assert sorted(s.match[0][:6].tolist()) == list(range(6)), "every plane finds itself"
    yield s
    s.ex.close()


def _slab_problems(s, rng, lane):
    """16 problems: the degenerate one over the three slabs in `lane`, around it the three facets with some of the slabs from starts
    turned by a few degrees"""
    x0 = _starts(rng, s.W2C, 16)
    x0[0, lane] = DEGENERATE_START
    subsets = np.array([[_words(s.facets + [i for i in s.slabs if rng.random() < 0.5]) for _ in range(16)]], np.uint32)
    subsets[0, lane] = _words(s.slabs)
    return x0, subsets


def test_a_rank_deficient_lane_among_full_rank_lanes(slabs):
    import cape_amd

    s, lane = slabs, 5
    x0, subsets = _slab_problems(s, np.random.default_rng(420), lane)
    rows, poses = _solve_and_compare(s.ex, 1, s.st, s.arrays, s.tracks, s.kept, x0, subsets)
    row = rows[0, lane]
    print(f"\nslabs: {_summary(rows[0])}; flags {rows[0]['flags'].tolist()}; the degenerate lane: status {row['status']}, nfev {row['nfev']}, "
          f"fnorm {row['fnorm0']:.4g} -> {row['fnorm']:.4g}, x {row['x'].tolist()}")
    others = np.arange(16) != lane
    assert row["flags"] == cape_amd.POSE_SOLVE_RANK_DEFICIENT and not rows[0, others]["flags"].any()
    assert row["status"] > 0 and row["n_pairs_used"] == 3 and np.array_equal(row["x"][:2], DEGENERATE_START[:2])
    assert np.isin(rows[0, others]["status"], (1, 2, 3)).all() and (rows[0, others]["n_pairs_used"] >= 3).all()
    # alone it gives the bytes it gives in company
    s.ex.map_pose_solve(1, x0[:, lane: lane + 1], subsets[:, lane: lane + 1], stream=s.st)
    alone, alone_poses = s.ex.pose_solutions(1)
    assert alone[0, 0].tobytes() == row.tobytes() and alone_poses[0, 0].tobytes() == poses[0, lane].tobytes()


def test_a_lane_that_overflows_among_converging_lanes(slabs):
    """x0[0] = 1e160: the residuals' squares overflow at the first evaluation -- CAPE_POSE_SOLVE_NOT_FINITE, arithmetic and no fault;
    the infinite fnorm0 compares as bytes"""
    import cape_amd

    s, lane = slabs, 9
    x0, subsets = _slab_problems(s, np.random.default_rng(430), 5)
    x0[0, lane, 0] = 1e160
    rows, poses = _solve_and_compare(s.ex, 1, s.st, s.arrays, s.tracks, s.kept, x0, subsets)
    row = rows[0, lane]
    print(f"\nslabs: {_summary(rows[0])}; the overflowing lane: status {row['status']}, nfev {row['nfev']}, fnorm0 {row['fnorm0']}")
    assert row["status"] == cape_amd.POSE_SOLVE_NOT_FINITE and row["nfev"] == 1 and row["iterations"] == 0
    assert np.array_equal(row["x"], x0[0, lane]) and np.isposinf(row["fnorm0"]) and np.array_equal(poses[0, lane], pose_of(x0[0, lane]))
    assert (rows[0, np.arange(16) != lane]["status"] > 0).all()


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

"""The pair rows cape_map_pose_score, cape_map_pose_solve and cape_map_pose_covariance share (cape_handle_s::PosePairs): the pairs kernel
runs only where the rows do not cover the call's frames for the current batch, map, tracks and match, so a row that outlives one of
its inputs would be a stale cache.  The invalidator loops of the other pose tests upload identical data again and cannot see one; here
every case changes an input the pairs kernel reads, runs ONE stage first and compares its bytes with a fresh handle that saw only the
final inputs.  No tolerance anywhere: the fresh path is what the other tests pin to the host twins.

A four-frame 640 x 480 handle (max_batch = 4) on room frames 20, 25, 30, 35 and the room map of tests/test_gpu_pose_solve.py.  Those
frames show at most two pairs, so their solves and covariances are refused rows -- whose bytes still carry n_pairs, n_invalid and the
flags of the rows read; the last test runs the whole chain on frames 40 .. 55, where problems are solved.  Every test prints its figures
before it asserts (`pytest -s`)."""
import ctypes as C

import numpy as np
import pytest
from test_gpu_pose_score import _det_planes, _hypotheses
from test_gpu_pose_solve import _starts, _subsets, rooms  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N = 4
STAGES = ("score", "solve", "covariance")
ITERATIONS = 16


class _Inputs:
    """what a handle is prepared from: the depth frames, the map, its tracks, the poses of the match and its skip words"""

    def __init__(self, depth, arrays, tracks, w2c, skip=None):
        self.depth, self.arrays, self.tracks, self.w2c, self.skip = depth, arrays, tracks, w2c, skip


def _extract(ex, st, depth):
    ex.extract_device(depth.data_ptr(), N, st)
    ex.build_polygons(N, st)


def _upload_and_match(ex, st, i, flags):
    ex.upload_map(i.arrays)
    ex.upload_tracks(i.tracks)
    ex.match_map_wide(N, i.w2c, i.skip, flags, st)


@pytest.fixture(scope="module")
def base(rooms):  # noqa: F811
    import torch

    from cape_amd import Extractor, synth, synth_gpu

    b = type("Base", (), {})()
    b.room, b.st, b.flags = rooms, rooms.st, rooms.flags
    frames = lambda first: torch.cat([synth_gpu.stream("room", 11, 1, start=first + 5 * i, device="cuda", chunk=1) for i in range(N)]).contiguous()
    b.depth, b.other_depth = frames(20), frames(40)  # the room's frames 0 .. 3 and 4 .. 7
    b.inputs = _Inputs(b.depth, rooms.arrays, rooms.tracks, rooms.W2C[:N])
    b.new = lambda: Extractor(640, 480, cylinders=False, max_batch=N, **synth.DEFAULT_INTRINSICS)
    b.ex = b.new()
    _extract(b.ex, b.st, b.depth)
    _upload_and_match(b.ex, b.st, b.inputs, b.flags)
    _, b.match, _, _ = b.ex.map_matches_wide(N)
    rng = np.random.default_rng(700)
    b.poses = _hypotheses(rng, rooms.W2C[:N], 5)
    b.x0, b.subsets = _starts(rng, rooms.W2C[:N], 5), np.full((N, 5, 4), 0xFFFFFFFF, np.uint32)  # (every pair: bits of unmatched planes are ignored)
    b.table = rng.normal(size=(ITERATIONS, 128, 4)) * 1e-3
    b.ex.map_pose_score(N, b.poses, 0, stream=b.st)
    b.scores, b.features = b.ex.pose_scores(N), b.ex.pose_features(N)
    print(f"\nthe original inputs: pairs per frame {b.scores[:, 0]['n_pairs'].tolist()}, invalid {b.scores[:, 0]['n_invalid'].tolist()}")
    assert b.scores[:, 0]["n_pairs"].max() >= 2 and not b.scores["n_invalid"].any()
    # the first frame with a pair and the map plane of its first pair, for the cases that change one
    b.frame = int(np.flatnonzero(b.scores[:, 0]["n_pairs"] >= 2)[0])
    b.plane = int(b.features[b.frame, 0]["map_index"])
    yield b
    b.ex.close()


def _original(b):
    """the shared handle on the original inputs, its rows filled by a score"""
    _extract(b.ex, b.st, b.depth)
    _upload_and_match(b.ex, b.st, b.inputs, b.flags)
    b.ex.map_pose_score(N, b.poses, 0, stream=b.st)
    assert b.ex.pose_features(N).tobytes() == b.features.tobytes()


def _fresh(b, inputs):
    ex = b.new()
    _extract(ex, b.st, inputs.depth)
    _upload_and_match(ex, b.st, inputs, b.flags)
    return ex


def _run(b, ex, stage, n=N):
    """one stage over the first n frames and everything it leaves, as arrays"""
    import cape_amd as ca

    if stage == "score":
        ex.map_pose_score(n, b.poses[:n], 0, stream=b.st)
        return [ex.pose_scores(n), ex.pose_features(n)]
    if stage == "solve":
        ex.map_pose_solve(n, b.x0[:n], b.subsets[:n], stream=b.st)
        return list(ex.pose_solutions(n))
    ex.map_pose_covariance(n, ITERATIONS, b.x0[:n, 0], b.subsets[:n, 0], deviates=b.table, flags=ca.POSE_COVARIANCE_TABLE | ca.POSE_COVARIANCE_KEEP_SAMPLES,
                           stream=b.st)
    return [ex.pose_covariance(n), ex.pose_covariance_samples(n)]


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: result {k} differs from the fresh handle's"


def _first_stage_against_fresh(b, stage, inputs, what):
    """the changed handle's first pose call against a fresh handle's; then both handles' feature rows"""
    fresh = _fresh(b, inputs)
    try:
        got, want = _run(b, b.ex, stage), _run(b, fresh, stage)
        _same(got, want, f"{what}, {stage} first")
        features, fresh_features = _run(b, b.ex, "score")[1], _run(b, fresh, "score")[1]
        assert features.tobytes() == fresh_features.tobytes(), what
        return got, features, fresh
    except BaseException:
        fresh.close()
        raise


@pytest.mark.parametrize("stage", STAGES)
def test_new_tracks_end_the_rows(base, stage):
    import cape_amd as ca

    b = base
    _original(b)
    tracks = b.inputs.tracks.copy()
    tracks[b.plane]["covariance"][0, 0] = np.nan
    b.ex.upload_tracks(tracks)
    got, features, fresh = _first_stage_against_fresh(b, stage, _Inputs(b.depth, b.inputs.arrays, tracks, b.inputs.w2c), "a NaN in a matched plane's covariance")
    fresh.close()
    print(f"\n{stage} first: {[(a.dtype.names or ('poses',))[0] for a in got]} equal the fresh handle's")
    if stage == "score":
        assert (got[0][b.frame]["n_invalid"] == 1).all() and (got[0][b.frame]["flags"] & ca.POSE_SCORE_INVALID_FEATURE).all()
    elif stage == "solve":
        assert (got[0][b.frame]["status"] == ca.POSE_SOLVE_INVALID_FEATURE).all(), "every problem of the frame is refused"
    else:
        assert got[0][b.frame]["status"] == ca.POSE_SOLVE_INVALID_FEATURE and got[0][b.frame]["n_ok"] == 0
    assert np.isnan(features[b.frame, 0]["stddev"][0])


@pytest.mark.parametrize("stage", STAGES)
def test_a_new_map_ends_the_rows(base, stage):
    b = base
    _original(b)
    P, R, V = (a.copy() for a in b.inputs.arrays)
    P["d"][b.plane] += 5.0
    moved = _Inputs(b.depth, (P, R, V), b.inputs.tracks, b.inputs.w2c)
    _upload_and_match(b.ex, b.st, moved, b.flags)
    got, features, fresh = _first_stage_against_fresh(b, stage, moved, "a map plane moved by 5 mm")
    fresh.close()
    rows = features[b.frame]
    k = int(np.flatnonzero((rows["map_index"] == b.plane) & (rows["map_id"] != 0))[0])
    print(f"\n{stage} first: feature row {k} of frame {b.frame} holds d = {rows[k]['map_plane'][3]!r}, the map {P['d'][b.plane]!r}")
    assert rows[k]["map_plane"][3] == P["d"][b.plane] != b.inputs.arrays[0]["d"][b.plane]


@pytest.mark.parametrize("stage", STAGES)
def test_a_new_match_ends_the_rows(base, stage):
    b = base
    _original(b)
    # the words drop the plane in every frame; in b.frame also every plane the frame left unmatched (the map holds the same wall as
    # lifted from other frames: the kept plane would pair with one of those instead, and n_pairs would stay)
    skip = np.zeros((N, (len(b.inputs.arrays[0]) + 31) // 32), np.uint32)
    skip[:, b.plane >> 5] = 1 << (b.plane & 31)
    for j in np.flatnonzero(b.match[b.frame] < 0):
        skip[b.frame, j >> 5] |= np.uint32(1 << (int(j) & 31))
    skipped = _Inputs(b.depth, b.inputs.arrays, b.inputs.tracks, b.inputs.w2c, skip)
    b.ex.match_map_wide(N, skipped.w2c, skip, b.flags, b.st)
    got, features, fresh = _first_stage_against_fresh(b, stage, skipped, "a matched map plane skipped")
    scores = fresh.pose_scores(N)
    fresh.close()
    before, after = b.features[b.frame], features[b.frame]
    n_before, n_after = int(b.scores[b.frame, 0]["n_pairs"]), int(scores[b.frame, 0]["n_pairs"])
    print(f"\n{stage} first: frame {b.frame} had pairs with map planes {before['map_index'][:n_before].tolist()}, has {after['map_index'][:n_after].tolist()}")
    assert n_after == n_before - 1
    assert after["map_index"][:n_after].tolist() == [j for j in before["map_index"][:n_before].tolist() if j != b.plane], "the rows close up"
    assert not after[n_after:].tobytes().strip(b"\0"), "zeros at and beyond n_pairs"


@pytest.mark.parametrize("stage", STAGES)
def test_a_new_batch_ends_the_rows(base, stage):
    b = base
    _original(b)
    other = _Inputs(b.other_depth, b.inputs.arrays, b.inputs.tracks, b.room.W2C[N: 2 * N])
    _extract(b.ex, b.st, other.depth)
    b.ex.match_map_wide(N, other.w2c, None, b.flags, b.st)
    got, features, fresh = _first_stage_against_fresh(b, stage, other, "four other frames")
    kept = fresh.kept_planes(N)
    fresh.close()
    assert features.tobytes() != b.features.tobytes()
    pairs = [int((features[f]["map_id"] != 0).sum()) for f in range(N)]
    print(f"\n{stage} first: pairs per frame {pairs} on the new batch")
    assert max(pairs) >= 2
    for f in range(N):
        det = _det_planes(kept[f][0])
        assert all(np.array_equal(r["matched"], det[r["kept_plane"]]) for r in features[f][: pairs[f]]), f"frame {f}: the matched planes are the new frame's"


def test_a_step_that_changes_the_map_ends_the_rows(base):
    import cape_amd as ca

    b, r = base, base.room
    ex, st = b.ex, b.st
    staged_tracks = b.inputs.tracks.copy()
    staged_tracks["flags"][b.plane] = ca.MAP_TRACK_STAGED  # (the plane of b.frame's first pair)
    _extract(ex, st, b.depth)
    _upload_and_match(ex, st, _Inputs(b.depth, b.inputs.arrays, staged_tracks, b.inputs.w2c), b.flags)
    ex.map_measure(N, r.T[:N], r.S[:N], st)
    ex.map_pose_score(N, b.poses, 0, stream=st)  # (fills the rows)
    result, _ = ex.map_step(b.frame, r.W2C[b.frame], None, b.flags, 0, 9000, st)
    arrays, tracks = ex.download_map()
    changed = arrays[0][b.plane].tobytes() != b.inputs.arrays[0][b.plane].tobytes()
    print(f"\nstep of frame {b.frame}: commit {int(result['commit']['flags']):#x}, {int(result['commit']['n_updated'])} updated, staged plane {b.plane} "
          f"changed: {changed}, d {b.inputs.arrays[0]['d'][b.plane]!r} -> {arrays[0]['d'][b.plane]!r}")
    assert result["commit"]["flags"] == ca.COMMIT_DONE and result["commit"]["n_updated"] >= 1 and changed
    ex.match_map_wide(N, b.inputs.w2c, None, b.flags, st)
    fresh = _fresh(b, _Inputs(b.depth, arrays, tracks, b.inputs.w2c))
    try:
        assert fresh.map_matches_wide(N)[1].tobytes() == ex.map_matches_wide(N)[1].tobytes(), "the committed map, uploaded again, matches alike"
        _same(_run(b, ex, "solve"), _run(b, fresh, "solve"), "a committed step, solve first")
        # (these frames' problems are refused: the rows the solve read, which a score behind it finds current, say what it saw of the map)
        features = _run(b, ex, "score")[1]
        assert features.tobytes() == _run(b, fresh, "score")[1].tobytes(), "the rows behind the solve are the committed map's"
        k = int(np.flatnonzero((features[b.frame]["map_index"] == b.plane) & (features[b.frame]["map_id"] != 0))[0])
        assert features[b.frame, k]["map_plane"][3] == arrays[0]["d"][b.plane]
    finally:
        fresh.close()
        ex.clear_retired()


def test_coverage_grows_and_never_shrinks(base):
    b = base
    fresh = _fresh(b, b.inputs)
    try:
        want = _run(b, fresh, "solve")
        # the rows of all four frames filled from the OTHER batch first: what a rebuild over more frames that was skipped would leave in
        # frames 2 and 3
        _extract(b.ex, b.st, b.other_depth)
        _upload_and_match(b.ex, b.st, _Inputs(b.other_depth, b.inputs.arrays, b.inputs.tracks, b.room.W2C[N: 2 * N]), b.flags)
        other = _run(b, b.ex, "score")[1]
        assert other[2:].tobytes() != b.features[2:].tobytes()
        _extract(b.ex, b.st, b.depth)
        _upload_and_match(b.ex, b.st, b.inputs, b.flags)
        two = _run(b, b.ex, "score", 2)
        _same(_run(b, b.ex, "solve"), want, "a score of 2 frames, then a solve of 4")
        assert b.ex.pose_features(2).tobytes() == two[1].tobytes() == b.features[:2].tobytes(), "the score's features, behind a solve over more frames"
        # (the problems of these frames are refused and say little of the rows: a score of 4 frames finds the solve's rows current and shows them)
        assert _run(b, b.ex, "score")[1].tobytes() == b.features.tobytes(), "the solve over 4 frames built the rows of frames 2 and 3"
        # the other way round: rows of 4 frames stay those of 4 frames behind a solve of 2
        _same(_run(b, b.ex, "solve", 2), [a[:2] for a in want], "a score of 4 frames, then a solve of 2")
        assert b.ex.pose_features(N).tobytes() == b.features.tobytes()
    finally:
        fresh.close()


def test_the_features_address_outlives_later_stages(base):
    b = base
    _original(b)
    b.ex.match_map_wide(N, b.inputs.w2c, None, b.flags, b.st)
    _run(b, b.ex, "score", 2)

    def address():
        scores, features = C.c_void_p(), C.c_void_p()
        assert b.ex.L.cape_pose_score_device(b.ex.h, C.byref(scores), C.byref(features)) == 0
        return features.value

    first = address()
    _run(b, b.ex, "solve")  # (over 4 frames: more than the score covered)
    second = address()
    _run(b, b.ex, "covariance")
    print(f"\nfeatures at {first:#x}, {second:#x} behind a solve, {address():#x} behind a covariance")
    assert first and first == second == address()
    assert b.ex.pose_features(2).tobytes() == b.features[:2].tobytes()


def test_rows_found_current_and_rows_rebuilt_give_the_same_chain(base):
    """score -> solve (119 three-pair subsets) -> select -> refit -> covariance (64 iterations, a table) twice: on a handle whose every
    stage behind the score finds the rows current, and with cape_map_upload_tracks of the same tracks in front of every stage that reads
    the rows, so that each rebuilds them.  An upload ends every pose result with the rows, so the second chain hands each stage what the
    first one reads on the device: the selection is the host twin's over the copied rows (tests/test_gpu_pose_solve.py pins the device's
    to it), the refit and the covariance take its x and words as arguments.  Scores, solutions and selection are compared over all frames;
    the refit only where a frame has a selection (without one the first chain reports NO_SELECTION, the second a start of zeros refused
    for its pairs), the covariance only where that refit succeeded (the first chain carries a failed refit's status, the second refuses
    on its own grounds): the printed line names those frames."""
    import cape_amd as ca

    b = base
    ex, st = b.ex, b.st
    rng = np.random.default_rng(710)
    H, iterations = 119, 64
    # (the room's frames 4 .. 7: a problem needs three pairs, which none of the frames 0 .. 3 has)
    w2c = b.room.W2C[N: 2 * N]
    _extract(ex, st, b.other_depth)
    _upload_and_match(ex, st, _Inputs(b.other_depth, b.inputs.arrays, b.inputs.tracks, w2c), b.flags)
    match = ex.map_matches_wide(N)[1]
    poses, x0, subsets = _hypotheses(rng, w2c, H), _starts(rng, w2c, H), _subsets(rng, match, H, 3)
    table = rng.normal(size=(iterations, 128, 4)) * 1e-3
    flags = ca.POSE_COVARIANCE_TABLE | ca.POSE_COVARIANCE_KEEP_SAMPLES
    ex.map_pose_score(N, poses, 0, stream=st)
    ex.map_pose_solve(N, x0, subsets, stream=st)
    solutions = ex.pose_solutions(N)[0]  # (read here: the refit below replaces the solve's rows; a copy replaces no input)
    ex.map_pose_select(N, st)
    ex.map_pose_solve(N, flags=ca.POSE_SOLVE_FROM_SELECTION, stream=st)
    ex.map_pose_covariance(N, iterations, deviates=table, flags=flags | ca.POSE_COVARIANCE_FROM_SOLUTION, stream=st)
    scores, selection = ex.pose_scores(N), ex.pose_selection(N)
    refit, rows, samples = ex.pose_solutions(N)[0], ex.pose_covariance(N), ex.pose_covariance_samples(N)

    def rebuild():
        ex.upload_tracks(b.inputs.tracks)

    rebuild()
    ex.map_pose_score(N, poses, 0, stream=st)
    scores2 = ex.pose_scores(N)
    rebuild()
    ex.map_pose_solve(N, x0, subsets, stream=st)
    solutions2 = ex.pose_solutions(N)[0]
    selection2 = np.array([ca.host_pose_select(scores2[f], solutions2[f]) for f in range(N)])
    rebuild()
    ex.map_pose_solve(N, selection2["x"][:, None], selection2["inlier_words"][:, None], stream=st)
    refit2 = ex.pose_solutions(N)[0]
    rebuild()
    ex.map_pose_covariance(N, iterations, refit2[:, 0]["x"], selection2["inlier_words"], deviates=table, flags=flags, stream=st)
    rows2, samples2 = ex.pose_covariance(N), ex.pose_covariance_samples(N)
    chosen = np.flatnonzero(selection["best"] >= 0)
    print(f"\nchain: refit compared on frames {chosen.tolist()}, pairs {scores[:, 0]['n_pairs'].tolist()}, best {selection['best'].tolist()}, refit statuses {refit[:, 0]['status'].tolist()}, covariance statuses {rows['status'].tolist()}, "
          f"n_ok {rows['n_ok'].tolist()}")
    assert scores2.tobytes() == scores.tobytes() and solutions2.tobytes() == solutions.tobytes() and selection2.tobytes() == selection.tobytes()
    assert refit2[chosen].tobytes() == refit[chosen].tobytes()
    ran = chosen[refit[chosen, 0]["status"] > 0]  # (a failed refit is refused as the refit's by the first chain, as a start's by the second)
    assert len(ran) >= 1 and (rows[ran]["n_ok"] > 0).all()
    assert rows2[ran].tobytes() == rows[ran].tobytes() and samples2[ran].tobytes() == samples[ran].tobytes()

"""cape_map_pose_covariance and cape_pose_draw_deviates on the device against their host twins cape_host_pose_covariance /
cape_host_pose_draw_deviates, which compile the same rules header (csrc/cape_pose_covariance.h).

With a table of deviates (POSE_COVARIANCE_TABLE) nothing transcendental stands in front of a sample's x: every kept sample row, n_ok,
the statuses, the nfev figures, the position part of the mean and the position block of the covariance must equal the twin's BIT FOR
BIT.  The three Euler angles of a pose vector go through atan2, sin and cos -- ocml's on the device, glibc's on the host --, so the
angle part of the mean and the 27 covariance entries that involve an angle are compared with the figures measured on the MI355X
(MEAN_ANGLES_MEASURED, COVARIANCE_ANGLES_MEASURED below), asserted at twice that.  Philox deviates go through log, cos and sin and are
compared with NORMALS_MEASURED; the generator mode itself is held device against device, through cape_pose_draw_deviates.

The frames: the chained batch [room, checkerboard, room] at 1280 x 960 against the noisy lifted map of the checkerboard's kept planes
(the room frames have no pair: their rows carry the refusal), and the slab frame of six planes at 640 x 480.  The two cannot share a
batch: a handle has one resolution.  Iteration counts 1, 2, 3, 63, 64, 65, 100, 256, 257 cross a wave and a workgroup.

Every test prints its figures before it asserts (`pytest -s`)."""
import ctypes as C

import numpy as np
import pytest
from test_gpu_pose_score import _det_planes
from test_gpu_pose_solve import W, _noisy_map, _starts, _subsets, checker, slabs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ITERATIONS = (1, 2, 3, 63, 64, 65, 100, 256, 257)
# the largest differences between the device and the twin over test_table_mode_against_the_twin's frames and iteration counts (measured
# on the MI355X with this file; printed by the test before it asserts): the angle part of the mean, absolute (radians); the covariance
# entries that involve an angle, relative to the frame's largest entry
MEAN_ANGLES_MEASURED = 2.8e-17
COVARIANCE_ANGLES_MEASURED = 1.1e-17
# the largest difference between the device's and the twin's normal deviates over a table of 100 x 128 x 4 (measured on the MI355X)
NORMALS_MEASURED = 4.5e-16


def _small_tracks(n, seed=600):
    """tracks whose standard deviations leave the samples near the optimum: 1e-4 .. 1e-3 in a normal's component, 0.1 .. 2 mm in d"""
    import cape_amd

    rng = np.random.default_rng(seed)
    tracks = np.zeros(n, cape_amd.MAP_TRACK_DTYPE)
    for j in range(n):
        tracks[j]["covariance"] = np.diag(np.concatenate([rng.uniform(1e-4, 1e-3, 3), rng.uniform(0.1, 2.0, 1)]) ** 2)
        tracks[j]["id"] = 700 + 3 * j
    return tracks


class _Set:
    pass


@pytest.fixture(scope="module")
def chained(checker):  # noqa: F811
    """the chained batch against the noisy lifted map with small standard deviations, matched under the lifting pose; x: per frame the
    optimum over all its pairs (the device's own solve), subsets: all its pairs"""
    import cape_amd

    c = checker
    s = _Set()
    s.ex, s.st, s.n, s.kept = c.ex, c.st, c.n, c.kept
    planes, w2c = _noisy_map(c.kept[1][0])
    s.arrays, s.tracks, s.W2C = cape_amd.pack_map(planes[::-1]), _small_tracks(len(planes)), np.stack([w2c] * c.n)
    s.flags = c.flags

    def restore():
        s.ex.upload_map(s.arrays)
        s.ex.upload_tracks(s.tracks)
        s.ex.match_map_wide(s.n, s.W2C, None, s.flags, s.st)

    s.restore = restore
    restore()
    _, s.match, _, _ = s.ex.map_matches_wide(s.n)
    assert 65 <= int((s.match[1] >= 0).sum()) <= W and (s.match[[0, 2]] >= 0).sum(axis=1).max() < 3, "the room frames stay below three pairs"
    rng = np.random.default_rng(601)
    s.subsets = _subsets(rng, s.match, 1, None)[:, 0]
    s.ex.map_pose_solve(s.n, _starts(rng, s.W2C, 1, shift=5.0, turn=0.002), s.subsets[:, None], stream=s.st)
    rows, _ = s.ex.pose_solutions(s.n)
    assert rows[1, 0]["status"] in (1, 2, 3)
    s.x = rows[:, 0]["x"].copy()
    yield s
    c.restore()


@pytest.fixture(scope="module")
def slab(slabs):  # noqa: F811
    """the slab frame with small standard deviations; x: the optimum over its six pairs"""
    b = slabs
    s = _Set()
    s.ex, s.st, s.n, s.kept, s.arrays, s.W2C = b.ex, b.st, 1, b.kept, b.arrays, b.W2C
    s.tracks = _small_tracks(6, 602)
    import cape_amd

    s.flags = cape_amd.MATCH_ALLOW_INDEX0

    def restore():
        s.ex.upload_map(s.arrays)
        s.ex.upload_tracks(s.tracks)
        s.ex.match_map_wide(1, s.W2C, None, s.flags, s.st)

    s.restore = restore
    restore()
    _, s.match, _, _ = s.ex.map_matches_wide(1)
    rng = np.random.default_rng(603)
    s.subsets = _subsets(rng, s.match, 1, None)[:, 0]
    s.ex.map_pose_solve(1, _starts(rng, s.W2C, 1, shift=5.0, turn=0.002), s.subsets[:, None], stream=s.st)
    rows, _ = s.ex.pose_solutions(1)
    assert rows[0, 0]["status"] > 0 and rows[0, 0]["n_pairs_used"] == 6
    s.x = rows[:, 0]["x"].copy()
    yield s
    b.ex.upload_map(b.arrays)
    b.ex.upload_tracks(b.tracks)
    b.ex.match_map_wide(1, b.W2C, None, s.flags, b.st)


def _twin(s, n_iterations, x=None, subsets=None, deviates=None, seed=0, frame_base=0, params=None, solutions=None, selection=None):
    """the twin's (rows, samples, vectors) of every frame on the device's own match"""
    import cape_amd

    mframes, match, _, _ = s.ex.map_matches_wide(s.n)
    rows, samples, vectors = [], [], []
    for f in range(s.n):
        det = _det_planes(s.kept[f][0])
        flagged = int(mframes[f]["flags"]) & cape_amd.MATCH_EXACT_OVERFLOW
        m = match[f] if match.shape[1] else np.zeros(0, np.int32)
        r, sm, v = cape_amd.host_pose_covariance(s.arrays, s.tracks, np.full(len(m), -1, np.int32) if flagged else m, det[:W] if flagged else det,
                                                 n_iterations, None if x is None else x[f], None if subsets is None else subsets[f], deviates=deviates,
                                                 seed=seed, frame_index=frame_base + f, params=params, frame_flags=flagged,
                                                 solution=None if solutions is None else solutions[f], selection=None if selection is None else selection[f])
        rows.append(r)
        samples.append(sm)
        vectors.append(v)
    return np.array(rows), np.stack(samples), np.stack(vectors)


def _ldlt_pivots(M):
    """the diagonal of an LDL^T of the symmetric M with diagonal pivoting (numpy, for the guard of the status comparison)"""
    A, d = np.array(M, float), []
    for k in range(len(A)):
        p = k + int(np.argmax(np.abs(np.diag(A)[k:])))
        A[[k, p]] = A[[p, k]]
        A[:, [k, p]] = A[:, [p, k]]
        d.append(A[k, k])
        if A[k, k] != 0.0:
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:]) / A[k, k]
    return np.array(d)


def _exact_parts_equal(rows, want):
    for name in ("n_ok", "n_iterations", "status", "flags", "nfev_min", "nfev_max", "nfev_sum"):
        assert np.array_equal(rows[name], want[name]), (name, rows[name].tolist(), want[name].tolist())
    assert rows["mean"][:, :3].tobytes() == want["mean"][:, :3].tobytes(), "the position part of the mean"
    assert np.ascontiguousarray(rows["covariance"][:, :3, :3]).tobytes() == np.ascontiguousarray(want["covariance"][:, :3, :3]).tobytes(), "the position block"


def _angle_differences(rows, want):
    """(mean angles: the largest absolute difference in radians; covariance entries that involve an angle: the largest difference
    relative to the frame's largest entry -- the slab frame's angle entries are a thousand times the chained frame's) over the rows where
    both are finite"""
    mask = np.ones((6, 6), bool)
    mask[:3, :3] = False
    d_mean = d_cov = 0.0
    for r, w in zip(rows, want):
        if np.isfinite(w["covariance"]).all():
            d_mean = max(d_mean, float(np.abs(r["mean"][3:] - w["mean"][3:]).max()))
            d_cov = max(d_cov, float(np.abs(r["covariance"][mask] - w["covariance"][mask]).max() / np.abs(w["covariance"]).max()) if w["covariance"].any() else 0.0)
        else:  # (n_ok = 1: 0 / 0 in every entry, on both sides)
            assert np.isnan(r["covariance"]).all() and np.isnan(w["covariance"]).all()
    return d_mean, d_cov


@pytest.mark.parametrize("n_iterations", ITERATIONS)
def test_table_mode_against_the_twin(chained, slab, n_iterations):
    import cape_amd

    flags = cape_amd.POSE_COVARIANCE_TABLE | cape_amd.POSE_COVARIANCE_KEEP_SAMPLES
    table = np.random.default_rng(610 + n_iterations).normal(size=(n_iterations, W, 4))
    if n_iterations >= 63:
        table[5::7, :, 3] = 1e200  # a seventh of the samples overflow and fail; 1, 2 and 3 iterations run clean
    worst_mean = worst_cov = 0.0
    for name, s in (("chained", chained), ("slab", slab)):
        # the twin first, and from its values alone whether a status could hang on rounding
        want, want_samples, _ = _twin(s, n_iterations, s.x, s.subsets, deviates=table)
        near = [bool(np.isfinite(w["covariance"]).all() and w["n_ok"] > 1 and
                     np.abs(_ldlt_pivots(w["covariance"])).min() <= 1e-12 * np.abs(w["covariance"]).max()) for w in want]
        assert sum(near) == 0, "no frame of these sets has a pivot within 1e-12 relative of zero"
        s.ex.map_pose_covariance(s.n, n_iterations, s.x, s.subsets, deviates=table, flags=flags, stream=s.st)
        rows, samples = s.ex.pose_covariance(s.n), s.ex.pose_covariance_samples(s.n)
        assert samples.shape == want_samples.shape == (s.n, n_iterations)
        for f in range(s.n):
            assert samples[f].tobytes() == want_samples[f].tobytes(), (f"{name}, frame {f}: sample rows; statuses {samples[f]['status'][:8].tolist()} != "
                                                                       f"{want_samples[f]['status'][:8].tolist()}")
        _exact_parts_equal(rows, want)
        d_mean, d_cov = _angle_differences(rows, want)
        worst_mean, worst_cov = max(worst_mean, d_mean), max(worst_cov, d_cov)
        print(f"\n{name}, {n_iterations} iterations: statuses {rows['status'].tolist()}, n_ok {rows['n_ok'].tolist()}, nfev {rows['nfev_min'].tolist()}.."
              f"{rows['nfev_max'].tolist()}; angle parts: mean {d_mean:.3e}, covariance {d_cov:.3e} from the twin")
    print(f"{n_iterations} iterations: mean angles at most {worst_mean:.3e}, covariance entries with an angle at most {worst_cov:.3e} from the twin")
    assert worst_mean <= 2 * MEAN_ANGLES_MEASURED and worst_cov <= 2 * COVARIANCE_ANGLES_MEASURED
    # what the frames are there for
    rows = chained.ex.pose_covariance(chained.n)
    assert (rows["status"][[0, 2]] == cape_amd.POSE_SOLVE_TOO_FEW_PAIRS).all() and not rows["n_ok"][[0, 2]].any() and not rows["covariance"][[0, 2]].any()
    expected = cape_amd.POSE_COVARIANCE_INVALID if n_iterations == 1 else cape_amd.POSE_COVARIANCE_VALID
    assert rows["status"][1] == expected and slab.ex.pose_covariance(1)["status"][0] == expected
    if n_iterations >= 63:
        assert rows["n_ok"][1] == n_iterations - len(range(5, n_iterations, 7))


def test_the_chain_without_a_host_wait(chained):
    """match -> solve -> score -> select -> refit -> covariance enqueued on one stream, nothing copied in between, against the same
    stages with every result copied to the host in between; the room frames carry the refit's refusal"""
    import cape_amd

    s = chained
    ex, n, st = s.ex, s.n, s.st
    rng = np.random.default_rng(620)
    n_hyp = 24
    x0, subsets = _starts(rng, s.W2C, n_hyp), _subsets(rng, s.match, n_hyp, 3)

    def chain(copies):
        out = []
        ex.match_map_wide(n, s.W2C, None, s.flags, st)
        if copies:
            out.append(ex.map_matches_wide(n)[1])
        ex.map_pose_solve(n, x0, subsets, stream=st)
        if copies:
            out.append(ex.pose_solutions(n))
        ex.map_pose_score(n, ex.pose_solve_device()[1], cape_amd.POSE_SCORE_DEVICE_POSES, n_hypotheses=n_hyp, stream=st)
        if copies:
            out.append(ex.pose_scores(n))
        ex.map_pose_select(n, st)
        if copies:
            out.append(ex.pose_selection(n))
        ex.map_pose_solve(n, flags=cape_amd.POSE_SOLVE_FROM_SELECTION, stream=st)
        if copies:
            out.append(ex.pose_solutions(n))
        ex.map_pose_covariance(n, 100, seed=2026, frame_base=40, flags=cape_amd.POSE_COVARIANCE_FROM_SOLUTION | cape_amd.POSE_COVARIANCE_KEEP_SAMPLES,
                               stream=st)
        return ex.pose_covariance(n), ex.pose_covariance_samples(n), out

    rows, samples, _ = chain(False)
    stepwise, stepwise_samples, copied = chain(True)
    sel, refit = copied[3], copied[4][0]
    print(f"\nchain: refit statuses {refit[:, 0]['status'].tolist()}, covariance statuses {rows['status'].tolist()}, n_ok {rows['n_ok'].tolist()}, "
          f"nfev {rows['nfev_min'].tolist()}..{rows['nfev_max'].tolist()}, position variances {np.diag(rows[1]['covariance'])[:3].tolist()}")
    assert rows.tobytes() == stepwise.tobytes() and samples.tobytes() == stepwise_samples.tobytes()
    assert refit[1, 0]["status"] in (1, 2, 3) and rows[1]["status"] == cape_amd.POSE_COVARIANCE_VALID and rows[1]["n_ok"] == 100
    assert (rows["status"][[0, 2]] == cape_amd.POSE_SOLVE_NO_SELECTION).all() and not rows["n_ok"][[0, 2]].any() and not samples[[0, 2]]["nfev"].any()
    # the refit's x and the selection's words given by hand are the same samples, and the twin's from the same rows
    ex.map_pose_covariance(n, 100, refit[:, 0]["x"], sel["inlier_words"], seed=2026, frame_base=40, flags=cape_amd.POSE_COVARIANCE_KEEP_SAMPLES, stream=st)
    assert ex.pose_covariance_samples(n)[1].tobytes() == samples[1].tobytes() and ex.pose_covariance(n)[1].tobytes() == rows[1].tobytes()
    table = ex.pose_draw_deviates(2026, 41, 100)
    want, want_samples, _ = _twin(s, 100, deviates=table, solutions=refit[:, 0], selection=sel)
    assert want_samples[1].tobytes() == samples[1].tobytes() and list(want["status"]) == list(rows["status"])
    # the position block is what cape_map_measure takes
    assert np.array_equal(rows[1]["covariance"][:3, :3], rows[1]["covariance"][:3, :3].T) and (np.linalg.eigvalsh(rows[1]["covariance"][:3, :3]) > 0).all()


def test_generator_mode(chained, slab):
    import cape_amd

    s = slab
    # the words: seed 0, frame 0, iteration 0, slot 0, block 0 is the first known answer, read through the uniforms
    u = s.ex.pose_draw_deviates(0, 0, 1, uniforms=True)[0, 0]
    assert u[0] == (((0x6627E8D5 << 32 | 0xE169C58D) >> 11) + 1) * 2.0 ** -53 and u[1] == (((0xBC57AC4C << 32 | 0x9B00DBD8) >> 11) + 1) * 2.0 ** -53
    seed, base = 0xFEDCBA9876543210, 5
    assert s.ex.pose_draw_deviates(seed, base, 100, uniforms=True).tobytes() == cape_amd.host_pose_draw_deviates(seed, base, 100, uniforms=True).tobytes()
    table = s.ex.pose_draw_deviates(seed, base, 100)
    d = float(np.abs(table - cape_amd.host_pose_draw_deviates(seed, base, 100)).max())
    print(f"\nnormals, device against twin over {table.size} deviates: at most {d:.3e} apart")
    assert d <= 2 * NORMALS_MEASURED
    # device against device through one function: a generator-mode call and a table call fed with what cape_pose_draw_deviates wrote
    keep = cape_amd.POSE_COVARIANCE_KEEP_SAMPLES
    for t, frame in ((slab, 0), (chained, 1)):
        t.ex.map_pose_covariance(t.n, 100, t.x, t.subsets, seed=seed, frame_base=base, flags=keep, stream=t.st)
        rows, samples = t.ex.pose_covariance(t.n), t.ex.pose_covariance_samples(t.n)
        drawn = t.ex.pose_draw_deviates(seed, base + frame, 100)
        t.ex.map_pose_covariance(t.n, 100, t.x, t.subsets, deviates=drawn, flags=keep | cape_amd.POSE_COVARIANCE_TABLE, stream=t.st)
        assert t.ex.pose_covariance(t.n)[frame].tobytes() == rows[frame].tobytes() and rows[frame]["status"] == cape_amd.POSE_COVARIANCE_VALID
        assert t.ex.pose_covariance_samples(t.n)[frame].tobytes() == samples[frame].tobytes()
        # the same seed again: the same bytes; another seed or another frame_base: other samples
        t.ex.map_pose_covariance(t.n, 100, t.x, t.subsets, seed=seed, frame_base=base, flags=keep, stream=t.st)
        assert t.ex.pose_covariance(t.n).tobytes() == rows.tobytes() and t.ex.pose_covariance_samples(t.n).tobytes() == samples.tobytes()
        for other in (dict(seed=seed + 1, frame_base=base), dict(seed=seed, frame_base=base + 1)):
            t.ex.map_pose_covariance(t.n, 100, t.x, t.subsets, flags=keep, stream=t.st, **other)
            assert t.ex.pose_covariance_samples(t.n)[frame].tobytes() != samples[frame].tobytes()
    # frame_base + frame is one index: frame 1 under base 5 is frame index 6
    assert chained.ex.pose_draw_deviates(seed, 6, 3).tobytes() == slab.ex.pose_draw_deviates(seed, 6, 3).tobytes()


def test_a_sample_alone_gives_the_bytes_it_gives_among_256_others(chained):
    import cape_amd

    s = chained
    flags = cape_amd.POSE_COVARIANCE_TABLE | cape_amd.POSE_COVARIANCE_KEEP_SAMPLES
    table = np.random.default_rng(630).normal(size=(257, W, 4))
    s.ex.map_pose_covariance(s.n, 257, s.x, s.subsets, deviates=table, flags=flags, stream=s.st)
    samples = s.ex.pose_covariance_samples(s.n)
    assert len({r.tobytes() for r in samples[1]}) == 257, "the samples give different rows"
    for i in (0, 63, 64, 255, 256):
        s.ex.map_pose_covariance(s.n, 1, s.x, s.subsets, deviates=table[i: i + 1], flags=flags, stream=s.st)
        assert s.ex.pose_covariance_samples(s.n)[1, 0].tobytes() == samples[1, i].tobytes(), f"sample {i}: the row depends on its company"


def test_chunks_of_frames_give_the_unchunked_rows(chained):
    import cape_amd

    s = chained
    keep = cape_amd.POSE_COVARIANCE_KEEP_SAMPLES
    # (chunking is about where a frame's planes lie in the slab: the chained frame is the first, the second or the only frame of its chunk)
    s.ex.map_pose_covariance(s.n, 65, s.x, s.subsets, seed=9, flags=keep, stream=s.st)
    rows, samples = s.ex.pose_covariance(s.n), s.ex.pose_covariance_samples(s.n)
    try:
        s.ex.set_pose_covariance_budget(4096 * 65)  # one frame's planes: three frames take three chunks
        s.ex.map_pose_covariance(s.n, 65, s.x, s.subsets, seed=9, flags=keep, stream=s.st)
        assert s.ex.pose_covariance(s.n).tobytes() == rows.tobytes() and s.ex.pose_covariance_samples(s.n).tobytes() == samples.tobytes()
        s.ex.set_pose_covariance_budget(4096 * 65 * 2)  # two chunks: frames 0 and 1, then frame 2
        s.ex.map_pose_covariance(s.n, 65, s.x, s.subsets, seed=9, flags=keep, stream=s.st)
        assert s.ex.pose_covariance(s.n).tobytes() == rows.tobytes() and s.ex.pose_covariance_samples(s.n).tobytes() == samples.tobytes()
        s.ex.set_pose_covariance_budget(4096 * 65 - 1)  # not one frame
        with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_covariance failed \(-4\)"):
            s.ex.map_pose_covariance(s.n, 65, s.x, s.subsets, seed=9, stream=s.st)
    finally:
        s.ex.set_pose_covariance_budget(0)
    assert rows[1]["status"] == cape_amd.POSE_COVARIANCE_VALID and rows[1]["n_ok"] == 65


def test_device_inputs_give_the_same_bytes(chained):
    import torch

    import cape_amd

    s = chained
    flags = cape_amd.POSE_COVARIANCE_TABLE | cape_amd.POSE_COVARIANCE_KEEP_SAMPLES
    table = np.random.default_rng(640).normal(size=(64, W, 4))
    s.ex.map_pose_covariance(s.n, 64, s.x, s.subsets, deviates=table, flags=flags, stream=s.st)
    rows, samples = s.ex.pose_covariance(s.n), s.ex.pose_covariance_samples(s.n)
    dx = torch.from_numpy(np.ascontiguousarray(s.x)).cuda()
    ds = torch.from_numpy(np.ascontiguousarray(s.subsets).view(np.int32)).cuda()
    dz = torch.from_numpy(np.ascontiguousarray(table)).cuda()
    torch.cuda.current_stream().synchronize()
    s.ex.map_pose_covariance(s.n, 64, dx.data_ptr(), ds.data_ptr(), deviates=dz.data_ptr(), flags=flags | cape_amd.POSE_COVARIANCE_DEVICE_INPUT, stream=s.st)
    assert s.ex.pose_covariance(s.n).tobytes() == rows.tobytes() and s.ex.pose_covariance_samples(s.n).tobytes() == samples.tobytes()
    assert s.ex.pose_covariance_device()
    # a table drawn into device memory is the table drawn into host memory
    s.ex.pose_draw_deviates(77, 3, 64, out=dz.data_ptr())
    assert dz.cpu().numpy().tobytes() == s.ex.pose_draw_deviates(77, 3, 64).tobytes()


def test_bookkeeping(chained):
    import cape_amd

    s = chained
    ex, n, st = s.ex, s.n, s.st
    CAP = r"cape_copy_pose_covariance failed \(-4\)"
    rng = np.random.default_rng(650)
    x0, subsets = _starts(rng, s.W2C, 4), _subsets(rng, s.match, 4, 3)
    s.restore()
    ex.map_pose_solve(n, x0, subsets, stream=st)
    ex.map_pose_score(n, ex.pose_solve_device()[1], cape_amd.POSE_SCORE_DEVICE_POSES, n_hypotheses=4, stream=st)
    before = [a.tobytes() for a in (*ex.pose_solutions(n), ex.pose_scores(n), ex.pose_features(n), ex.map_matches_wide(n)[1])]
    ex.map_pose_covariance(n, 10, s.x, s.subsets, seed=1, stream=st)
    first = ex.pose_covariance(n)
    after = [a.tobytes() for a in (*ex.pose_solutions(n), ex.pose_scores(n), ex.pose_features(n), ex.map_matches_wide(n)[1])]
    assert before == after, "the solve's, the score's and the match's results are unchanged by a covariance call"
    # the samples were not kept
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_pose_covariance_samples failed \(-1\)"):
        ex.pose_covariance_samples(n)
    # the argument checks behind the handle
    xp, sp = s.x.ctypes.data_as(C.c_void_p), s.subsets.ctypes.data_as(C.c_void_p)
    call = ex.L.cape_map_pose_covariance
    assert call(ex.h, n, 0, xp, sp, None, 0, 0, None, 0, C.c_void_p(st)) == -1
    assert call(ex.h, n, 10, xp, sp, None, 0, 0, None, 1 << 4, C.c_void_p(st)) == -1
    assert call(ex.h, n, 10, xp, sp, None, 0, 0, None, cape_amd.POSE_COVARIANCE_TABLE, C.c_void_p(st)) == -1
    assert call(ex.h, n, 10, None, sp, None, 0, 0, None, 0, C.c_void_p(st)) == -1
    assert call(ex.h, n, 10, xp, None, None, 0, 0, None, 0, C.c_void_p(st)) == -1
    assert call(ex.h, -1, 10, xp, sp, None, 0, 0, None, 0, C.c_void_p(st)) == -1
    bad = cape_amd.pose_solve_params(xtol=float("nan"))
    assert call(ex.h, n, 10, xp, sp, None, 0, 0, bad.ctypes.data_as(C.c_void_p), 0, C.c_void_p(st)) == -1
    # (an argument error leaves the last results alone; a refusal for capacity leaves none)
    assert ex.pose_covariance(n).tobytes() == first.tobytes()
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_covariance failed \(-4\)"):
        ex.map_pose_covariance(n, 10, flags=cape_amd.POSE_COVARIANCE_FROM_SOLUTION, stream=st)  # the current solve is no refit
    with pytest.raises(cape_amd.CapeError, match=CAP):
        ex.pose_covariance(1)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_covariance failed \(-4\)"):
        ex.map_pose_covariance(n, (1 << 22) // n + 1, s.x, s.subsets, flags=cape_amd.POSE_COVARIANCE_KEEP_SAMPLES, stream=st)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_pose_covariance failed \(-4\)"):
        ex.map_pose_covariance(n + 1, 10, np.zeros((n + 1, 6)), np.zeros((n + 1, 4), np.uint32), stream=st)  # more frames than the match covered
    # each call that ends the solve's results ends these
    T, S = np.linalg.inv(s.W2C), np.stack([0.01 * np.eye(3)] * n)
    invalidators = {
        "cape_map_upload": lambda: ex.upload_map(s.arrays),
        "cape_map_upload_tracks": lambda: ex.upload_tracks(s.tracks),
        "cape_match_map_wide": lambda: ex.match_map_wide(n, s.W2C, None, s.flags, st),
        "cape_map_measure": lambda: ex.map_measure(n, T, S, st),
    }
    address = C.c_void_p()
    for name, invalidate in invalidators.items():
        s.restore()
        ex.map_pose_solve(n, x0, subsets, stream=st)
        ex.map_pose_covariance(n, 10, s.x, s.subsets, seed=1, stream=st)
        assert ex.pose_covariance(n).tobytes() == first.tobytes(), name
        invalidate()
        with pytest.raises(cape_amd.CapeError, match=CAP):
            ex.pose_covariance(1)
        with pytest.raises(cape_amd.CapeError, match=r"cape_copy_pose_solutions failed \(-4\)"):
            ex.pose_solutions(1)
        assert ex.L.cape_pose_covariance_device(ex.h, C.byref(address)) == -4, name
    s.restore()

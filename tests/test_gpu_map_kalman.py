"""cape_map_kalman: the state half of the map update on the device -- per frame and per map plane the Kalman step on the match of
cape_match_map_wide and the rows of cape_map_measure, the triple normalisation, the frame of the polygon step, the counters and the
promote / drop / lost decisions -- against its host twin cape_host_map_kalman, fed with the device's own measurement rows, bit for bit
(there is no pow on this path), and against the whole host update cape_host_map_update within a bound measured on the CPU.

Every test prints its figures before it asserts (`pytest -s`)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 128  # cape_amd.MATCH_MAP_WIDE_MAX_PLANES

# Test 5's bound.  The device's R differs from the host's by ocml's pow against the C library's: tests/test_gpu_map_measure.py grants
# the covariances 1e-12 relative.  profiles/map_kalman_bound.py feeds cape_host_kalman_update the host's own R of these eight room
# frames' matched pairs perturbed by 1e-12 relative (200 random symmetric directions per pair) and takes the largest relative change
# of x' and P' (profiles/r12_map_kalman_bound.txt); the bound is 4 x that, to cover another perturbation direction.  Under every one
# of those perturbations the host's result bits and counters stayed the same.
PERTURBATION_EFFECT = 5.074e-13  # largest relative change measured on the CPU: of P' (that of the new plane is 7.155e-15)
KALMAN_BOUND = 4 * PERTURBATION_EFFECT


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _bits_nan(a):
    """bit patterns with every NaN as one pattern: which NaN an invalid operation generates is the hardware's choice (x86 sets the sign
    bit of its default NaN, gfx950 does not), not the algebra's; everything that is not a NaN is compared bit for bit"""
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return b


def _c2w(R, o):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, o
    return T


def _tracks(meas):
    """the tracks of a map made of measurements: each covariance as a staged plane would hold it; local and staged planes in turn,
    with counters one short of each threshold (promote at 4 successive matches, drop at 2 failures, lost at 10)"""
    import cape_amd

    tracks = np.zeros(len(meas), cape_amd.MAP_TRACK_DTYPE)
    kinds = ((cape_amd.MAP_TRACK_STAGED, 3, 0), (0, 5, 9), (cape_amd.MAP_TRACK_STAGED, 0, 1), (0, 2, 0))
    for j, m in enumerate(meas):
        tracks[j]["covariance"] = m["covariance"]
        tracks[j]["flags"], tracks[j]["successive_matched"], tracks[j]["failed_tracking"] = kinds[j % len(kinds)]
        tracks[j]["id"] = 100 + j
    return tracks


def _compare_with_twin(ex, n, arrays, tracks):
    """every frame of the last map_kalman against cape_host_map_kalman on the device's own match and measurement rows, byte for byte;
    returns (frames, rows, track results, the wide match, the measurements)"""
    import cape_amd

    frames, rows, results = ex.map_kalman_rows(n)
    mframes, match, _, map_of = ex.map_matches_wide(n)
    meas = ex.map_measurements(n)
    assert results.shape == (n, len(arrays[0]))
    for f in range(n):
        n_cur = len(meas[f])
        assert mframes[f]["flags"] == 0 and mframes[f]["n_cur"] == n_cur <= W, f"frame {f} is flagged"
        frame, trows, tres = cape_amd.host_map_kalman(arrays, tracks, match[f], meas[f])
        assert frames[f].tobytes() == frame.tobytes(), f"frame {f}: header {frames[f]} != {frame}"
        for i in range(n_cur):
            assert rows[f, i].tobytes() == trows[i].tobytes(), f"frame {f}, kept plane {i}: {rows[f, i]} != {trows[i]}"
        assert not rows[f, n_cur:].view(np.uint8).any(), f"frame {f}: rows beyond n_cur"
        assert results[f].tobytes() == tres.tobytes(), f"frame {f}: track results {results[f]} != {tres}"
        assert np.array_equal(rows[f, :n_cur]["map_plane"], map_of[f, :n_cur])
    return frames, rows, results, (mframes, match, map_of), meas


# ---- 1. the algebra through debug_eval ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(host_binaries):
    import cape_amd

    return cape_amd._host_library()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_kalman_step_equals_the_host_twin_on_bit_patterns(host):
    import cape_amd
    from test_map_update_host import _spd, _unit

    rng = np.random.default_rng(17)
    cases = []
    for k in range(3000):
        x = np.append(_unit(rng), rng.uniform(-4000, 4000))
        z = x + np.append(rng.normal(scale=0.01, size=3), rng.normal(scale=5))
        kind = k % 10
        # SPD P, R over several magnitudes; near the singular threshold (det S = 2.2e-16 at S = 1.2e-4 I) on both sides of it
        sp, sr = (10.0 ** rng.uniform(-7, 3), 10.0 ** rng.uniform(-7, 3)) if kind < 6 else (10.0 ** rng.uniform(-5, -3.5),) * 2
        P, R = _spd(rng, 4, sp), _spd(rng, 4, sr)
        if kind >= 6:
            P, R = sp * np.eye(4) * rng.uniform(0.9, 1.1), sr * np.eye(4) * rng.uniform(0.9, 1.1)
        if kind == 8:  # a non-finite entry somewhere
            target = (x, P, z, R)[rng.integers(4)]
            target.flat[rng.integers(target.size)] = (np.nan, np.inf, -np.inf)[rng.integers(3)]
        if kind == 9:  # an invalid covariance: asymmetric, or indefinite
            if rng.integers(2):
                (P, R)[rng.integers(2)][0, 1] += 1e-3
            else:
                (P, R)[rng.integers(2)][3, 3] = -1.0
        cases.append(np.concatenate([x, P.ravel(), z, R.ravel()]))
    a = np.ascontiguousarray(np.stack(cases))
    got = cape_amd.debug_eval("kalman", a)
    assert got.shape == (len(a), 21)
    want = np.zeros_like(got)
    for k, row in enumerate(a):
        xo, Po = np.zeros(4), np.zeros(16)
        st = host.cape_host_kalman_update(_p(row[0:4]), _p(row[4:20]), _p(row[20:24]), _p(row[24:40]), _p(xo), _p(Po))
        want[k, 0] = st
        if st == 0:
            want[k, 1:5], want[k, 5:] = xo, Po
    counts = [int(np.count_nonzero(want[:, 0] == s)) for s in range(4)]
    print(f"\nkalman: {len(a)} cases, status counts OK / INVALID_INPUT / SINGULAR / INVALID_OUTPUT = {counts}")
    assert counts[0] > 1000 and counts[1] > 100 and counts[2] > 100
    bad = np.flatnonzero((_bits_nan(got) != _bits_nan(want)).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} cases differ, first {bad[:3].tolist()}: {got[bad[0]]} != {want[bad[0]]}"


def test_plane_frame_equals_the_host_twin_on_bit_patterns(host):
    import cape_amd
    from test_map_update_host import _unit

    rng = np.random.default_rng(19)
    normals = [_unit(rng) for _ in range(2000)]
    # each branch of select_correct_transform (the smallest component decides first; the next one within 0.1 of it would decide
    # if the first did not) and normals within 0.1 of its boundaries, on either side
    for perm in ((0, 1, 2), (1, 0, 2), (2, 0, 1), (0, 2, 1), (1, 2, 0), (2, 1, 0)):
        for _ in range(150):
            a = rng.uniform(0, 0.45)
            b = a + 0.1 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-17, -1)
            c2 = 1 - a * a - b * b
            if b < 0 or c2 <= 0:
                continue
            v = np.zeros(3)
            v[list(perm)] = (a, b, np.sqrt(c2))
            normals.append(v * rng.choice([-1, 1], 3))
    # the norm check at 1e-9, non-finite entries, the zero vector
    for _ in range(200):
        normals.append(_unit(rng) * (1 + rng.choice([-1, 1]) * 10.0 ** rng.uniform(-10, -8)))
    normals += [np.zeros(3), np.array([np.nan, 0, 1.0]), np.array([np.inf, 0, 0]), np.array([0, 0, 1.0]), np.array([0, -1.0, 0]),
                np.array([1.0, 0, 0])]
    a = np.ascontiguousarray(np.stack(normals))
    got = cape_amd.debug_eval("plane_frame", a)
    assert got.shape == (len(a), 7)
    want = np.zeros_like(got)
    for k, n in enumerate(a):
        out = np.zeros(6)
        ok = host.cape_host_plane_frame(_p(n), _p(out))
        want[k, 0] = ok
        if ok:
            want[k, 1:] = out
    firsts = [int(np.count_nonzero((want[:, 0] == 1) & (want[:, 1 + k] == 0))) for k in range(3)]  # x = n x e_k has no k component
    print(f"\nplane_frame: {len(a)} normals, {int(want[:, 0].sum())} accepted; x axis orthogonal to e_k (branch k taken): {firsts}")
    assert 0 < want[:, 0].sum() < len(a) and min(firsts) > 100
    bad = np.flatnonzero((_bits_nan(got) != _bits_nan(want)).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} normals differ, first {bad[:3].tolist()}: {a[bad[0]]}: {got[bad[0]]} != {want[bad[0]]}"


# ---- 2. eight room frames ------------------------------------------------------------------------------------------------------
class _Room:
    pass


@pytest.fixture(scope="module")
def room():
    import cape_amd
    from test_gpu_map_match import _stream, _w2c
    from test_gpu_map_measure import _detected, _pose_covariances

    r = _Room()
    r.n = 8
    r.ex, r.st, r.c2w = _stream("room", 11, 20, 5, r.n)
    r.T = np.stack([_c2w(*r.c2w[f]) for f in range(r.n)])
    r.W2C = np.stack([_w2c(*r.c2w[f]) for f in range(r.n)])
    r.S = _pose_covariances(np.random.default_rng(21), r.n)
    r.flags = cape_amd.MATCH_ALLOW_INDEX0
    r.ex.map_measure(r.n, r.T, r.S, r.st)
    meas = r.ex.map_measurements(r.n)
    # the map: the stageable measurements of the first frame with several planes
    r.source = next(f for f in range(r.n) if len(meas[f]) > 1)
    r.map_meas = [m for m in meas[r.source] if m["flags"] & cape_amd.MEASURE_STAGEABLE]
    assert len(r.map_meas) > 1
    r.arrays = cape_amd.pack_map([m["plane"] for m in r.map_meas])
    r.tracks = _tracks(r.map_meas)
    r.det = _detected(r.ex, r.n)
    r.restore = lambda: _run(r, r.T, r.S, None, r.tracks)
    r.restore()
    r.frames, r.rows, r.results, r.matches, r.meas = _compare_with_twin(r.ex, r.n, r.arrays, r.tracks)
    yield r
    r.ex.close()


def _run(r, T, S, skip, tracks):
    r.ex.upload_map(r.arrays)
    r.ex.upload_tracks(tracks)
    r.ex.match_map_wide(r.n, r.W2C, skip, r.flags, r.st)
    r.ex.map_measure(r.n, T, S, r.st)
    r.ex.map_kalman(r.n, r.st)


def test_room_frames_equal_the_twin(room):
    import cape_amd

    n_map = len(room.arrays[0])
    updated = (room.results["result"] & cape_amd.MAP_RESULT_UPDATED) != 0
    changed_normals = changed_cov = pairs = 0
    for f in range(room.n):
        for j in np.flatnonzero(updated[f]):
            row = room.rows[f, room.results[f, j]["kept_plane"]]
            assert row["map_plane"] == j and row["flags"] & cape_amd.FUSION_STATE and row["flags"] & cape_amd.FUSION_FRAME
            pairs += 1
            changed_normals += int(not np.array_equal(_bits(row["normal"]), _bits(room.arrays[0][j]["normal"])))
            # every updated covariance differs from the track's
            assert not np.array_equal(_bits(row["covariance"]), _bits(room.tracks[j]["covariance"]))
            changed_cov += 1
    print(f"\nroom frames: map of {n_map} planes, {pairs} updated pairs over {room.n} frames, {changed_normals} new normals differ from the "
          f"map's in a bit, n_updated per frame {room.frames['n_updated'].tolist()}")
    assert np.array_equal(room.frames["n_updated"], updated.sum(axis=1)) and np.all(room.frames["n_map"] == n_map)
    assert changed_normals >= 1 and changed_cov == pairs and int(room.frames["n_updated"].sum()) >= n_map
    # in the frame the map came from every map plane takes the plane it came from
    assert np.all(updated[room.source])
    # the decisions are not all the same: the counters sit one short of each threshold
    decisions = cape_amd.MAP_RESULT_PROMOTE | cape_amd.MAP_RESULT_DROP | cape_amd.MAP_RESULT_LOST
    assert len({int(v) for v in (room.results["result"] & decisions).ravel()}) > 1


# ---- 3. the chained frame ------------------------------------------------------------------------------------------------------
def test_a_chained_frame_is_fused_through_the_kept_plane_table():
    import cape_amd
    from test_gpu_map_match import _w2c
    from test_gpu_map_measure import _pose_covariances
    from test_gpu_match_map_wide import _chained_input, _extract
    from test_map_update_host import _pose

    frames, Wd, Ht, intr = _chained_input()
    ex, st = _extract(frames, Wd, Ht, intr)
    n = len(frames)
    rng = np.random.default_rng(33)
    T, S = np.stack([_pose(rng) for _ in range(n)]), _pose_covariances(rng, n)
    W2C = np.stack([_w2c(T[f][:3, :3], T[f][:3, 3]) for f in range(n)])
    ex.map_measure(n, T, S, st)
    source = ex.map_measurements(n)[1]
    map_meas = [m for m in source if m["flags"] & cape_amd.MEASURE_STAGEABLE]
    assert len(source) > 64 and len(map_meas) > 64
    arrays, tracks = cape_amd.pack_map([m["plane"] for m in map_meas]), _tracks(map_meas)
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)
    ex.match_map_wide(n, W2C, None, cape_amd.MATCH_ALLOW_INDEX0, st)
    ex.map_kalman(n, st)
    fr, rows, results, _, meas = _compare_with_twin(ex, n, arrays, tracks)
    used, _, _ = ex.spill_info()
    updated = np.flatnonzero(results[1]["result"] & cape_amd.MAP_RESULT_UPDATED)
    kept_of = results[1]["kept_plane"][updated]
    in_spill = [i for i in kept_of if meas[1][i]["segment"] >= 64]
    print(f"\nchained frame: {fr[1]['n_cur']} kept planes against a map of {len(map_meas)}, {len(updated)} updated pairs, "
          f"{int((kept_of >= 64).sum())} with i >= 64, {len(in_spill)} measured in the spill record")
    assert used >= 1 and fr[1]["n_cur"] > 64 and int((kept_of >= 64).sum()) >= 1 and len(in_spill) >= 1
    # the kept-plane table resolved the spill record's rows: the twin above took them from cape_copy_spill_measurements by the chain
    # walk of map_measurements, the device through (record, segment) of the wide match's table
    assert all(rows[1, i]["flags"] & cape_amd.FUSION_STATE and rows[1, i]["map_plane"] >= 0 for i in in_spill)
    ex.close()


# ---- 4. failures follow the twin -----------------------------------------------------------------------------------------------
def test_failures_follow_the_twin(room):
    import cape_amd

    n_map = len(room.arrays[0])
    T, S = room.T.copy(), room.S.copy()
    base_match = room.matches[1]
    hit_frames = [f for f in range(room.n) if (base_match[f] >= 0).any()]
    assert len(hit_frames) >= 3
    f_nan, f_cov, f_skip = hit_frames[0], hit_frames[1], hit_frames[-1]
    j_skip = int(np.flatnonzero(base_match[f_skip] >= 0)[0])
    T[f_nan, 1, 3] = np.nan  # a NaN translation: the measurement rows fail, every matched plane of the frame is FAIL_DETECTION
    S[f_cov, 0, 1] += 1e-3   # an invalid pose covariance
    skip = np.zeros((room.n, (n_map + 31) // 32), np.uint32)
    skip[f_skip, j_skip >> 5] = 1 << (j_skip & 31)  # frame f_skip does not visit map plane j_skip
    _run(room, T, S, skip, room.tracks)
    frames, rows, results, (_, match, _), meas = _compare_with_twin(room.ex, room.n, room.arrays, room.tracks)
    others = [f for f in range(room.n) if f not in (f_nan, f_cov, f_skip)]
    for a, b in ((frames, room.frames), (rows, room.rows), (results, room.results)):
        assert np.array_equal(a[others].view(np.uint8), b[others].view(np.uint8)), "an untouched frame changed"
    M, FD = cape_amd.MAP_RESULT_MATCHED, cape_amd.MAP_RESULT_FAIL_DETECTION
    for f, flag in ((f_nan, 0), (f_cov, cape_amd.KALMAN_BAD_POSE_COV)):
        matched = match[f] >= 0
        assert matched.any() and frames[f]["flags"] == flag and frames[f]["n_updated"] == 0
        assert np.all((results[f]["result"][matched] & (M | FD | cape_amd.MAP_RESULT_UPDATED)) == (M | FD))
        assert not rows[f]["covariance"].any() and not rows[f]["normal"].any()
    assert all(m["flags"] == cape_amd.MEASURE_KEPT | cape_amd.MEASURE_BAD_POSE_COV for m in meas[f_cov])
    assert all(m["flags"] == cape_amd.MEASURE_KEPT | cape_amd.MEASURE_FAIL_WORLD_COV for m in meas[f_nan])
    # the hidden map plane is unmatched and its counters follow update_unmatched
    hidden = results[f_skip, j_skip]
    assert match[f_skip, j_skip] == -1 and hidden["kept_plane"] == -1 and not hidden["result"] & M
    assert hidden["failed_tracking"] == room.tracks[j_skip]["failed_tracking"] + 1
    assert hidden["successive_matched"] == room.tracks[j_skip]["successive_matched"] - 1
    print(f"\nfailures: NaN pose in frame {f_nan}, bad pose covariance in frame {f_cov}, map plane {j_skip} hidden from frame {f_skip}")
    # one map plane with an asymmetric covariance
    bad = room.tracks.copy()
    bad[1]["covariance"][0, 1] += 1e-3
    _run(room, room.T, room.S, None, bad)
    frames, rows, results, (_, match, _), _ = _compare_with_twin(room.ex, room.n, room.arrays, bad)
    hit = match[:, 1] >= 0
    assert hit.any() and np.all(results[hit, 1]["result"] & cape_amd.MAP_RESULT_FAIL_STATE)
    assert not np.any(results[:, [j for j in range(n_map) if j != 1]]["result"] & cape_amd.MAP_RESULT_FAIL_STATE)
    room.restore()


# ---- 5. against the whole host update ----------------------------------------------------------------------------------------------
def test_against_the_whole_host_update(room):
    import cape_amd
    from test_map_update_host import _rel

    n_map = len(room.arrays[0])
    _, match, _ = room.matches
    worst_x = worst_p = 0.0
    pairs = 0
    for f in range(room.n):
        det, _ = room.det[f]
        (P, _, _), Tr, used, _ = cape_amd.host_map_update(room.arrays, room.tracks, match[f], det, room.T[f], room.S[f])
        res = room.results[f]
        assert np.array_equal(res["result"], Tr["result"][:n_map] & ~np.uint32(cape_amd.MAP_RESULT_OVERFLOW)), f"frame {f}: result bits"
        assert np.array_equal(res["successive_matched"], Tr["successive_matched"][:n_map]), f"frame {f}"
        assert np.array_equal(res["failed_tracking"], Tr["failed_tracking"][:n_map]), f"frame {f}"
        n_cur = len(det)
        assert [bool(v) for v in room.rows[f, :n_cur]["flags"] & cape_amd.FUSION_USED] == used.tolist(), f"frame {f}: used"
        for j in np.flatnonzero(res["result"] & cape_amd.MAP_RESULT_UPDATED):
            row = room.rows[f, res[j]["kept_plane"]]
            worst_x = max(worst_x, _rel(np.append(row["normal"], row["d"]), np.append(P[j]["normal"], P[j]["d"])))
            worst_p = max(worst_p, _rel(row["covariance"], Tr[j]["covariance"]))
            pairs += 1
    print(f"\nagainst cape_host_map_update: {pairs} updated pairs, largest relative difference of the new plane {worst_x:.3g}, of the new "
          f"covariance {worst_p:.3g} (bound {KALMAN_BOUND:.3g} = 4 x {PERTURBATION_EFFECT:.3g})")
    assert pairs >= n_map
    assert worst_x <= KALMAN_BOUND and worst_p <= KALMAN_BOUND


# ---- 6. bookkeeping ------------------------------------------------------------------------------------------------------------
def test_bookkeeping(room):
    import torch

    import cape_amd
    from cape_amd import Extractor, synth, synth_gpu

    ex, n, st = room.ex, room.n, room.st
    CAP = r"failed \(-4\)"

    def state():
        rows, ver = ex.measurement_rows(n)
        pol, pver = ex.polygons(n)
        return [np.ascontiguousarray(a).view(np.uint8).copy() for a in (*ex.map_matches_wide(n), rows, ver, pol, pver)]

    # two calls give byte-equal results; the map, the tracks, the matches, the measurement rows and the polygons are left alone
    ex.match_map_wide(n, room.W2C, None, room.flags | cape_amd.MATCH_MAP_AREAS, st)
    before = [np.ascontiguousarray(a).view(np.uint8).copy() for a in ex.map_matches_wide(n, areas=True)] + state()
    ex.map_kalman(n, st)
    first = ex.map_kalman_rows(n)
    ex.map_kalman(n, st)
    second = ex.map_kalman_rows(n)
    after = [np.ascontiguousarray(a).view(np.uint8).copy() for a in ex.map_matches_wide(n, areas=True)] + state()
    for a, b, c in zip(first, second, (room.frames, room.rows, room.results)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # (the map and the tracks: a third call after the inputs were read back still sees the same state)
    ex.map_kalman(n, st)
    assert np.array_equal(ex.map_kalman_rows(n)[1].view(np.uint8), room.rows.view(np.uint8))
    # fewer frames may be copied, more may not
    ex.map_kalman(4, st)
    assert np.array_equal(ex.map_kalman_rows(4)[2].view(np.uint8), room.results[:4].view(np.uint8))
    with pytest.raises(cape_amd.CapeError, match="cape_copy_map_kalman " + CAP):
        ex.map_kalman_rows(5)
    # upload_tracks with a wrong n
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_upload_tracks failed \(-1\)"):
        ex.upload_tracks(room.tracks[:-1])
    # CAPE_ERR_CAPACITY: after a cape_map_upload (no tracks, no wide match against this map) ...
    ex.upload_map(room.arrays)
    with pytest.raises(cape_amd.CapeError, match="cape_map_kalman " + CAP):
        ex.map_kalman(n, st)
    with pytest.raises(cape_amd.CapeError, match="cape_copy_map_kalman " + CAP):
        ex.map_kalman_rows(1)
    ex.upload_tracks(room.tracks)
    with pytest.raises(cape_amd.CapeError, match="cape_map_kalman " + CAP):
        ex.map_kalman(n, st)  # ... tracks, but no wide match since the upload
    ex.match_map_wide(4, room.W2C[:4], None, room.flags, st)
    with pytest.raises(cape_amd.CapeError, match="cape_map_kalman " + CAP):
        ex.map_kalman(5, st)  # ... more frames than the wide match covered
    ex.map_kalman(4, st)
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_measure(4, room.T[:4], room.S[:4], st)
    with pytest.raises(cape_amd.CapeError, match="cape_map_kalman " + CAP):
        ex.map_kalman(5, st)  # ... more frames than the measure covered
    room.restore()
    assert np.array_equal(ex.map_kalman_rows(n)[1].view(np.uint8), room.rows.view(np.uint8))
    # a second handle: without tracks, without a measure, without a wide match, after a new extract; the empty map
    dev = torch.cat([synth_gpu.stream("room", 11, 1, start=20 + 5 * i, device="cuda", chunk=1) for i in range(4)]).contiguous()
    ex2 = Extractor(640, 480, cylinders=False, max_batch=4, **synth.DEFAULT_INTRINSICS)
    ex2.extract_device(dev.data_ptr(), 4, st)
    ex2.build_polygons(4, st)
    ex2.upload_map(room.arrays)
    ex2.match_map_wide(4, room.W2C[:4], None, room.flags, st)
    ex2.map_measure(4, room.T[:4], room.S[:4], st)
    with pytest.raises(cape_amd.CapeError, match="cape_map_kalman " + CAP):
        ex2.map_kalman(4, st)  # no tracks
    ex2.upload_tracks(room.tracks)
    ex2.map_kalman(4, st)
    assert np.array_equal(ex2.map_kalman_rows(4)[1].view(np.uint8), room.rows[:4].view(np.uint8))
    ex2.build_polygons(4, st)  # (discards the measurements)
    with pytest.raises(cape_amd.CapeError, match="cape_map_kalman " + CAP):
        ex2.map_kalman(4, st)  # no measure
    with pytest.raises(cape_amd.CapeError, match="cape_copy_map_kalman " + CAP):
        ex2.map_kalman_rows(1)
    ex2.map_measure(4, room.T[:4], room.S[:4], st)
    ex2.map_kalman(4, st)
    ex2.extract_device(dev.data_ptr(), 4, st)
    with pytest.raises(cape_amd.CapeError, match="cape_copy_map_kalman " + CAP):
        ex2.map_kalman_rows(1)  # the copy after a new extract
    frames_p = C.c_void_p()
    assert ex2.L.cape_device_map_kalman(ex2.h, C.byref(frames_p), None, None) == -4
    ex2.build_polygons(4, st)
    ex2.map_measure(4, room.T[:4], room.S[:4], st)
    with pytest.raises(cape_amd.CapeError, match="cape_map_kalman " + CAP):
        ex2.map_kalman(4, st)  # no wide match on the new batch
    # an empty map succeeds and writes frame headers only
    ex2.upload_map(cape_amd.pack_map([]))
    ex2.upload_tracks(np.zeros(0, cape_amd.MAP_TRACK_DTYPE))
    ex2.match_map_wide(4, room.W2C[:4], None, room.flags, st)
    ex2.map_kalman(4, st)
    frames, rows, results = ex2.map_kalman_rows(4)
    assert results.shape == (4, 0) and np.all(frames["n_map"] == 0) and np.all(frames["n_updated"] == 0)
    assert np.array_equal(frames["n_cur"], room.frames["n_cur"][:4]) and int(frames["n_cur"].sum()) > 0
    for f in range(4):
        k = frames[f]["n_cur"]
        assert np.all(rows[f, :k]["map_plane"] == -1) and not rows[f, :k]["flags"].any() and not rows[f, k:].view(np.uint8).any()
    assert ex2.L.cape_device_map_kalman(ex2.h, C.byref(frames_p), None, None) == 0 and frames_p.value
    fus = ex2.map_fusions(4)
    assert [len(rows_f) for _, rows_f, _ in fus] == frames["n_cur"].tolist()
    ex2.close()

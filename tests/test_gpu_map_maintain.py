"""cape_map_maintain and the retired log (cape_map_retired_info / _download / _clear): PROMOTE, DROP and LOST executed on the device
map -- against the host twin cape_host_map_maintain on the device's own downloaded input, byte for byte (header, planes, rings,
vertices, tracks and log are compared with tobytes()), and, over a loop of eight frames of commit + maintain, against the pure host
route.

Every test prints its figures before it asserts (`pytest -s`)."""
import numpy as np
import pytest

import map_maintain_cases as MC
from test_gpu_map_commit import _commit_both, _wall_copies
from test_gpu_map_kalman import room  # noqa: F401  (the eight room frames after the four calls)

pytestmark = pytest.mark.gpu

CAP = r"failed \(-4\)"
N, X, Y = np.array([0.0, 0.0, -1.0]), np.array([1.0, 0, 0]), np.array([0, 1.0, 0])
TRIANGLE = np.array([[0.0, 0.0], [0.0, 100.0], [100.0, 0.0]])  # clockwise: the host class's outer ring


def _maintain_both(ca, ex, st, what=""):
    """the call on the device and through the twin on the downloaded map, tracks and log: header, map, tracks and log byte for byte --
    the old ones where the call is not DONE.  Returns (result, the map and tracks after, the log after)."""
    before, log_before = ex.download_map(), ex.download_retired()
    new, Tr, log_want, want = ca.host_map_maintain(before[0], before[1], log_before)
    result = ex.map_maintain(0, st)
    after, log_after = ex.download_map(), ex.download_retired()
    print(f"{what}flags {int(result['flags']):#x}, {int(result['n_planes'])} planes ({int(result['n_local'])} local, {int(result['n_staged'])} staged), "
          f"{int(result['n_rings'])} rings, {int(result['n_vertices'])} vertices; promoted {int(result['n_promoted'])}, refused "
          f"{int(result['n_promote_refused'])}, dropped {int(result['n_dropped'])}, lost {int(result['n_lost'])}; log {int(result['n_retired'])} planes, "
          f"{int(result['n_retired_rings'])} rings, {int(result['n_retired_vertices'])} vertices")
    assert result.tobytes() == want.tobytes(), f"{what}header {result} != {want}"
    assert ex.map_info() == (int(result["n_planes"]), int(result["n_rings"]), int(result["n_vertices"]))
    assert ex.retired_info() == (int(result["n_retired"]), int(result["n_retired_rings"]), int(result["n_retired_vertices"]))
    if result["flags"] == ca.MAINTAIN_DONE:
        MC.same_map(after, (new, Tr), what + "the new map")
    else:
        MC.same_map(after, before, what + "the map of a call that is not DONE")
    MC.same_map(log_after, log_want, what + "the log")
    return result, after, log_after


def _bad_covariances(cov):
    nan = cov.copy()
    nan[1, 2] = np.nan
    skew = cov.copy()
    skew[0, 1] += 0.5 * np.abs(cov).max()
    return [nan, skew, np.diag([1.0, 1.0, -1.0, 1.0])]


# a track of each class: (flags, successive_matched, failed_tracking, a covariance that is not valid)
def _track_of(ca, cls, rng, cov):
    staged, moving = ca.MAP_TRACK_STAGED, (ca.MAP_TRACK_MOVING if rng.integers(4) == 0 else 0)
    bad = _bad_covariances(cov)
    return {MC.KEEP_LOCAL: (moving, int(rng.integers(-3, 9)), int(rng.integers(0, 10)), None),
            MC.PROMOTED: (staged | moving, int(rng.integers(4, 9)), int(rng.integers(0, 4)), None),
            MC.KEEP_STAGED: (staged, int(rng.integers(-3, 4)), int(rng.integers(0, 2)), None),
            MC.DROPPED: (staged, int(rng.integers(-3, 4)), int(rng.integers(2, 5)), None),
            MC.LOST: (moving, int(rng.integers(-3, 9)), int(rng.integers(10, 13)), None),
            MC.PROMOTE_REFUSED: (staged, int(rng.integers(4, 9)), int(rng.integers(0, 4)), bad[int(rng.integers(3))])}[cls]


def _random_map(ca, room, size, rng):  # noqa: F811
    """`size` wall copies, every fifth with one or two holes, and tracks of classes drawn per plane"""
    arrays, tracks = _wall_copies(ca, room, size, rng, far=True)
    entries = MC.entries_of(arrays, tracks)
    classes = rng.integers(0, 6, size)
    for j, e in enumerate(entries):
        if j % 5 == 2:
            centre = e["rings"][0].mean(axis=0)
            e["rings"] += [centre + (k + 1) * TRIANGLE[::-1] * 0.2 for k in range(1 + j % 2)]
        flags, sm, ft, bad = _track_of(ca, int(classes[j]), rng, e["track"]["covariance"])
        e["track"]["flags"], e["track"]["successive_matched"], e["track"]["failed_tracking"] = flags, sm, ft
        e["track"]["result"] = 3 * j + 1
        if bad is not None:
            e["track"]["covariance"] = bad
    return MC.arrays_of(ca, entries), classes


def _tiny_map(ca, n, flags=0, sm=0, ft=10, first_id=0):
    """n planes of one triangle each, all with the same counters"""
    planes = [(N, 1000.0 + j, X, Y, np.array([0, 0, 1000.0 + j]), TRIANGLE + [j, 0], []) for j in range(n)]
    tracks = np.zeros(n, ca.MAP_TRACK_DTYPE)
    tracks["covariance"] = np.eye(4)
    tracks["flags"], tracks["successive_matched"], tracks["failed_tracking"] = flags, sm, ft
    tracks["id"] = first_id + np.arange(n)
    return ca.pack_map(planes), tracks


def _upload(ex, arrays, tracks):
    ex.upload_map(arrays)
    ex.upload_tracks(tracks)


# ---- 1. widths ------------------------------------------------------------------------------------------------------------------
# the plan kernel decides four map planes per lane (3 / 4 / 5), 256 per wave (255 / 256 / 257) and 1 024 per workgroup; 63 / 64 / 65
# lie on either side of a quarter of a wave's planes
WIDTHS = [3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024]


@pytest.mark.parametrize("size", WIDTHS)
def test_map_widths(room, size):  # noqa: F811
    import cape_amd as ca

    ex, st = room.ex, room.st
    ex.clear_retired()
    (arrays, tracks), classes = _random_map(ca, room, size, np.random.default_rng(100 + size))
    _upload(ex, arrays, tracks)
    print()
    result, (_, Tr), (_, logT) = _maintain_both(ca, ex, st, f"{size} planes, ")
    count = [int(np.count_nonzero(classes == c)) for c in range(6)]
    assert [int(result[k]) for k in ("n_promoted", "n_dropped", "n_lost", "n_promote_refused")] == [count[MC.PROMOTED], count[MC.DROPPED], count[MC.LOST],
                                                                                                   count[MC.PROMOTE_REFUSED]]
    assert (result["n_local"], result["n_staged"]) == (count[MC.KEEP_LOCAL] + count[MC.PROMOTED], count[MC.KEEP_STAGED] + count[MC.PROMOTE_REFUSED])
    if size >= 63:
        assert min(count) >= 1 and result["flags"] == ca.MAINTAIN_DONE
        # every class on both sides of each wave boundary the map reaches, and in both halves of some lane's four planes
        for edge in (b for b in (256, 512, 768) if 64 < b < size - 64):
            assert set(classes[edge - 64: edge]) == set(classes[edge: edge + 64]) == set(range(6)), edge
    if result["flags"] == ca.MAINTAIN_DONE:
        ids = 5000 + np.arange(size)
        keep = np.concatenate([ids[(classes == MC.KEEP_LOCAL) | (classes == MC.PROMOTED)], ids[(classes == MC.KEEP_STAGED) | (classes == MC.PROMOTE_REFUSED)]])
        assert Tr["id"].tolist() == keep.tolist() and logT["id"].tolist() == ids[classes == MC.LOST].tolist()
        # idempotent: the second call finds nothing due
        again, _, _ = _maintain_both(ca, ex, st, f"{size} planes again, ")
        assert again["flags"] == ca.MAINTAIN_NOTHING and again["n_promote_refused"] == result["n_promote_refused"]
    if size == WIDTHS[-1]:
        ex.clear_retired()
        room.restore()


# ---- 2. nothing due, everything removed -----------------------------------------------------------------------------------------
def test_a_map_where_nothing_is_due(room):  # noqa: F811
    """the room's own map and tracks, whose counters are one short of each threshold: NOTHING -- the download, the Kalman and the union
    results are unchanged and still current, and the frame still commits"""
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    room.restore()
    ex.map_union_cut(n, st)
    state = [np.ascontiguousarray(a).tobytes() for a in (*ex.map_kalman_rows(n), *ex.map_union_rows(n), ex.map_union_ring_rows(n))]
    print()
    result, _, _ = _maintain_both(ca, ex, st, "the room's map, ")
    assert result["flags"] == ca.MAINTAIN_NOTHING and result["n_planes"] == len(room.arrays[0])
    assert [np.ascontiguousarray(a).tobytes() for a in (*ex.map_kalman_rows(n), *ex.map_union_rows(n), ex.map_union_ring_rows(n))] == state
    f = room.source
    commit, _, _, _ = _commit_both(ca, ex, st, n, f, room.meas[f], 0, 0, what="after NOTHING, ")
    assert commit["flags"] == ca.COMMIT_DONE
    room.restore()


def test_a_map_that_is_removed_whole(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    ex.clear_retired()
    tracks = room.tracks.copy()
    staged = (tracks["flags"] & ca.MAP_TRACK_STAGED) != 0
    tracks["successive_matched"] = 0
    tracks["failed_tracking"] = np.where(staged, 2, 10)
    _upload(ex, room.arrays, tracks)
    print()
    result, ((P, R, V), Tr), (_, logT) = _maintain_both(ca, ex, st, "every plane due, ")
    assert result["flags"] == ca.MAINTAIN_DONE and (result["n_planes"], result["n_rings"], result["n_vertices"]) == (0, 0, 0)
    assert len(P) == len(R) == len(V) == len(Tr) == 0 and logT["id"].tolist() == tracks["id"][~staged].tolist()
    assert result["n_dropped"] == np.count_nonzero(staged) >= 1 and result["n_lost"] == np.count_nonzero(~staged) >= 1
    # the next frame runs against the empty map
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    frames, _, results = ex.map_kalman_rows(n)
    assert np.all(frames["n_map"] == 0) and np.all(frames["n_updated"] == 0) and results.shape == (n, 0)
    ex.clear_retired()
    room.restore()


# ---- 3. refused promotions ------------------------------------------------------------------------------------------------------
def test_refused_promotions(room):  # noqa: F811
    """a NaN entry, an asymmetric covariance, one with a negative pivot: is_covariance_valid<4> on the device refuses each as the host
    algebra does.  The fourth cause, a normal that is not a unit vector, cannot reach the device map through cape_map_upload, which
    refuses it; the twin's case is in tests/test_map_maintain_host.py."""
    import cape_amd as ca

    ex, st = room.ex, room.st
    (P, R, V), tracks = room.arrays, room.tracks.copy()
    tracks["flags"], tracks["successive_matched"], tracks["failed_tracking"] = ca.MAP_TRACK_STAGED, 5, 6
    bad = _bad_covariances(tracks[0]["covariance"])
    assert len(tracks) >= 2
    print()
    for k, cov in enumerate(bad):
        sent = tracks.copy()
        sent[0]["covariance"] = cov
        _upload(ex, room.arrays, sent)
        result, (_, Tr), _ = _maintain_both(ca, ex, st, f"bad covariance {k}, ")
        assert result["flags"] == ca.MAINTAIN_DONE and result["n_promote_refused"] == 1 and result["n_promoted"] == len(tracks) - 1
        assert result["n_dropped"] == 0 and Tr[-1].tobytes() == sent[0].tobytes() and np.all(Tr["flags"][:-1] == 0)
        # alone it is nothing to do
        _upload(ex, (P[:1], R[:P[0]["ring_count"]], V[:int(R[:P[0]["ring_count"]]["vertex_count"].sum())]), sent[:1])
        result, _, _ = _maintain_both(ca, ex, st, f"bad covariance {k} alone, ")
        assert result["flags"] == ca.MAINTAIN_NOTHING and result["n_promote_refused"] == 1
    scaled = P.copy()
    scaled[0]["normal"] = scaled[0]["normal"] * (1.0 + 1e-12)
    with pytest.raises(ca.CapeError, match=r"cape_map_upload failed \(-1\)"):
        ex.upload_map((scaled, R, V))
    room.restore()


# ---- 4. the log -----------------------------------------------------------------------------------------------------------------
def test_the_log_over_two_calls_and_cleared(room):  # noqa: F811
    import cape_amd as ca

    ex, st = room.ex, room.st
    ex.clear_retired()
    assert ex.retired_info() == (0, 0, 0) and len(ex.download_retired()[1]) == 0
    print()
    (arrays, tracks), classes = _random_map(ca, room, 120, np.random.default_rng(5))
    _upload(ex, arrays, tracks)
    first, _, (_, logT) = _maintain_both(ca, ex, st, "first call, ")
    (arrays2, tracks2), classes2 = _random_map(ca, room, 200, np.random.default_rng(6))
    tracks2["id"] += 1000
    _upload(ex, arrays2, tracks2)  # (the log survives the upload)
    assert ex.retired_info()[0] == first["n_retired"] == first["n_lost"] >= 1
    second, _, ((LP, LR, LV), LT) = _maintain_both(ca, ex, st, "second call, ")
    assert second["n_lost"] >= 1 and second["n_retired"] == first["n_lost"] + second["n_lost"]
    assert LT["id"].tolist() == (5000 + np.flatnonzero(classes == MC.LOST)).tolist() + (6000 + np.flatnonzero(classes2 == MC.LOST)).tolist()
    assert np.any(LP["ring_count"] > 1), "no logged plane has a hole"
    # the log is a map of its own: offsets relative to its own arrays, back to back
    assert LP["ring_first"].tolist() == np.concatenate([[0], np.cumsum(LP["ring_count"])[:-1]]).tolist()
    assert LR["vertex_offset"].tolist() == np.concatenate([[0], np.cumsum(LR["vertex_count"])[:-1]]).tolist() and len(LV) == LR["vertex_count"].sum()
    # arrays that are too small
    n, r, v = ex.retired_info()
    for caps in ((n - 1, r, v), (n, r - 1, v), (n, r, v - 1)):
        assert ex.L.cape_map_retired_download(ex.h, LP.ctypes.data, caps[0], LR.ctypes.data, caps[1], LV.ctypes.data, caps[2], None) == ca.CAPE_ERR_CAPACITY
    ex.clear_retired()
    assert ex.retired_info() == (0, 0, 0)
    _upload(ex, arrays, tracks)
    third, _, (_, logT3) = _maintain_both(ca, ex, st, "after the clear, ")
    assert logT3.tobytes() == logT.tobytes() and third["n_retired"] == first["n_retired"]
    ex.clear_retired()
    room.restore()


def _fill_log(ca, ex, st, count):
    """`count` lost triangles into the cleared log, 1 024 per call"""
    ex.clear_retired()
    at = 0
    while at < count:
        n = min(ca.MAP_MAX_PLANES, count - at)
        _upload(ex, *_tiny_map(ca, n, first_id=at))
        result = ex.map_maintain(0, st)
        assert result["flags"] == ca.MAINTAIN_DONE and result["n_lost"] == n
        at += n
    assert ex.retired_info() == (count, count, 3 * count)


def test_the_log_is_full_at_its_cap(room):  # noqa: F811
    import cape_amd as ca

    ex, st = room.ex, room.st
    cap = ca.MAP_RETIRED_MAX_PLANES
    _fill_log(ca, ex, st, cap - 1)
    print()
    _upload(ex, *_tiny_map(ca, 2, first_id=9000))
    result, _, _ = _maintain_both(ca, ex, st, f"{cap - 1} in the log, two lost, ")
    assert result["flags"] == ca.MAINTAIN_LOG_FULL and result["n_retired"] == cap - 1 and result["n_planes"] == 2
    _upload(ex, *_tiny_map(ca, 1, first_id=9000))
    result, _, (_, logT) = _maintain_both(ca, ex, st, f"{cap - 1} in the log, one lost, ")
    assert result["flags"] == ca.MAINTAIN_DONE and result["n_retired"] == cap and logT["id"].tolist() == list(range(cap - 1)) + [9000]
    _upload(ex, *_tiny_map(ca, 1, first_id=9001))
    result, _, _ = _maintain_both(ca, ex, st, f"{cap} in the log, one lost, ")
    assert result["flags"] == ca.MAINTAIN_LOG_FULL and result["n_lost"] == 1
    # a full log refuses no call that loses nothing
    _upload(ex, *_tiny_map(ca, 3, flags=ca.MAP_TRACK_STAGED, ft=2))
    result, _, _ = _maintain_both(ca, ex, st, f"{cap} in the log, three dropped, ")
    assert result["flags"] == ca.MAINTAIN_DONE and result["n_dropped"] == 3 and result["n_retired"] == cap
    ex.clear_retired()
    room.restore()


# ---- 5. the loop ----------------------------------------------------------------------------------------------------------------
def test_a_loop_of_eight_frames_of_commit_and_maintain(room):  # noqa: F811
    """The room's map plus three far wall copies that never match -- a staged one at failed_tracking 1, a local one at 9 -- with the
    room's own staged planes at successive_matched 3.  For f = 0 .. 7 on the same batch: wide match, Kalman, union_cut, commit(f),
    maintain, no upload in between.  After every step the download is the twins' on the device's rows.  After the last step the map and
    the log are compared with the pure host route (cape_host_match_map + cape_host_map_update + cape_host_map_maintain per frame):
    counts, ids, counters, flags and result bits must agree; the largest parameter and vertex differences are printed (the
    covariances pass through two different pows; no bound is fixed for them)."""
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    ex.clear_retired()
    far, far_tracks = _wall_copies(ca, room, 3, np.random.default_rng(12), far=True)
    far_tracks["flags"] = [ca.MAP_TRACK_STAGED, 0, ca.MAP_TRACK_STAGED]
    far_tracks["successive_matched"] = [0, 2, -1]
    far_tracks["failed_tracking"] = [1, 9, 0]
    far_tracks["id"] = [900, 901, 902]
    arrays, tracks = MC.arrays_of(ca, MC.entries_of(room.arrays, room.tracks) + MC.entries_of(far, far_tracks))
    assert np.any((tracks["flags"] & ca.MAP_TRACK_STAGED != 0) & (tracks["successive_matched"] == 3))
    _upload(ex, arrays, tracks)
    start = ex.download_map()  # (the rings as the host class holds them)
    next_id, totals = 1000, np.zeros(3, int)
    print()
    for f in range(n):
        ex.match_map_wide(n, room.W2C, None, room.flags, st)
        ex.map_kalman(n, st)
        ex.map_union_cut(n, st)
        commit, next_id, committed, _ = _commit_both(ca, ex, st, n, f, room.meas[f], ca.COMMIT_ADD_STAGED, next_id, what="loop, ")
        assert commit["flags"] == ca.COMMIT_DONE, f"step {f} is refused"
        # the counters the commit wrote name the class its result bits name
        for t in committed[1]:
            assert MC.class_of(ca, t) == MC.class_of_result(ca, int(t["result"]), bool(t["flags"] & ca.MAP_TRACK_STAGED))
        result, device, log = _maintain_both(ca, ex, st, f"loop, frame {f}: ")
        assert result["n_promote_refused"] == 0
        totals += [int(result["n_promoted"]), int(result["n_dropped"]), int(result["n_lost"])]
    print(f"over the loop: {totals[0]} promoted, {totals[1]} dropped, {totals[2]} lost")
    assert np.all(totals >= 1)
    (P, R, V), Tr = device
    (LP, LR, LV), LT = log
    assert 901 in LT["id"].tolist() and 900 not in Tr["id"].tolist() + LT["id"].tolist() and len(LT) == totals[2]
    # the pure host route
    A, Th, host_id, host_log = start[0], start[1], 1000, None
    for f in range(n):
        det, _ = room.det[f]
        match, _ = ca.host_match_map(A, [d[:7] for d in det], room.W2C[f], None, room.flags)
        A, Th, _, host_id = ca.host_map_update(A, Th, match, det, room.T[f], room.S[f], ca.MAP_ADD_STAGED, host_id)
        A2, Th2, host_log, result = ca.host_map_maintain(A, Th, host_log)
        if result["flags"] == ca.MAINTAIN_DONE:
            A, Th = A2, Th2
    (HP, HR, HV), (HLP, HLR, HLV), HLT = A, host_log[0], host_log[1]
    print(f"after eight frames: device {len(P)} planes, {len(R)} rings, {len(V)} vertices, log {len(LP)}, next id {next_id}; host route {len(HP)} planes, "
          f"{len(HR)} rings, {len(HV)} vertices, log {len(HLP)}, next id {host_id}")
    same_shape = (len(P), len(R), len(V), len(LP), len(LR), len(LV)) == (len(HP), len(HR), len(HV), len(HLP), len(HLR), len(HLV))
    if same_shape:
        params = max(float(np.max(np.abs(P[k] - HP[k]))) for k in ("normal", "d", "x_axis", "y_axis", "center"))
        print(f"largest parameter difference {params:.3g}, largest covariance difference (relative) "
              f"{float(np.max(np.abs(Tr['covariance'] - Th['covariance']) / np.maximum(np.abs(Th['covariance']), 1e-300).max())):.3g}, "
              f"largest vertex difference {float(np.max(np.abs(V - HV))) if len(V) else 0.0:.3g} mm")
    assert same_shape and next_id == host_id
    assert np.array_equal(R["vertex_count"], HR["vertex_count"]) and np.array_equal(P["ring_count"], HP["ring_count"])
    for k in ("id", "successive_matched", "failed_tracking", "result", "flags"):
        assert np.array_equal(Tr[k], Th[k]), k
        assert np.array_equal(LT[k], HLT[k]), "log: " + k
    ex.clear_retired()
    room.restore()


# ---- 6. bookkeeping -------------------------------------------------------------------------------------------------------------
def test_bookkeeping(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    ex.clear_retired()
    with pytest.raises(ca.CapeError, match=r"cape_map_maintain failed \(-1\)"):
        ex.map_maintain(1, st)
    ex.upload_map(room.arrays)  # a new map discards the tracks: none are current
    with pytest.raises(ca.CapeError, match="cape_map_maintain " + CAP):
        ex.map_maintain(0, st)

    def buffers():
        rows, ver = ex.measurement_rows(n)
        return [np.ascontiguousarray(a).view(np.uint8).copy() for a in (*ex.map_matches_wide(n), rows, ver, *ex.map_kalman_rows(n), *ex.map_union_rows(n),
                                                                          ex.map_union_ring_rows(n))]

    # a refused call (the log made full, a local plane lost) leaves every result buffer as it was, and current
    _fill_log(ca, ex, st, ca.MAP_RETIRED_MAX_PLANES)
    due = room.tracks.copy()
    local = int(np.flatnonzero((due["flags"] & ca.MAP_TRACK_STAGED) == 0)[0])
    due[local]["failed_tracking"] = 10
    ex.upload_map(room.arrays)
    ex.upload_tracks(due)
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    ex.map_union_cut(n, st)
    full = buffers()
    print()
    result, _, _ = _maintain_both(ca, ex, st, "bookkeeping, the full log, ")
    assert result["flags"] == ca.MAINTAIN_LOG_FULL and result["n_lost"] == 1
    assert all(np.array_equal(a, b) for a, b in zip(full, buffers())), "a refused call wrote into a result buffer"
    # after DONE (the log cleared): the match, Kalman and union results are gone until a new wide match ...
    ex.clear_retired()
    result, maintained, (_, logT) = _maintain_both(ca, ex, st, "bookkeeping, ")
    assert result["flags"] == ca.MAINTAIN_DONE and logT["id"].tolist() == [int(due[local]["id"])]
    with pytest.raises(ca.CapeError, match="cape_map_kalman " + CAP):
        ex.map_kalman(n, st)
    with pytest.raises(ca.CapeError, match="cape_copy_map_union " + CAP):
        ex.map_union_rows(1)
    with pytest.raises(ca.CapeError, match="cape_map_commit " + CAP):
        ex.map_commit(0, 0, 0, st)
    # ... the measurement rows are still valid, and the tracks are the maintained ones: wide match + Kalman without upload_tracks
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    frames, rows, results = ex.map_kalman_rows(n)
    _, match, _, _ = ex.map_matches_wide(n)
    for g in range(n):
        frame, trows, tres = ca.host_map_kalman(maintained[0], maintained[1], match[g], room.meas[g])
        k = len(room.meas[g])
        assert frames[g].tobytes() == frame.tobytes() and rows[g, :k].tobytes() == trows.tobytes() and results[g].tobytes() == tres.tobytes(), g
    ex.clear_retired()
    room.restore()

"""cape_map_step: one frame through wide match, Kalman step, union with cuts, commit and maintenance in one call with one wait --
against the five calls (cape_match_map_wide, cape_map_kalman, cape_map_union_cut, cape_map_commit and, behind a DONE commit,
cape_map_maintain) on a second upload of the same map, tracks and log.  Everything is compared byte for byte (tobytes()): the two
headers, the map, the tracks with their ids, the retired log and next_id.  Where the five-call route goes through _commit_both and
_maintain_both it is itself checked against the two host twins on the device's own rows.

Every test prints its figures before it asserts (`pytest -s`)."""
import ctypes as C

import numpy as np
import pytest

import capacity_cases as K
import map_maintain_cases as MC
from test_gpu_map_commit import _commit_both, _wall_copies
from test_gpu_map_kalman import room  # noqa: F401  (the eight room frames after the four calls)
from test_gpu_map_maintain import _fill_log, _maintain_both, _random_map, _upload

pytestmark = pytest.mark.gpu

INV, CAP = r"failed \(-1\)", r"failed \(-4\)"


def _state(ex):
    """what a step may change: the map with its tracks and ids, and the log"""
    return ex.download_map(), ex.download_retired()


def _same_state(got, want, what):
    MC.same_map(got[0], want[0], what + ": the map")
    MC.same_map(got[1], want[1], what + ": the log")


def _five_calls(ca, ex, st, n, f, W2C, skip, match_flags, commit_flags, next_id, meas_f=None, what=""):
    """the route the step stands for, on the first n frames of the batch.  With meas_f the commit and the maintenance go through
    _commit_both and _maintain_both: each against its twin on the device's own rows.  Returns (commit, maintain, next_id)."""
    ex.match_map_wide(n, W2C, skip, match_flags, st)
    ex.map_kalman(n, st)
    ex.map_union_cut(n, st)
    if meas_f is None:
        commit, nid = ex.map_commit(f, commit_flags, next_id, st)
    else:
        commit, nid, _, _ = _commit_both(ca, ex, st, n, f, meas_f, commit_flags, next_id, what=what + "five calls, ")
    maintain = np.zeros(1, ca.MAP_MAINTAIN_RESULT_DTYPE)[0]
    if commit["flags"] & ca.COMMIT_DONE:
        maintain = ex.map_maintain(0, st) if meas_f is None else _maintain_both(ca, ex, st, what + "five calls, ")[0]
    return commit, maintain, nid


def _step(ca, ex, st, f, W2C, skip_f, match_flags, commit_flags, next_id, want, what):
    """the step, and its two headers, next_id and the sizes the handle reports against `want` = _five_calls' result"""
    result, nid = ex.map_step(f, W2C[f] if W2C is not None else np.eye(4), skip_f, match_flags, commit_flags, next_id, st)
    c, m = result["commit"], result["maintain"]
    print(f"{what}step({f}): commit {int(c['flags']):#x}, {int(c['n_planes'])} planes, updated {int(c['n_updated'])}, appended {int(c['n_appended'])}; "
          f"maintain {int(m['flags']):#x}, {int(m['n_planes'])} planes, promoted {int(m['n_promoted'])}, dropped {int(m['n_dropped'])}, lost "
          f"{int(m['n_lost'])}, log {int(m['n_retired'])}; next id {nid}")
    assert c.tobytes() == want[0].tobytes(), f"{what}commit header {c} != {want[0]}"
    assert m.tobytes() == want[1].tobytes(), f"{what}maintain header {m} != {want[1]}"
    assert nid == want[2]
    last = m if m["flags"] & ca.MAINTAIN_DONE else c
    assert ex.map_info() == (int(last["n_planes"]), int(last["n_rings"]), int(last["n_vertices"]))
    if m["flags"]:
        assert ex.retired_info() == (int(m["n_retired"]), int(m["n_retired_rings"]), int(m["n_retired_vertices"]))
    return c, m, nid


def _both_routes(ca, room, f, arrays, tracks, commit_flags, next_id, what, skip_f=None, fill=None, twins=True):  # noqa: F811
    """frame f of the room by the five calls and by the step, each from its own upload of (arrays, tracks) and the log `fill` leaves
    (None: the cleared log).  Returns (commit, maintain, the state after, the state before)."""
    ex, n, st = room.ex, room.n, room.st
    skip = None
    if skip_f is not None:
        skip = np.zeros((n, len(skip_f)), np.uint32)
        skip[f] = skip_f
    states = []
    for route in ("five", "step"):
        if fill is None:
            ex.clear_retired()
        elif route == "five":
            fill()  # (a route that leaves the log as it was needs no second filling: asserted below)
        _upload(ex, arrays, tracks)
        before = _state(ex)
        if route == "five":
            want = _five_calls(ca, ex, st, n, f, room.W2C, skip, room.flags, commit_flags, next_id, room.meas[f] if twins else None, what)
            log_five = before[1]
        else:
            if fill is not None:
                MC.same_map(before[1], log_five, what + "the log before the second route")
            c, m, _ = _step(ca, ex, st, f, room.W2C, skip_f, room.flags, commit_flags, next_id, want, what)
        states.append(_state(ex))
    _same_state(states[1], states[0], what + "after the step")
    return c, m, states[1], before


def _loop_map(ca, room):  # noqa: F811
    """the room's map plus three far wall copies that never match: a staged one at failed_tracking 1, a local one at 9"""
    far, far_tracks = _wall_copies(ca, room, 3, np.random.default_rng(12), far=True)
    far_tracks["flags"] = [ca.MAP_TRACK_STAGED, 0, ca.MAP_TRACK_STAGED]
    far_tracks["successive_matched"] = [0, 2, -1]
    far_tracks["failed_tracking"] = [1, 9, 0]
    far_tracks["id"] = [900, 901, 902]
    return MC.arrays_of(ca, MC.entries_of(room.arrays, room.tracks) + MC.entries_of(far, far_tracks))


def _stageable(ca, room, f):  # noqa: F811
    return sum(bool(m["flags"] & ca.MEASURE_STAGEABLE) for m in room.meas[f])


# ---- 6. growth of the destination set (first: the module's handle has not stepped yet, its third buffer set is empty) ------------
def test_the_third_set_grows_from_a_map_uploaded_at_its_exact_size(room):  # noqa: F811
    """cape_map_upload allocates the map at its exact size.  The first step appends planes (the commit's destination grows) and its
    maintenance is DONE (it writes the third set, allocated by this call, to the commit's bounds); the second step follows without an
    upload, its front set the first one's third."""
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    arrays, tracks = _loop_map(ca, room)
    f = max(range(n), key=lambda g: _stageable(ca, room, g))
    g = (f + 1) % n
    print()
    ex.clear_retired()
    _upload(ex, arrays, tracks)
    first = _five_calls(ca, ex, st, n, f, room.W2C, None, room.flags, ca.COMMIT_ADD_STAGED, 400, room.meas[f], "growth, ")
    mid = _state(ex)
    second = _five_calls(ca, ex, st, n, g, room.W2C, None, room.flags, ca.COMMIT_ADD_STAGED, first[2], room.meas[g], "growth, ")
    end = _state(ex)
    ex.clear_retired()
    _upload(ex, arrays, tracks)
    c, m, nid = _step(ca, ex, st, f, room.W2C, None, room.flags, ca.COMMIT_ADD_STAGED, 400, first, "growth, ")
    assert c["flags"] == ca.COMMIT_DONE and c["n_appended"] >= 1 and c["n_planes"] > len(arrays[0]) and m["flags"] == ca.MAINTAIN_DONE
    _same_state(_state(ex), mid, "growth, after the first step")
    c, m, nid = _step(ca, ex, st, g, room.W2C, None, room.flags, ca.COMMIT_ADD_STAGED, nid, second, "growth, ")
    assert c["flags"] == ca.COMMIT_DONE
    _same_state(_state(ex), end, "growth, after the second step")
    ex.clear_retired()
    room.restore()


# ---- 1. each room frame alone ---------------------------------------------------------------------------------------------------
def test_each_room_frame_alone(room):  # noqa: F811
    """from the same upload, frames f = 0 .. 7 one at a time: at f > 0 the frame's chain is found through the chain base"""
    import cape_amd as ca

    done = updated = appended = 0
    print()
    for f in range(room.n):
        c, m, after, _ = _both_routes(ca, room, f, room.arrays, room.tracks, ca.COMMIT_ADD_STAGED, 1000 + f, f"frame {f}, ")
        assert c["flags"] == ca.COMMIT_DONE and c["frame"] == f and c["n_updated"] == room.frames[f]["n_updated"]
        assert m["flags"] in (ca.MAINTAIN_DONE, ca.MAINTAIN_NOTHING)
        done += int(m["flags"] == ca.MAINTAIN_DONE)
        updated += int(c["n_updated"])
        appended += int(c["n_appended"])
    print(f"eight room frames, each alone: {updated} planes updated, {appended} appended, the maintenance DONE behind {done} of them")
    assert updated >= len(room.arrays[0]) and appended >= 1
    room.ex.clear_retired()
    room.restore()


# ---- 2. a frame whose record chain spills ---------------------------------------------------------------------------------------
def test_a_chained_frame_at_batch_position_one():
    """the wall behind the lattice with 65 panes at batch position 1 (position 0: the 64-pane lattice): 65 kept planes over two
    records -- record 1 and a spill record -- appended to an empty map, then matched against the map they made"""
    import cape_amd as ca
    from test_gpu_map_measure import _pose_covariances
    from test_gpu_match_wide import _extract

    depth, intr, _ = K.lattice_with(65, 1280, 960, 4, 5)
    other, _, _ = K.lattice_with(64, 1280, 960, 4, 5)
    ex, st = _extract(np.stack([other, depth]), 1280, 960, intr)
    assert len(ex.results(2).chain(1)) == 2
    ex.map_measure(2, None, _pose_covariances(np.random.default_rng(4), 2), st)
    meas = ex.map_measurements(2)
    assert len(meas[1]) == 65 and meas[1][-1]["segment"] >= 64
    empty = (ca.pack_map([]), np.zeros(0, ca.MAP_TRACK_DTYPE))
    flags, add = ca.MATCH_ALLOW_INDEX0, ca.COMMIT_ADD_STAGED
    print()
    _upload(ex, *empty)
    first = _five_calls(ca, ex, st, 2, 1, None, None, flags, add, 300, meas[1], "lattice, ")
    mid = _state(ex)
    second = _five_calls(ca, ex, st, 2, 1, None, None, flags, add, first[2], meas[1], "lattice again, ")
    end = _state(ex)
    _upload(ex, *empty)
    c, m, nid = _step(ca, ex, st, 1, None, None, flags, add, 300, first, "lattice, ")
    assert c["flags"] == ca.COMMIT_DONE and c["n_appended"] == 65 and nid == 365
    _same_state(_state(ex), mid, "lattice, after the first step")
    assert _state(ex)[0][1]["id"].tolist() == list(range(300, 365))
    c, m, nid = _step(ca, ex, st, 1, None, None, flags, add, nid, second, "lattice again, ")
    _same_state(_state(ex), end, "lattice, after the second step")
    if c["flags"] & ca.COMMIT_DONE:
        assert c["n_updated"] + c["n_appended"] >= 1
    ex.close()


# ---- 3. the loop ----------------------------------------------------------------------------------------------------------------
def test_a_loop_of_eight_steps_without_an_upload(room):  # noqa: F811
    """the setup of test_gpu_map_maintain's loop, by the five calls and then by eight steps with no upload in between: equal after
    every step"""
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    arrays, tracks = _loop_map(ca, room)
    print()
    ex.clear_retired()
    _upload(ex, arrays, tracks)
    want, states, next_id = [], [], 1000
    for f in range(n):
        want.append(_five_calls(ca, ex, st, n, f, room.W2C, None, room.flags, ca.COMMIT_ADD_STAGED, next_id, room.meas[f], "loop, "))
        next_id = want[-1][2]
        states.append(_state(ex))
    ex.clear_retired()
    _upload(ex, arrays, tracks)
    next_id, totals = 1000, np.zeros(3, int)
    for f in range(n):
        c, m, next_id = _step(ca, ex, st, f, room.W2C, None, room.flags, ca.COMMIT_ADD_STAGED, next_id, want[f], "loop, ")
        assert c["flags"] == ca.COMMIT_DONE, f"step {f} is refused"
        _same_state(_state(ex), states[f], f"loop, after step {f}")
        totals += [int(m["n_promoted"]), int(m["n_dropped"]), int(m["n_lost"])]
    print(f"over the loop: {totals[0]} promoted, {totals[1]} dropped, {totals[2]} lost")
    assert np.all(totals >= 1)
    (_, Tr), (_, LT) = _state(ex)
    assert 901 in LT["id"].tolist() and 900 not in Tr["id"].tolist() + LT["id"].tolist() and len(LT) == totals[2]
    ex.clear_retired()
    room.restore()


# ---- 4. every outcome of the table ----------------------------------------------------------------------------------------------
def test_a_refused_commit_changes_nothing(room):  # noqa: F811
    import cape_amd as ca

    f = max(range(room.n), key=lambda g: _stageable(ca, room, g))
    assert _stageable(ca, room, f) >= 3
    (arrays, tracks), _ = _random_map(ca, room, ca.MAP_MAX_PLANES - 2, np.random.default_rng(41))
    print()
    c, m, after, before = _both_routes(ca, room, f, arrays, tracks, ca.COMMIT_ADD_STAGED, 70, "1 022 planes + 3, ", twins=False)
    assert c["flags"] == ca.COMMIT_CAPACITY and c["next_id"] == 70 and not m.tobytes().strip(b"\0")
    _same_state(after, before, "a refused commit")
    room.ex.clear_retired()
    room.restore()


def test_done_and_nothing(room):  # noqa: F811
    import cape_amd as ca

    tracks = room.tracks.copy()
    tracks["flags"], tracks["successive_matched"], tracks["failed_tracking"] = 0, 0, 0
    print()
    c, m, after, before = _both_routes(ca, room, room.source, room.arrays, tracks, 0, 5, "nothing due, ")
    assert c["flags"] == ca.COMMIT_DONE and m["flags"] == ca.MAINTAIN_NOTHING and c["n_updated"] >= 1
    assert after[0][1].tobytes() != before[0][1].tobytes() and len(after[1][1]) == 0  # the committed tracks, the empty log
    room.restore()


def test_done_and_done(room):  # noqa: F811
    import cape_amd as ca

    arrays, tracks = _loop_map(ca, room)
    print()
    c, m, after, _ = _both_routes(ca, room, 0, arrays, tracks, ca.COMMIT_ADD_STAGED, 5, "due, ")
    assert c["flags"] == ca.COMMIT_DONE and m["flags"] == ca.MAINTAIN_DONE and m["n_lost"] >= 1 and m["n_dropped"] >= 1
    assert 901 in after[1][1]["id"].tolist() and 900 not in after[0][1]["id"].tolist() and m["n_planes"] < c["n_planes"]
    room.ex.clear_retired()
    room.restore()


def test_done_and_a_full_log(room):  # noqa: F811
    """the log pre-filled to its cap, one local plane at failed_tracking 9 that the frame misses: the committed map, the log untouched"""
    import cape_amd as ca

    ex, st = room.ex, room.st
    far, far_tracks = _wall_copies(ca, room, 1, np.random.default_rng(13), far=True)
    far_tracks["flags"], far_tracks["successive_matched"], far_tracks["failed_tracking"], far_tracks["id"] = 0, 2, 9, 901
    arrays, tracks = MC.arrays_of(ca, MC.entries_of(room.arrays, room.tracks) + MC.entries_of(far, far_tracks))
    tracks["flags"], tracks["successive_matched"] = 0, 0  # (nothing else is due)
    tracks["failed_tracking"][:-1] = 0
    print()
    c, m, after, before = _both_routes(ca, room, room.source, arrays, tracks, 0, 5, "the full log, ",
                                       fill=lambda: _fill_log(ca, ex, st, ca.MAP_RETIRED_MAX_PLANES))
    assert c["flags"] == ca.COMMIT_DONE and m["flags"] == ca.MAINTAIN_LOG_FULL and m["n_lost"] == 1
    assert m["n_retired"] == ca.MAP_RETIRED_MAX_PLANES and len(after[0][1]) == len(tracks) and after[0][1]["failed_tracking"][-1] == 10
    MC.same_map(after[1], before[1], "the log of a refused maintenance")
    ex.clear_retired()
    room.restore()


# ---- 5. counts that only the device knows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("committed", [257, 1024])
def test_the_committed_count_crosses_a_plan_boundary(room, committed):  # noqa: F811
    """far wall copies, every fifth with holes, of every class, and the k stageable planes of a frame appended behind them: the old map
    ends below a boundary of the maintenance plan (256 planes per wave, 1 024 per workgroup: 257 - k <= 255, 1 024 - k <= 1 021), the
    committed map on or beyond it.  Only the commit's header in device memory says so.  The appended planes are staged and never due;
    the classes that are due lie before them, on both sides of every earlier wave boundary.  The copy grid is launched for old + 128
    planes where that is below 1 024: more workgroups than the committed map has planes."""
    import cape_amd as ca

    f = max(range(room.n), key=lambda g: _stageable(ca, room, g))
    k = _stageable(ca, room, f)
    assert k >= 3
    old = committed - k
    (arrays, tracks), classes = _random_map(ca, room, old, np.random.default_rng(50 + committed))
    assert np.any(arrays[0]["ring_count"] > 1)
    print()
    c, m, after, _ = _both_routes(ca, room, f, arrays, tracks, ca.COMMIT_ADD_STAGED, 9000, f"{old} -> {committed} planes, ", twins=False)
    assert c["flags"] == ca.COMMIT_DONE and (c["n_planes"], c["n_appended"]) == (committed, k)
    assert m["flags"] == ca.MAINTAIN_DONE and min(m["n_promoted"], m["n_dropped"], m["n_lost"]) >= 1
    assert m["n_local"] + m["n_staged"] + m["n_dropped"] + m["n_lost"] == committed  # every committed plane was decided
    assert after[0][1]["id"][-k:].tolist() == list(range(9000, 9000 + k))           # the appended ones are the list's tail
    if old + 128 < ca.MAP_MAX_PLANES:
        assert committed < old + 128
    room.ex.clear_retired()
    room.restore()


# ---- 7. skip words --------------------------------------------------------------------------------------------------------------
def test_a_skip_word_hides_a_matched_map_plane(room):  # noqa: F811
    import cape_amd as ca

    f = room.source
    hidden = int(np.flatnonzero(room.results[f]["result"] & ca.MAP_RESULT_UPDATED)[0])
    words = np.zeros((len(room.arrays[0]) + 31) // 32, np.uint32)
    words[hidden >> 5] = 1 << (hidden & 31)
    print()
    c, m, after, _ = _both_routes(ca, room, f, room.arrays, room.tracks, 0, 5, f"plane {hidden} hidden, ", skip_f=words)
    assert c["flags"] == ca.COMMIT_DONE
    track = after[0][1][after[0][1]["id"] == room.tracks[hidden]["id"]]
    assert len(track) == 1 and not track[0]["result"] & ca.MAP_RESULT_UPDATED  # (unhidden it is updated: room.results, above)
    room.ex.clear_retired()
    room.restore()


# ---- 8. bookkeeping -------------------------------------------------------------------------------------------------------------
def test_bookkeeping(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    ex.clear_retired()
    room.restore()
    T = room.W2C[0]
    for args in ((-1, T, None, 0, 0), (0, T, None, ca.MATCH_MAP_AREAS, 0), (0, T, None, ca.MATCH_MAP_DEVICE_SKIP, 0), (0, T, None, 1 << 20, 0),
                 (0, T, None, 0, 2)):
        with pytest.raises(ca.CapeError, match="cape_map_step " + INV):
            ex.map_step(*args, 0, st)
    out = np.zeros(1, ca.MAP_STEP_RESULT_DTYPE)
    assert ex.L.cape_map_step(ex.h, 0, None, None, 0, 0, C.byref(C.c_uint64(0)), out.ctypes.data_as(C.c_void_p), C.c_void_p(st)) == -1
    with pytest.raises(ca.CapeError, match="cape_map_step " + CAP):
        ex.map_step(n, T, None, room.flags, 0, 0, st)  # beyond the polygons and the measurements
    ex.upload_map(room.arrays)  # a new map discards the tracks: none are current
    with pytest.raises(ca.CapeError, match="cape_map_step " + CAP):
        ex.map_step(0, T, None, room.flags, 0, 0, st)
    # after a step -- here one whose commit is refused: the map is full -- the batch-wide results are not current
    full, full_tracks = _wall_copies(ca, room, ca.MAP_MAX_PLANES, np.random.default_rng(8), far=True)
    f = room.source
    for arrays, tracks, flags in ((full, full_tracks, ca.COMMIT_CAPACITY), (room.arrays, room.tracks, ca.COMMIT_DONE)):
        _upload(ex, arrays, tracks)
        ex.match_map_wide(n, room.W2C, None, room.flags, st)
        ex.map_kalman(n, st)
        ex.map_union_cut(n, st)
        before = _state(ex)
        result, nid = ex.map_step(f, room.W2C[f], None, room.flags, ca.COMMIT_ADD_STAGED, 10, st)
        print(f"\nbookkeeping: commit {int(result['commit']['flags']):#x}, maintain {int(result['maintain']['flags']):#x}")
        assert result["commit"]["flags"] == flags
        with pytest.raises(ca.CapeError, match="cape_copy_map_kalman " + CAP):
            ex.map_kalman_rows(1)
        with pytest.raises(ca.CapeError, match="cape_copy_map_union " + CAP):
            ex.map_union_rows(1)
        with pytest.raises(ca.CapeError, match="cape_copy_map_matches_wide " + CAP):
            ex.map_matches_wide(1)
        with pytest.raises(ca.CapeError, match="cape_map_kalman " + CAP):
            ex.map_kalman(n, st)
        with pytest.raises(ca.CapeError, match="cape_map_commit " + CAP):
            ex.map_commit(f, 0, nid, st)
        if flags == ca.COMMIT_CAPACITY:
            _same_state(_state(ex), before, "a refused step")
            assert nid == 10
    last = result["maintain"] if result["maintain"]["flags"] & ca.MAINTAIN_DONE else result["commit"]
    assert ex.map_info() == (int(last["n_planes"]), int(last["n_rings"]), int(last["n_vertices"]))
    assert ex.retired_info()[0] == int(result["maintain"]["n_retired"])
    # the measurement rows are still valid and the map and tracks are the step's: a five-call sequence gives the twins' bytes
    g = (f + 1) % n
    commit, maintain, _ = _five_calls(ca, ex, st, n, g, room.W2C, None, room.flags, ca.COMMIT_ADD_STAGED, nid, room.meas[g], "after a step, ")
    assert commit["flags"] == ca.COMMIT_DONE
    ex.clear_retired()
    room.restore()

"""cape_map_step_visible: cape_map_step with the frame's skip words decided on the device in the same call -- against the four-call
route it stands for, on a second upload of the same map, tracks and log:

    moving = the CAPE_MAP_TRACK_MOVING bits of the device tracks;  cape_map_visibility(1, T, moving);
    cape_copy_map_visibility(1, words, &und);  cape_map_step(f, T, words, match_flags, commit_flags, &id, &r).

Everything is compared byte for byte (tobytes()): the step's two headers, next_id, the map, the tracks with their ids and the retired
log; the words of cape_map_step_skip_words bit for bit with the route's AND with the host twin cape_host_map_visibility on the map as it
was before the step; n_undecided with the route's.  No tolerance anywhere.

Every test prints its figures before it asserts (`pytest -s`)."""
import ctypes as C
import math

import numpy as np
import pytest

import map_maintain_cases as MC
from test_gpu_map_commit import _wall_copies
from test_gpu_map_kalman import room  # noqa: F401  (the eight room frames after the four calls)
from test_gpu_map_maintain import _fill_log, _random_map, _upload
from test_gpu_map_match import _lift
from test_gpu_map_step import _five_calls, _loop_map, _same_state, _stageable, _state
from test_map_visibility_host import GON_CASES, H, HAND_CASES, W, _box, _fronto, bits

pytestmark = pytest.mark.gpu

INV, CAP = r"failed \(-1\)", r"failed \(-4\)"


def _intr():
    from cape_amd import synth

    return synth.DEFAULT_INTRINSICS


def _moving_words(ca, tracks):
    """step 1 of the route: bit j set where track j has MAP_TRACK_MOVING"""
    words = np.zeros((len(tracks) + 31) // 32, np.uint32)
    for j in np.flatnonzero(tracks["flags"] & ca.MAP_TRACK_MOVING):
        words[j >> 5] |= np.uint32(1 << (int(j) & 31))
    return words


def _twin_words(ca, arrays, T, moving, intr):
    return ca.host_map_visibility(arrays, T, W, H, intr["fx"], intr["fy"], intr["cx"], intr["cy"], moving if len(moving) else None)


def _four_calls(ca, ex, st, f, T, match_flags, commit_flags, next_id):
    """the route the call stands for.  Returns (step result, next_id, words, n_undecided)."""
    tracks = ex.download_map()[1]
    moving = _moving_words(ca, tracks)
    ex.map_visibility(1, T[None], moving if len(moving) else None, st)
    words, undecided = ex.map_visibility_words(1)
    result, nid = ex.map_step(f, T, words[0] if words.shape[1] else None, match_flags, commit_flags, next_id, st)
    return result, nid, words[0].copy(), undecided


def _visible_step(ca, ex, st, f, T, match_flags, commit_flags, next_id, want, intr, what):
    """the call, the reader and the twin on the map before the step, against `want` = _four_calls' result on another upload"""
    before, tracks = ex.download_map()
    moving = _moving_words(ca, tracks)
    twin = _twin_words(ca, before, T, moving, intr)
    result, nid = ex.map_step_visible(f, T, match_flags, commit_flags, next_id, st)
    words, n_map = ex.map_step_skip_words()
    c, m = result["step"]["commit"], result["step"]["maintain"]
    print(f"{what}step_visible({f}): map of {int(result['n_map'])} planes, {int(result['n_moving'])} moving, {int(result['n_listed'])} listed, "
          f"{int(result['n_undecided'])} undecided, {sum(bits(words, n_map))} skipped; commit {int(c['flags']):#x}, {int(c['n_planes'])} planes, updated "
          f"{int(c['n_updated'])}, appended {int(c['n_appended'])}; maintain {int(m['flags']):#x}, {int(m['n_planes'])} planes; next id {nid}")
    assert n_map == len(tracks) == result["n_map"] and len(words) == (n_map + 31) // 32
    assert np.array_equal(words, want[2]), f"{what}planes {[j for j in range(n_map) if bits(words, n_map)[j] != bits(want[2], n_map)[j]]} differ from the route's words"
    assert np.array_equal(words, twin), f"{what}planes {[j for j in range(n_map) if bits(words, n_map)[j] != bits(twin, n_map)[j]]} differ from the twin's words"
    if n_map % 32:
        assert int(words[-1]) >> (n_map % 32) == 0  # the bits beyond n_map
    assert result["n_undecided"] == want[3] and result["pad"] == 0
    assert result["n_moving"] == int(np.count_nonzero(tracks["flags"] & ca.MAP_TRACK_MOVING))
    visible = n_map - sum(bits(words, n_map))
    assert visible <= result["n_listed"] <= n_map - result["n_moving"]  # (only a listed plane can turn out visible)
    assert result["step"].tobytes() == want[0].tobytes(), f"{what}step result {result['step']} != {want[0]}"
    assert nid == want[1]
    last = m if m["flags"] & ca.MAINTAIN_DONE else c
    assert ex.map_info() == (int(last["n_planes"]), int(last["n_rings"]), int(last["n_vertices"]))
    return result, nid, words


def _both_routes(ca, room, f, arrays, tracks, commit_flags, next_id, what, T=None, fill=None, ex=None, st=None, flags=None, intr=None):  # noqa: F811
    """frame f by the four calls and by cape_map_step_visible, each from its own upload of (arrays, tracks) and the log `fill` leaves
    (None: the cleared log).  Returns (result, words, the state after, the state before)."""
    ex, st = (room.ex, room.st) if ex is None else (ex, st)
    T = room.W2C[f] if T is None else T
    flags = room.flags if flags is None else flags
    intr = _intr() if intr is None else intr
    states = []
    for route in ("four", "visible"):
        if fill is None:
            ex.clear_retired()
        elif route == "four":
            fill()  # (a route that leaves the log as it was needs no second filling: asserted below)
        _upload(ex, arrays, tracks)
        before = _state(ex)
        if route == "four":
            want = _four_calls(ca, ex, st, f, T, flags, commit_flags, next_id)
            log_four = before[1]
        else:
            if fill is not None:
                MC.same_map(before[1], log_four, what + "the log before the second route")
            result, _, words = _visible_step(ca, ex, st, f, T, flags, commit_flags, next_id, want, intr, what)
        states.append(_state(ex))
    _same_state(states[1], states[0], what + "after the step")
    return result, words, states[1], before


def _added(ca, room, planes, flags, first_id):  # noqa: F811
    """entries for plane tuples, local tracks with the covariance of the room's first track"""
    tracks = np.zeros(len(planes), ca.MAP_TRACK_DTYPE)
    tracks["covariance"] = room.tracks[0]["covariance"]
    tracks["flags"] = flags
    tracks["id"] = first_id + np.arange(len(planes))
    return MC.entries_of(ca.pack_map(planes), tracks)


def _copy_of(entry, flags, sm, ft, new_id):
    e = dict(plane=entry["plane"].copy(), rings=[r.copy() for r in entry["rings"]], track=entry["track"].copy())
    e["track"]["flags"], e["track"]["successive_matched"], e["track"]["failed_tracking"], e["track"]["id"] = flags, sm, ft, new_id
    return e


def _matched_plane(ca, room, f):  # noqa: F811
    """a map plane of the room that frame f updates (None: the frame updates none)"""
    hit = np.flatnonzero(room.results[f]["result"] & ca.MAP_RESULT_UPDATED)
    return int(hit[0]) if len(hit) else None


def _pose_with_a_vertex_at_depth_zero(T, center):
    """the pose with its last translation nudged (by rounding errors' size) so that the camera Z of `center` is exactly 0 in the
    kernels' and the twin's order of operations: ((T20 c0 + T21 c1) + T22 c2) + T23"""
    T = T.copy()
    T[2, 3] = -((T[2, 0] * center[0] + T[2, 1] * center[1]) + T[2, 2] * center[2])
    assert ((T[2, 0] * center[0] + T[2, 1] * center[1]) + T[2, 2] * center[2]) + T[2, 3] == 0.0
    return T


# ---- 1. each room frame alone, with planes outside the view and a moving copy -----------------------------------------------------
def test_each_room_frame_alone(room):  # noqa: F811
    """the room's planes, then four added ones per frame, built in that frame's camera and lifted to the world: a wall beside the
    screen, one behind the camera, a triangle through the optical centre whose first vertex has camera Z == 0 exactly (a non-finite
    screen coordinate) and a copy of a map plane the frame updates, flagged MOVING"""
    import cape_amd as ca

    intr = _intr()
    base_tracks = room.tracks.copy()
    base_tracks["flags"] &= ~np.uint32(ca.MAP_TRACK_MOVING)
    base = MC.entries_of(room.arrays, base_tracks)
    n_room, with_copy = len(base), 0
    print()
    for f in range(room.n):
        R, o = room.c2w[f]
        beside = _lift(_fronto(_box(800, 1000, 100, 300), intr=intr), R, o)
        behind = _lift(_fronto(_box(200, 400, 150, 300), intr=intr, z=-1000.0), R, o)
        through = _lift((np.array([0.0, -1.0, 0.0]), 0.0, np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]), np.zeros(3),
                         np.array([[0.0, 0.0], [100.0, 500.0], [-100.0, 500.0]]), 0.0), R, o)
        hit = _matched_plane(ca, room, f)
        copy = _copy_of(base[hit if hit is not None else 0], ca.MAP_TRACK_MOVING, 0, 0, 703)
        arrays, tracks = MC.arrays_of(ca, base + _added(ca, room, [beside, behind, through], 0, 700) + [copy])
        T = _pose_with_a_vertex_at_depth_zero(room.W2C[f], arrays[0][n_room + 2]["center"])
        # the twin first: the case decides something
        twin = bits(_twin_words(ca, arrays, T, _moving_words(ca, tracks), intr), len(tracks))
        print(f"frame {f}: the twin skips {[j for j, s in enumerate(twin) if s]} of {len(twin)} planes (the room's: 0 .. {n_room - 1})")
        assert twin[n_room] and twin[n_room + 2] and twin[n_room + 3]  # beside the screen; the non-finite coordinate; moving
        assert not all(twin[:n_room]), "no room plane is visible"
        result, words, after, _ = _both_routes(ca, room, f, arrays, tracks, ca.COMMIT_ADD_STAGED, 1000 + f, f"frame {f}, ", T=T)
        c = result["step"]["commit"]
        assert c["flags"] == ca.COMMIT_DONE and c["frame"] == f and result["n_moving"] == 1
        track = after[0][1][after[0][1]["id"] == 703]
        assert len(track) == 1 and not track[0]["result"] & ca.MAP_RESULT_MATCHED  # the moving copy takes no match
        if hit is not None and not twin[hit]:
            original = after[0][1][after[0][1]["id"] == room.tracks[hit]["id"]]
            assert len(original) == 1 and original[0]["result"] & ca.MAP_RESULT_UPDATED  # ... the plane it copies does
            with_copy += 1
    assert with_copy >= 1
    room.ex.clear_retired()
    room.restore()


# ---- 2. random maps at the widths of the classify kernel --------------------------------------------------------------------------
def _ngon(centre, radius, k):
    a = 0.1 + np.linspace(0, 2 * math.pi, k, endpoint=False)
    return centre + radius * np.stack([np.cos(a), np.sin(a)], 1)


# a workgroup decides 64 planes and writes two words (63 / 64 / 65, 255 / 256 / 257), a word holds 32 (31 / 32 / 33), a wave takes every
# eighth plane of its group; 1 024 is the largest map
@pytest.mark.parametrize("size", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1024])
def test_random_maps(room, size):  # noqa: F811
    """_random_map's far wall copies (holes in every fifth, every class of track drawn per plane, MOVING in some), with outer rings
    of 3, 64, 65 and 512 vertices among them (the edges of the intersection tiers, and more vertices than a wave has lanes) and every
    fourth ring moved 60 m along its plane, off the screen"""
    import cape_amd as ca

    (arrays, tracks), _ = _random_map(ca, room, size, np.random.default_rng(60 + size))
    entries = MC.entries_of(arrays, tracks)
    counts = set()
    for j, e in enumerate(entries):
        if len(e["rings"]) > 1:
            continue  # (a plane with holes keeps its rings)
        k = {3: 3, 8: 64, 11: 65, 23: 512}.get(j % 29)
        if k:
            ring = e["rings"][0]
            e["rings"][0] = _ngon(ring.mean(axis=0), 0.5 * float(np.ptp(ring, axis=0).max()), k)
            counts.add(k)
        if j % 4 == 1:
            e["rings"][0] = e["rings"][0] + np.array([60000.0, 0.0])
    arrays, tracks = MC.arrays_of(ca, entries)
    f, T, intr = room.source, room.W2C[room.source], _intr()
    twin = bits(_twin_words(ca, arrays, T, _moving_words(ca, tracks), intr), size)
    print(f"\n{size} planes: the twin skips {sum(twin)}, {int(np.count_nonzero(tracks['flags'] & ca.MAP_TRACK_MOVING))} are moving, "
          f"{int(np.count_nonzero(arrays[0]['ring_count'] > 1))} have holes, outer rings of {sorted(counts)} vertices among them")
    if size >= 31:
        assert counts == {3, 64, 65, 512} and 0 < sum(twin) < size and np.any(arrays[0]["ring_count"] > 1)
        assert np.any(tracks["flags"] & ca.MAP_TRACK_MOVING)
    add = ca.COMMIT_ADD_STAGED if size + 128 <= ca.MAP_MAX_PLANES else 0
    result, words, _, _ = _both_routes(ca, room, f, arrays, tracks, add, 9000, f"{size} planes, ")
    assert result["step"]["commit"]["flags"] == ca.COMMIT_DONE and result["n_map"] == size
    room.ex.clear_retired()
    room.restore()


# ---- 3. rings that touch the rectangle exactly ------------------------------------------------------------------------------------
def test_rings_that_touch_the_rectangle_exactly():
    """fx = fy = 512, the identity pose and map planes at Z = 512: x = -319 mm lands on u == 1.0 and x = 319 on u == 639.0 without
    rounding (tests/test_gpu_map_visibility.py's squares) -- and, under the same pose, the hand-built planes and the n-gons of the
    visibility cases, the two with a vertex at Z == 0 among them -- as the map of a step"""
    import torch
    import cape_amd as ca
    from cape_amd import Extractor, synth_gpu
    from test_gpu_map_measure import _pose_covariances

    intr = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)

    def square(x0, x1):
        ring = np.array([[x0, -50.0], [x1, -50.0], [x1, 50.0], [x0, 50.0]])
        return (np.array([0.0, 0.0, 1.0]), -512.0, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 512.0]), ring, [])

    planes = [square(-400.0, -319.0), square(-400.0, np.nextafter(-319.0, 0.0)), square(319.0, 400.0), square(np.nextafter(319.0, 0.0), 400.0),
              square(-100.0, 100.0)] + [c[1] for c in HAND_CASES + GON_CASES]
    arrays = ca.pack_map(planes)
    tracks = np.zeros(len(planes), ca.MAP_TRACK_DTYPE)
    tracks["covariance"] = np.eye(4)
    tracks["id"] = 100 + np.arange(len(planes))
    T = np.eye(4)
    twin = bits(_twin_words(ca, arrays, T, _moving_words(ca, tracks), intr), len(planes))
    print("\ntwin:", twin)
    assert twin[0] and twin[2] and not twin[4]  # max_u == 1.0 / min_u == 639.0: no area in common (the full computation)
    for j, (name, _, visible, _) in enumerate(HAND_CASES):
        if "Z = 0" in name or "optical centre" in name:
            assert twin[5 + j], name  # (a non-finite screen coordinate under the identity pose, whatever the intrinsics)
    dev = synth_gpu.stream("room", 11, 1, start=20, device="cuda", chunk=1).contiguous()
    ex = Extractor(W, H, cylinders=False, max_batch=1, **intr)
    st = torch.cuda.current_stream().cuda_stream
    ex.extract_device(dev.data_ptr(), 1, st)
    ex.build_polygons(1, st)
    ex.map_measure(1, None, _pose_covariances(np.random.default_rng(4), 1), st)
    result, words, _, _ = _both_routes(ca, None, 0, arrays, tracks, ca.COMMIT_ADD_STAGED, 300, "exact touches, ", T=T, ex=ex, st=st,
                                       flags=ca.MATCH_ALLOW_INDEX0, intr=intr)
    assert result["n_undecided"] == 0 and result["n_moving"] == 0 and bits(words, len(planes)) == twin
    ex.clear_retired()
    ex.close()


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------
def test_a_loop_of_eight_steps_without_an_upload(room):  # noqa: F811
    """test_gpu_map_step's loop map, and: for f = 0 .. 6 a small wall at the left edge of frame f's screen (u from 3 to 9 at 2 m), which
    the camera's turn takes off the screen of frame f + 1 -- the words change from frame to frame; a staged copy of a plane frame 1
    updates, flagged MOVING with successive_matched 8: promoted behind step 0, skipped in step 1 and after."""
    import cape_amd as ca

    ex, n, st, intr = room.ex, room.n, room.st, _intr()
    arrays, tracks = _loop_map(ca, room)
    entries = MC.entries_of(arrays, tracks)
    n_base = len(entries)
    edge = [_lift(_fronto(_box(3, 9, 200, 280), intr=intr, z=2000.0), *room.c2w[f]) for f in range(n - 1)]
    hit = _matched_plane(ca, room, 1)
    copy = _copy_of(entries[hit if hit is not None else 0], ca.MAP_TRACK_STAGED | ca.MAP_TRACK_MOVING, 8, 0, 950)
    arrays, tracks = MC.arrays_of(ca, entries + _added(ca, room, edge, 0, 800) + [copy])
    # the twin first, on the map as uploaded: plane n_base + f is visible at f and hidden at f + 1
    moving = _moving_words(ca, tracks)
    twin = [bits(_twin_words(ca, arrays, room.W2C[f], moving, intr), len(tracks)) for f in range(n)]
    for f in range(n - 1):
        assert not twin[f][n_base + f] and twin[f + 1][n_base + f], f"the wall at the edge of frame {f}"
        assert twin[f] != twin[f + 1]
    print()
    ex.clear_retired()
    _upload(ex, arrays, tracks)
    want, states, next_id = [], [], 1000
    for f in range(n):
        want.append(_four_calls(ca, ex, st, f, room.W2C[f], room.flags, ca.COMMIT_ADD_STAGED, next_id))
        next_id = want[-1][1]
        states.append(_state(ex))
    ex.clear_retired()
    _upload(ex, arrays, tracks)
    next_id, totals, all_words = 1000, np.zeros(4, int), []
    for f in range(n):
        ids_before = ex.download_map()[1]["id"].tolist()
        result, next_id, words = _visible_step(ca, ex, st, f, room.W2C[f], room.flags, ca.COMMIT_ADD_STAGED, next_id, want[f], intr, "loop, ")
        c, m = result["step"]["commit"], result["step"]["maintain"]
        assert c["flags"] == ca.COMMIT_DONE, f"step {f} is refused"
        _same_state(_state(ex), states[f], f"loop, after step {f}")
        totals += [int(c["n_appended"]), int(m["n_promoted"]), int(m["n_dropped"]), int(m["n_lost"])]
        skipped = dict(zip(ids_before, bits(words, len(ids_before))))
        all_words.append(skipped)
        assert skipped[950] and result["n_moving"] >= 1  # the moving copy: staged in step 0, local from then on
        if f < n - 1:
            assert not skipped[800 + f]
        if f > 0:
            assert skipped[800 + f - 1]  # visible in the step before, hidden now: words of the step before would not do
        track = [t for t in _state(ex)[0][1] if t["id"] == 950]
        assert len(track) == 1 and not track[0]["result"] & ca.MAP_RESULT_MATCHED
        if f == 0:
            assert track[0]["flags"] == ca.MAP_TRACK_MOVING  # promoted, MOVING kept
    print(f"over the loop: {totals[0]} appended, {totals[1]} promoted, {totals[2]} dropped, {totals[3]} lost")
    assert np.all(totals >= 1)
    ex.clear_retired()
    room.restore()


# ---- 5. every outcome of the step's table -----------------------------------------------------------------------------------------
def test_a_refused_commit_changes_nothing_and_the_words_are_readable(room):  # noqa: F811
    import cape_amd as ca

    f = max(range(room.n), key=lambda g: _stageable(ca, room, g))
    assert _stageable(ca, room, f) >= 3
    (arrays, tracks), _ = _random_map(ca, room, ca.MAP_MAX_PLANES - 2, np.random.default_rng(41))
    print()
    result, words, after, before = _both_routes(ca, room, f, arrays, tracks, ca.COMMIT_ADD_STAGED, 70, "1 022 planes + 3, ")
    c, m = result["step"]["commit"], result["step"]["maintain"]
    assert c["flags"] == ca.COMMIT_CAPACITY and c["next_id"] == 70 and not m.tobytes().strip(b"\0")
    _same_state(after, before, "a refused commit")
    again, n_map = room.ex.map_step_skip_words()
    assert n_map == ca.MAP_MAX_PLANES - 2 and np.array_equal(again, words) and result["n_moving"] >= 1
    room.ex.clear_retired()
    room.restore()


def test_done_and_nothing(room):  # noqa: F811
    import cape_amd as ca

    tracks = room.tracks.copy()
    tracks["flags"], tracks["successive_matched"], tracks["failed_tracking"] = 0, 0, 0
    print()
    result, _, after, before = _both_routes(ca, room, room.source, room.arrays, tracks, 0, 5, "nothing due, ")
    c, m = result["step"]["commit"], result["step"]["maintain"]
    assert c["flags"] == ca.COMMIT_DONE and m["flags"] == ca.MAINTAIN_NOTHING and c["n_updated"] >= 1
    assert after[0][1].tobytes() != before[0][1].tobytes() and len(after[1][1]) == 0  # the committed tracks, the empty log
    room.restore()


def test_done_and_done(room):  # noqa: F811
    import cape_amd as ca

    arrays, tracks = _loop_map(ca, room)
    print()
    result, _, after, _ = _both_routes(ca, room, 0, arrays, tracks, ca.COMMIT_ADD_STAGED, 5, "due, ")
    c, m = result["step"]["commit"], result["step"]["maintain"]
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
    result, _, after, before = _both_routes(ca, room, room.source, arrays, tracks, 0, 5, "the full log, ",
                                            fill=lambda: _fill_log(ca, ex, st, ca.MAP_RETIRED_MAX_PLANES))
    c, m = result["step"]["commit"], result["step"]["maintain"]
    assert c["flags"] == ca.COMMIT_DONE and m["flags"] == ca.MAINTAIN_LOG_FULL and m["n_lost"] == 1
    assert m["n_retired"] == ca.MAP_RETIRED_MAX_PLANES and len(after[0][1]) == len(tracks) and after[0][1]["failed_tracking"][-1] == 10
    MC.same_map(after[1], before[1], "the log of a refused maintenance")
    ex.clear_retired()
    room.restore()


# ---- 6. the empty map -------------------------------------------------------------------------------------------------------------
def test_the_empty_map(room):  # noqa: F811
    import cape_amd as ca

    f = max(range(room.n), key=lambda g: _stageable(ca, room, g))
    empty = (ca.pack_map([]), np.zeros(0, ca.MAP_TRACK_DTYPE))
    print()
    result, words, after, _ = _both_routes(ca, room, f, *empty, ca.COMMIT_ADD_STAGED, 300, "the empty map, ")
    c = result["step"]["commit"]
    assert (result["n_map"], result["n_moving"], result["n_listed"], result["n_undecided"]) == (0, 0, 0, 0) and len(words) == 0
    assert c["flags"] == ca.COMMIT_DONE and c["n_appended"] == _stageable(ca, room, f) >= 1 and len(after[0][1]) == c["n_appended"]
    n_map = C.c_int32(-1)
    assert room.ex.L.cape_map_step_skip_words(room.ex.h, None, 0, C.byref(n_map)) == 0 and n_map.value == 0  # no words: none are asked for
    # ... and the step after it decides the words of the planes this one appended
    g = (f + 1) % room.n
    want = None
    for route in ("four", "visible"):
        room.ex.clear_retired()
        _upload(room.ex, *after[0])
        if route == "four":
            want = _four_calls(ca, room.ex, room.st, g, room.W2C[g], room.flags, ca.COMMIT_ADD_STAGED, 400)
            state = _state(room.ex)
        else:
            result, _, _ = _visible_step(ca, room.ex, room.st, g, room.W2C[g], room.flags, ca.COMMIT_ADD_STAGED, 400, want, _intr(), "behind it, ")
            _same_state(_state(room.ex), state, "behind the empty map")
    assert result["n_map"] == c["n_appended"]
    room.ex.clear_retired()
    room.restore()


# ---- 7. bookkeeping and errors ----------------------------------------------------------------------------------------------------
def test_bookkeeping(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    ex.clear_retired()
    room.restore()  # (an upload: no step's words are current)
    T = room.W2C[0]
    with pytest.raises(ca.CapeError, match="cape_map_step_skip_words " + CAP):
        ex.map_step_skip_words()
    for args in ((-1, T, 0, 0), (0, T, ca.MATCH_MAP_AREAS, 0), (0, T, ca.MATCH_MAP_DEVICE_SKIP, 0), (0, T, 1 << 20, 0), (0, T, 0, 2)):
        with pytest.raises(ca.CapeError, match="cape_map_step_visible " + INV):
            ex.map_step_visible(*args, 0, st)
    with pytest.raises(ca.CapeError, match="cape_map_step " + INV):  # the plain step still refuses the flag
        ex.map_step(0, T, None, ca.MATCH_MAP_DEVICE_SKIP, 0, 0, st)
    with pytest.raises(ca.CapeError, match="cape_map_step_visible " + CAP):
        ex.map_step_visible(n, T, room.flags, 0, 0, st)  # beyond the polygons and the measurements
    ex.upload_map(room.arrays)  # a new map discards the tracks: none are current
    with pytest.raises(ca.CapeError, match="cape_map_step_visible " + CAP):
        ex.map_step_visible(0, T, room.flags, 0, 0, st)
    with pytest.raises(ca.CapeError, match="cape_map_step_skip_words " + CAP):  # (a refused call decides no words)
        ex.map_step_skip_words()
    # the words of cape_map_visibility are another buffer: a step leaves them as cape_map_step does -- readable and unchanged behind
    # a refused commit, refused once the commit is DONE (they were the old map's)
    full, full_tracks = _wall_copies(ca, room, ca.MAP_MAX_PLANES, np.random.default_rng(8), far=True)
    f = room.source
    for arrays, tracks, flags in ((full, full_tracks, ca.COMMIT_CAPACITY), (room.arrays, room.tracks, ca.COMMIT_DONE)):
        _upload(ex, arrays, tracks)
        ex.map_visibility(2, room.W2C[:2], None, st)
        batch_words, _ = ex.map_visibility_words(2)
        ex.match_map_wide(n, room.W2C, None, room.flags, st)
        ex.map_kalman(n, st)
        ex.map_union_cut(n, st)
        before = _state(ex)
        result, nid = ex.map_step_visible(f, room.W2C[f], room.flags, ca.COMMIT_ADD_STAGED, 10, st)
        print(f"\nbookkeeping: commit {int(result['step']['commit']['flags']):#x}, maintain {int(result['step']['maintain']['flags']):#x}")
        assert result["step"]["commit"]["flags"] == flags and result["n_map"] == len(tracks)
        words, n_map = ex.map_step_skip_words()
        assert n_map == len(tracks) and len(words) == (n_map + 31) // 32
        # the reader with too small a capacity: CAPACITY, n_map still reported, nothing written
        short, got = np.full(len(words), 0xFFFFFFFF, np.uint32), C.c_int32(-1)
        assert ex.L.cape_map_step_skip_words(ex.h, short.ctypes.data_as(C.c_void_p), len(words) - 1, C.byref(got)) == -4
        assert got.value == n_map and np.all(short == 0xFFFFFFFF)
        assert ex.L.cape_map_step_skip_words(ex.h, None, len(words), None) == -1  # NULL words with n_map > 0
        for reader, name in ((ex.map_kalman_rows, "cape_copy_map_kalman"), (ex.map_union_rows, "cape_copy_map_union"),
                             (ex.map_matches_wide, "cape_copy_map_matches_wide")):
            with pytest.raises(ca.CapeError, match=name + " " + CAP):
                reader(1)
        if flags == ca.COMMIT_CAPACITY:
            _same_state(_state(ex), before, "a refused step")
            assert nid == 10
            again, _ = ex.map_visibility_words(2)
            assert np.array_equal(again, batch_words)
        else:
            with pytest.raises(ca.CapeError, match="cape_copy_map_visibility " + CAP):
                ex.map_visibility_words(1)
            assert np.array_equal(ex.map_step_skip_words()[0], words)  # (the step's own words stay readable: the map before the step)
    # the map and tracks are the step's and the measurement rows still valid: a plain step and a five-call sequence give the twins' bytes
    g, k = (f + 1) % n, (f + 2) % n
    state = ex.download_map()
    ex.clear_retired()
    want = ex.map_step(g, room.W2C[g], None, room.flags, ca.COMMIT_ADD_STAGED, nid, st)
    stepped = _state(ex)
    ex.clear_retired()
    _upload(ex, *state)
    five = _five_calls(ca, ex, st, n, g, room.W2C, None, room.flags, ca.COMMIT_ADD_STAGED, nid, room.meas[g], "after a visible step, ")
    assert want[0]["commit"].tobytes() == five[0].tobytes() and want[0]["maintain"].tobytes() == five[1].tobytes() and want[1] == five[2]
    _same_state(_state(ex), stepped, "a plain step after a visible one")
    commit, _, _ = _five_calls(ca, ex, st, n, k, room.W2C, None, room.flags, ca.COMMIT_ADD_STAGED, five[2], room.meas[k], "and again, ")
    assert commit["flags"] == ca.COMMIT_DONE
    ex.upload_map(room.arrays)
    with pytest.raises(ca.CapeError, match="cape_map_step_skip_words " + CAP):  # a new upload discards the words
        ex.map_step_skip_words()
    ex.clear_retired()
    room.restore()

"""What a changed device map invalidates, through the three calls that change it -- a DONE cape_map_commit, a DONE cape_map_maintain
and a cape_map_step whose buffer set changes -- and what their idle counterparts (a refused commit, a NOTHING maintenance, a step
whose commit is refused) leave alone.  After a changed map:

  * cape_match_map(CAPE_MATCH_MAP_DEVICE_SKIP) refuses: the words of the last cape_map_visibility stood for the old map;
  * cape_copy_map_union and cape_map_kalman refuse, the latter until a new cape_match_map_wide;
  * cape_map_info tells the sizes of the call's header and cape_map_download returns the new map's tracks, not zeros.

cape_map_step_skip_words outlives a commit (its words stand for the map the step found) and ends with a cape_map_upload.

The room's eight frames and its own map; a map of 1 024 far planes for the refusals.  Every test prints its figures before it asserts
(`pytest -s`)."""
import numpy as np
import pytest

import map_maintain_cases as MC
from test_gpu_map_commit import _pipeline, _wall_copies
from test_gpu_map_kalman import room  # noqa: F401  (the eight room frames after the four calls)

pytestmark = pytest.mark.gpu

CAP = r"failed \(-4\)"


def _make_current(ca, room, arrays, tracks):  # noqa: F811
    """a fresh upload, then everything a changed map invalidates made current: the wide match, the Kalman rows and the union of the
    batch and the visibility words of frame 0 -- and used once, so that a refusal below is the route's doing"""
    ex, st = room.ex, room.st
    ex.clear_retired()
    _pipeline(room, arrays, tracks)
    ex.map_visibility(1, room.W2C[:1], None, st)
    ex.match_map(1, room.W2C[:1], None, room.flags | ca.MATCH_MAP_DEVICE_SKIP, st)
    ex.map_union_rows(1)
    return ex.download_map()


def _sizes(header):
    return int(header["n_planes"]), int(header["n_rings"]), int(header["n_vertices"])


def _is_invalidated(ca, room, sizes, what):  # noqa: F811
    ex, n, st = room.ex, room.n, room.st
    with pytest.raises(ca.CapeError, match="cape_match_map " + CAP):
        ex.match_map(1, room.W2C[:1], None, room.flags | ca.MATCH_MAP_DEVICE_SKIP, st)
    with pytest.raises(ca.CapeError, match="cape_copy_map_union " + CAP):
        ex.map_union_rows(1)
    with pytest.raises(ca.CapeError, match="cape_map_kalman " + CAP):
        ex.map_kalman(1, st)
    info = ex.map_info()
    (P, R, V), T = ex.download_map()
    print(f"{what}: the map of {info} planes, rings, vertices; {np.count_nonzero(T['covariance'])} covariance entries are not zero")
    assert info == sizes and (len(P), len(R), len(V)) == sizes
    assert len(T) == sizes[0] and np.all(np.any(T["covariance"] != 0, axis=(1, 2))), what + ": the tracks of the new map"
    # a new wide match and new words make both possible again, on the map as it stands
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    ex.map_visibility(1, room.W2C[:1], None, st)
    ex.match_map(1, room.W2C[:1], None, room.flags | ca.MATCH_MAP_DEVICE_SKIP, st)


def _promotable(ca, room):  # noqa: F811
    """the room's map, nothing due but plane 0: staged and matched five times in a row"""
    tracks = room.tracks.copy()
    tracks["flags"], tracks["successive_matched"], tracks["failed_tracking"] = 0, 0, 0
    tracks["flags"][0], tracks["successive_matched"][0] = ca.MAP_TRACK_STAGED, 5
    return tracks


@pytest.mark.parametrize("route", ["commit", "maintain", "step"])
def test_a_changed_map_invalidates_the_same_through_every_route(room, route):  # noqa: F811
    import cape_amd as ca

    ex, st, f = room.ex, room.st, room.source
    print()
    before = _make_current(ca, room, room.arrays, _promotable(ca, room) if route == "maintain" else room.tracks)
    if route == "commit":
        header, nid = ex.map_commit(f, 0, 5, st)
        assert header["flags"] == ca.COMMIT_DONE and header["n_updated"] >= 1
    elif route == "maintain":
        header = ex.map_maintain(0, st)
        assert header["flags"] == ca.MAINTAIN_DONE and header["n_promoted"] == 1
    else:
        result, nid = ex.map_step(f, room.W2C[f], None, room.flags, 0, 5, st)
        assert result["commit"]["flags"] == ca.COMMIT_DONE
        header = result["maintain"] if result["maintain"]["flags"] & ca.MAINTAIN_DONE else result["commit"]
    _is_invalidated(ca, room, _sizes(header), route)
    assert ex.download_map()[1].tobytes() != before[1].tobytes()  # (the committed counters, or the promoted flag)
    ex.clear_retired()
    room.restore()


@pytest.fixture(scope="module")
def full(room):  # noqa: F811
    """1 024 far planes: a commit that appends is refused with CAPE_COMMIT_CAPACITY"""
    import cape_amd as ca

    return _wall_copies(ca, room, ca.MAP_MAX_PLANES, np.random.default_rng(8), far=True)


@pytest.mark.parametrize("route", ["refused commit", "nothing maintenance", "idle step"])
def test_the_idle_counterparts_invalidate_none_of_it(room, full, route):  # noqa: F811
    import cape_amd as ca

    ex, n, st = room.ex, room.n, room.st
    f = max(range(n), key=lambda g: sum(bool(m["flags"] & ca.MEASURE_STAGEABLE) for m in room.meas[g]))
    arrays, tracks = (room.arrays, room.tracks) if route == "nothing maintenance" else full
    print()
    before = _make_current(ca, room, arrays, tracks)
    sizes = ex.map_info()
    if route == "refused commit":
        header, nid = ex.map_commit(f, ca.COMMIT_ADD_STAGED, 70, st)
        assert header["flags"] == ca.COMMIT_CAPACITY and nid == 70
    elif route == "nothing maintenance":
        header = ex.map_maintain(0, st)
        assert header["flags"] == ca.MAINTAIN_NOTHING
    else:
        result, nid = ex.map_step(f, room.W2C[f], None, room.flags, ca.COMMIT_ADD_STAGED, 70, st)
        assert result["commit"]["flags"] == ca.COMMIT_CAPACITY and nid == 70 and not result["maintain"].tobytes().strip(b"\0")
    print(f"{route}: the map of {ex.map_info()} planes, rings, vertices")
    ex.match_map(1, room.W2C[:1], None, room.flags | ca.MATCH_MAP_DEVICE_SKIP, st)  # the words are still the map's
    assert ex.map_info() == sizes
    MC.same_map(ex.download_map(), before, route + ": the map and its tracks")
    if route == "idle step":
        # the step worked in row 0 of the batch-wide tables, whatever its headers say: their results are not current
        with pytest.raises(ca.CapeError, match="cape_copy_map_union " + CAP):
            ex.map_union_rows(1)
        with pytest.raises(ca.CapeError, match="cape_map_kalman " + CAP):
            ex.map_kalman(1, st)
    else:
        ex.map_union_rows(1)
        ex.map_kalman(n, st)
    ex.clear_retired()
    room.restore()


def test_the_step_words_outlive_a_commit_and_end_with_an_upload(room):  # noqa: F811
    import cape_amd as ca

    ex, n, st, f = room.ex, room.n, room.st, room.source
    room.restore()
    n_before = ex.map_info()[0]
    result, nid = ex.map_step_visible(f, room.W2C[f], room.flags, 0, 5, st)
    words, n_map = ex.map_step_skip_words()
    print(f"\nstep_visible: commit {int(result['step']['commit']['flags']):#x}, the words of {n_map} planes: {words.tolist()}")
    assert result["step"]["commit"]["flags"] == ca.COMMIT_DONE and n_map == n_before == result["n_map"]
    ex.match_map_wide(n, room.W2C, None, room.flags, st)
    ex.map_kalman(n, st)
    ex.map_union_cut(n, st)
    header, nid = ex.map_commit((f + 1) % n, ca.COMMIT_ADD_STAGED, nid, st)
    assert header["flags"] == ca.COMMIT_DONE
    again, n_again = ex.map_step_skip_words()
    assert n_again == n_map and again.tolist() == words.tolist()  # the words of the map the step found, whatever became of it
    ex.upload_map(room.arrays)
    with pytest.raises(ca.CapeError, match="cape_map_step_skip_words " + CAP):
        ex.map_step_skip_words()
    ex.clear_retired()
    room.restore()

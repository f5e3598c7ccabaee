"""cape_host_map_maintain -- the host twin of cape_map_maintain: PROMOTE, DROP and LOST executed on the ordered map list, with the
retired log -- against the reference's loops restated on Python lists (tests/map_maintain_cases.py).  The call moves data and
compares integers, so every comparison is on bytes: planes, rings, vertices, tracks, the log and the result header.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import map_maintain_cases as MC
from test_map_commit_host import _inputs
from test_map_update_host import CTR, D, N, X, Y, L, _det, _map, _square, ca  # noqa: F401


@pytest.fixture(scope="module")
def cov(ca, L):  # noqa: F811
    """a valid 4 x 4 plane covariance: the hand-built maps' own"""
    c = _map(ca, L, 1)[1][0]["covariance"].copy()
    assert L.cape_host_covariance_valid(np.ascontiguousarray(c).ctypes.data_as(C.c_void_p), 4) == 1
    return c


def _bad_covariances(cov):
    nan = cov.copy()
    nan[1, 2] = np.nan
    skew = cov.copy()
    skew[0, 1] += 0.5 * np.abs(cov).max()
    return dict(nan=nan, asymmetric=skew, negative_pivot=np.diag([1.0, 1.0, -1.0, 1.0]))


def _plane(staged=False, sm=0, ft=0, rings=1, moving=False, covariance=None, scale=1.0):
    return dict(staged=staged, sm=sm, ft=ft, rings=rings, moving=moving, covariance=covariance, scale=scale)


def _build(ca, cov, specs, first_id=100):  # noqa: F811
    """a map of one plane per spec, each 3 m beside the last, its holes small squares inside it: every ring in the host class's
    orientation (outer ring clockwise, holes counter-clockwise), so the class leaves the vertices as they are.  Returns (arrays,
    tracks, promotable)."""
    planes, tracks, promotable = [], np.zeros(len(specs), ca.MAP_TRACK_DTYPE), []
    for j, s in enumerate(specs):
        holes = [_square(-450 + 100 * k, -400 + 100 * k, -25 - j, 25 + j)[::-1] + [3000 * j, 0] for k in range(s["rings"] - 1)]
        planes.append((N * s["scale"], D, X, Y, CTR, _square(-500, 500, -500 - j, 500 + j) + [3000 * j, 0], holes))
        tracks[j]["covariance"] = cov if s["covariance"] is None else s["covariance"]
        tracks[j]["successive_matched"], tracks[j]["failed_tracking"] = s["sm"], s["ft"]
        tracks[j]["flags"] = (ca.MAP_TRACK_STAGED if s["staged"] else 0) | (ca.MAP_TRACK_MOVING if s["moving"] else 0)
        tracks[j]["result"], tracks[j]["id"] = 0x40 + j, first_id + j
        promotable.append(s["covariance"] is None and s["scale"] == 1.0)
    return ca.pack_map(planes), tracks, promotable


def _both(ca, arrays, tracks, promotable, retired=None, retired_held=None):  # noqa: F811
    """the twin and the restated loops on the same map: header, map, tracks and log byte for byte.  Returns (result, the new map and
    tracks or None, the log)."""
    entries = MC.entries_of(arrays, tracks)
    log0 = retired if retired is not None else MC.arrays_of(ca, [])
    held = retired_held if retired_held is not None else (len(log0[0][0]), len(log0[0][1]), len(log0[0][2]))
    want, new, lost = MC.reference_maintain(ca, entries, promotable, held)
    got_map, got_tracks, got_log, result = ca.host_map_maintain(arrays, tracks, retired, retired_held)
    assert result.tobytes() == want.tobytes(), f"header {result} != {want}"
    if new is None:
        assert got_map is None and got_tracks is None
        if retired_held is None:
            MC.same_map(got_log, log0, "the log of a call that is not DONE")
        return result, None, got_log
    MC.same_map((got_map, got_tracks), MC.arrays_of(ca, new), "the new map")
    if retired_held is None:
        MC.same_map(got_log, MC.arrays_of(ca, lost, log0), "the log")
    return result, (got_map, got_tracks), got_log


# ---- thresholds -----------------------------------------------------------------------------------------------------------------
def test_the_thresholds_at_their_edges(ca, cov):  # noqa: F811
    specs = [_plane(True, sm=3), _plane(True, sm=4), _plane(True, ft=1), _plane(True, ft=2), _plane(ft=9), _plane(ft=10)]
    arrays, tracks, ok = _build(ca, cov, specs)
    result, (new, Tr), (log, logT) = _both(ca, arrays, tracks, ok)
    assert result["flags"] == ca.MAINTAIN_DONE
    assert (result["n_promoted"], result["n_dropped"], result["n_lost"], result["n_promote_refused"]) == (1, 1, 1, 0)
    # local survivors first -- the promoted plane (id 101) among them, in list order -- then the staged ones
    assert Tr["id"].tolist() == [101, 104, 100, 102] and (result["n_local"], result["n_staged"]) == (2, 2)
    assert Tr["flags"].tolist() == [0, 0, ca.MAP_TRACK_STAGED, ca.MAP_TRACK_STAGED]
    assert Tr["failed_tracking"].tolist() == [0, 9, 0, 1] and Tr["successive_matched"].tolist() == [4, 0, 3, 0]
    assert Tr[0]["result"] == 0x41 and Tr[0]["covariance"].tobytes() == tracks[1]["covariance"].tobytes()
    assert logT["id"].tolist() == [105] and logT[0]["failed_tracking"] == 10 and result["n_retired"] == 1
    # one below each threshold alone: nothing is due
    arrays, tracks, ok = _build(ca, cov, [specs[0], specs[2], specs[4]])
    result, new, _ = _both(ca, arrays, tracks, ok)
    assert result["flags"] == ca.MAINTAIN_NOTHING and new is None and result["n_planes"] == 3


def test_promote_wins_over_drop_and_a_local_plane_is_never_promoted(ca, cov):  # noqa: F811
    arrays, tracks, ok = _build(ca, cov, [_plane(True, sm=7, ft=5), _plane(False, sm=9, ft=3)])
    result, (new, Tr), (log, logT) = _both(ca, arrays, tracks, ok)
    assert result["flags"] == ca.MAINTAIN_DONE and (result["n_promoted"], result["n_dropped"], result["n_lost"]) == (1, 0, 0)
    assert Tr["id"].tolist() == [100, 101] and Tr["flags"].tolist() == [0, 0] and Tr["failed_tracking"].tolist() == [0, 3]
    assert Tr["successive_matched"].tolist() == [7, 9] and len(logT) == 0
    # the local plane alone: nothing happens
    arrays, tracks, ok = _build(ca, cov, [_plane(False, sm=9, ft=3)])
    assert _both(ca, arrays, tracks, ok)[0]["flags"] == ca.MAINTAIN_NOTHING


def test_a_moving_lost_plane_is_logged_with_its_flag(ca, cov):  # noqa: F811
    arrays, tracks, ok = _build(ca, cov, [_plane(ft=10, moving=True, rings=2), _plane(ft=11), _plane(ft=2)])
    result, (new, Tr), (log, logT) = _both(ca, arrays, tracks, ok)
    assert result["flags"] == ca.MAINTAIN_DONE and result["n_lost"] == 2 and Tr["id"].tolist() == [102]
    assert logT["id"].tolist() == [100, 101] and logT["flags"].tolist() == [ca.MAP_TRACK_MOVING, 0]
    assert logT["result"].tolist() == [0x40, 0x41] and log[0]["ring_count"].tolist() == [2, 1]


@pytest.mark.parametrize("cause", ["nan", "asymmetric", "negative_pivot", "normal"])
def test_a_refused_promotion_stays_staged_and_is_not_dropped(ca, L, cov, cause):  # noqa: F811
    bad = _bad_covariances(cov)
    for c in bad.values():  # the three covariances are invalid for the host algebra, each for its own reason
        assert L.cape_host_covariance_valid(np.ascontiguousarray(c).ctypes.data_as(C.c_void_p), 4) == 0
    spec = _plane(True, sm=5, ft=6, scale=1.0 + 1e-12) if cause == "normal" else _plane(True, sm=5, ft=6, covariance=bad[cause])
    # alone: counted, and nothing is due
    arrays, tracks, ok = _build(ca, cov, [spec])
    assert ok == [False]
    result, new, _ = _both(ca, arrays, tracks, ok)
    assert result["flags"] == ca.MAINTAIN_NOTHING and result["n_promote_refused"] == 1 and result["n_staged"] == 1 and new is None
    # beside a plane that is dropped: it stays staged and unchanged behind the local planes
    arrays, tracks, ok = _build(ca, cov, [spec, _plane(True, ft=2), _plane(ft=1)])
    result, (new, Tr), _ = _both(ca, arrays, tracks, ok)
    assert result["flags"] == ca.MAINTAIN_DONE and (result["n_promote_refused"], result["n_dropped"], result["n_promoted"]) == (1, 1, 0)
    assert Tr["id"].tolist() == [102, 100] and Tr[1].tobytes() == tracks[0].tobytes()
    assert new[0][1]["normal"].tobytes() == arrays[0][0]["normal"].tobytes()


# ---- shapes and orders ----------------------------------------------------------------------------------------------------------
def test_an_empty_map_and_a_map_that_is_removed_whole(ca, cov):  # noqa: F811
    arrays, tracks, ok = _build(ca, cov, [])
    result, new, (log, logT) = _both(ca, arrays, tracks, ok)
    assert result["flags"] == ca.MAINTAIN_NOTHING and result["n_planes"] == 0 and len(logT) == 0
    arrays, tracks, ok = _build(ca, cov, [_plane(ft=10, rings=3), _plane(True, ft=2), _plane(ft=12), _plane(True, ft=9, sm=-9)])
    result, (new, Tr), (log, logT) = _both(ca, arrays, tracks, ok)
    assert result["flags"] == ca.MAINTAIN_DONE
    assert (result["n_planes"], result["n_rings"], result["n_vertices"]) == (0, 0, 0) and len(new[0]) == len(new[1]) == len(new[2]) == 0
    assert (result["n_dropped"], result["n_lost"]) == (2, 2) and logT["id"].tolist() == [100, 102] and len(log[1]) == 4


def test_a_mixed_order_becomes_a_stable_partition(ca, cov):  # noqa: F811
    # S keep, L keep, S promote, L lost, S drop, L keep, S promote, S keep, L keep
    specs = [_plane(True), _plane(), _plane(True, sm=4), _plane(ft=10), _plane(True, ft=2), _plane(), _plane(True, sm=6), _plane(True, sm=3), _plane()]
    arrays, tracks, ok = _build(ca, cov, specs)
    result, (new, Tr), (log, logT) = _both(ca, arrays, tracks, ok)
    assert Tr["id"].tolist() == [101, 102, 105, 106, 108, 100, 107] and (result["n_local"], result["n_staged"]) == (5, 2)
    assert logT["id"].tolist() == [103]
    # a list that has its local planes first: the promoted plane goes behind the last local one, the rest keeps its order
    specs = [_plane(), _plane(), _plane(True), _plane(True, sm=4), _plane(True)]
    arrays, tracks, ok = _build(ca, cov, specs)
    _, (new, Tr), _ = _both(ca, arrays, tracks, ok)
    assert Tr["id"].tolist() == [100, 101, 103, 102, 104]


def test_rings_and_vertices_are_rebased_in_the_map_and_in_the_log(ca, cov):  # noqa: F811
    # 1, 2 and 9 rings among the removed and the kept planes
    specs = [_plane(rings=9), _plane(ft=10, rings=2), _plane(True, ft=2, rings=9), _plane(rings=1), _plane(ft=10, rings=9), _plane(True, rings=2),
             _plane(ft=10, rings=1), _plane(True, sm=4, rings=9)]
    arrays, tracks, ok = _build(ca, cov, specs)
    first = ca.pack_map([(N, D, X, Y, CTR, _square(0, 7, 0, 7), [_square(1, 2, 1, 2)[::-1]])])
    retired = (first, np.zeros(1, ca.MAP_TRACK_DTYPE))
    result, ((P, R, V), Tr), ((LP, LR, LV), LT) = _both(ca, arrays, tracks, ok, retired)
    assert P["ring_count"].tolist() == [9, 1, 9, 2] and P["ring_first"].tolist() == [0, 9, 10, 19] and Tr["id"].tolist() == [100, 103, 107, 105]
    assert R["vertex_offset"].tolist() == list(range(0, 4 * 21, 4)) and len(V) == 84
    assert LP["ring_count"].tolist() == [2, 2, 9, 1] and LP["ring_first"].tolist() == [0, 2, 4, 13] and LT["id"].tolist() == [0, 101, 104, 106]
    assert LR["vertex_offset"].tolist() == list(range(0, 4 * 14, 4))
    assert (result["n_retired"], result["n_retired_rings"], result["n_retired_vertices"]) == (4, 14, 56)
    for j, src in ((1, 1), (2, 4), (3, 6)):  # each logged plane's rings are the map plane's own
        a = MC.entries_of((LP, LR, LV), LT)[j]["rings"]
        b = MC.entries_of(arrays, tracks)[src]["rings"]
        assert len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- call behaviour -------------------------------------------------------------------------------------------------------------
def test_the_call_is_idempotent(ca, cov):  # noqa: F811
    bad = _bad_covariances(cov)["nan"]
    specs = [_plane(True, sm=4), _plane(ft=10), _plane(True, ft=2), _plane(True, sm=4, covariance=bad), _plane(), _plane(True)]
    arrays, tracks, ok = _build(ca, cov, specs)
    result, (new, Tr), log = _both(ca, arrays, tracks, ok)
    assert result["flags"] == ca.MAINTAIN_DONE
    again, nothing, log2 = _both(ca, new, Tr, [True, True, False, True], log)
    assert again["flags"] == ca.MAINTAIN_NOTHING and nothing is None and again["n_promote_refused"] == 1
    assert (again["n_planes"], again["n_rings"], again["n_vertices"]) == (result["n_planes"], result["n_rings"], result["n_vertices"])
    MC.same_map(log2, log, "the log after a second call")


def test_the_log_grows_over_two_calls(ca, cov):  # noqa: F811
    arrays, tracks, ok = _build(ca, cov, [_plane(ft=10, rings=2), _plane(), _plane(ft=10)])
    _, _, log = _both(ca, arrays, tracks, ok)
    arrays, tracks, ok = _build(ca, cov, [_plane(), _plane(ft=11, rings=3)], first_id=200)
    result, _, (log, logT) = _both(ca, arrays, tracks, ok, log)
    assert logT["id"].tolist() == [100, 102, 201] and log[0]["ring_first"].tolist() == [0, 2, 3] and result["n_retired"] == 3
    # cleared: the next call starts an empty log again
    result, _, (log, logT) = _both(ca, arrays, tracks, ok, None)
    assert logT["id"].tolist() == [201] and log[0]["ring_first"].tolist() == [0] and result["n_retired"] == 1


def test_the_log_is_full_at_its_cap(ca, cov):  # noqa: F811
    cap = ca.MAP_RETIRED_MAX_PLANES
    arrays, tracks, ok = _build(ca, cov, [_plane(ft=10), _plane(True, ft=2), _plane(ft=10), _plane()])
    # two lost planes: they fit a log of cap - 2 ...
    result, new, (log, logT) = _both(ca, arrays, tracks, ok, None, (cap - 2, 5, 70))
    assert result["flags"] == ca.MAINTAIN_DONE and result["n_retired"] == cap and len(logT) == cap
    assert logT["id"][cap - 2:].tolist() == [100, 102] and log[0]["ring_first"][cap - 2:].tolist() == [5, 6]
    assert log[1]["vertex_offset"][5:].tolist() == [70, 74] and (result["n_retired_rings"], result["n_retired_vertices"]) == (7, 78)
    # ... and not one of cap - 1: refused, nothing changed, though other planes were due
    result, new, (log, logT) = _both(ca, arrays, tracks, ok, None, (cap - 1, 5, 70))
    assert result["flags"] == ca.MAINTAIN_LOG_FULL and new is None and result["n_retired"] == cap - 1 and len(logT) == cap - 1
    assert (result["n_planes"], result["n_lost"], result["n_dropped"]) == (4, 2, 1) and not logT.view(np.uint8).any()
    # a full log does not refuse a call that loses nothing
    arrays, tracks, ok = _build(ca, cov, [_plane(True, ft=2), _plane()])
    assert _both(ca, arrays, tracks, ok, None, (cap, 0, 0))[0]["flags"] == ca.MAINTAIN_DONE


def test_a_plane_outside_the_maps_buffers_refuses_the_call(ca, cov):  # noqa: F811
    arrays, tracks, ok = _build(ca, cov, [_plane(ft=10), _plane(True, ft=2), _plane()])
    P, R, V = arrays
    for field, value in (("ring_first", 3), ("ring_count", 10), ("ring_count", 0)):
        broken = P.copy()
        broken[2][field] = value
        new, _, (_, logT), result = ca.host_map_maintain((broken, R, V), tracks)
        assert result["flags"] == ca.MAINTAIN_CAPACITY and new is None and len(logT) == 0 and result["n_planes"] == 3
    short = R.copy()
    short[1]["vertex_offset"] = len(V) - 3
    assert ca.host_map_maintain((P, short, V), tracks)[3]["flags"] == ca.MAINTAIN_CAPACITY


def test_arrays_that_are_too_small(ca, cov):  # noqa: F811
    Lh = ca._host_library()
    arrays, tracks, _ = _build(ca, cov, [_plane(ft=10), _plane(True, ft=2), _plane()])
    src, view = ca._map_arrays(arrays, np.ascontiguousarray(tracks, ca.MAP_TRACK_DTYPE))

    def room(planes, rings, vertices):
        a = dict(planes=np.zeros(max(planes, 1), ca.MAP_PLANE_DTYPE), rings=np.zeros(max(rings, 1), ca.MAP_RING_DTYPE),
                 vertices=np.zeros((max(vertices, 1), 2)), tracks=np.zeros(max(planes, 1), ca.MAP_TRACK_DTYPE))
        return a, ca._view(ca.cape_host_map, a, planes_capacity=planes, rings_capacity=rings, vertices_capacity=vertices)

    result = np.zeros(1, ca.MAP_MAINTAIN_RESULT_DTYPE)
    for out_caps, log_caps, want in (((1, 1, 4), (1, 1, 4), 0), ((0, 1, 4), (1, 1, 4), ca.CAPE_ERR_CAPACITY), ((1, 1, 3), (1, 1, 4), ca.CAPE_ERR_CAPACITY),
                                     ((1, 1, 4), (0, 1, 4), ca.CAPE_ERR_CAPACITY), ((1, 1, 4), (1, 0, 4), ca.CAPE_ERR_CAPACITY)):
        (out, v), (log, lv) = room(*out_caps), room(*log_caps)
        assert Lh.cape_host_map_maintain(C.byref(view), C.byref(v), C.byref(lv), result.ctypes.data) == want, (out_caps, log_caps)
        assert result[0]["flags"] == ca.MAINTAIN_DONE
        if want:
            assert lv.n_planes == 0 and not any(a.view(np.uint8).any() for a in (*out.values(), *log.values())), "an output was written"
    assert Lh.cape_host_map_maintain(None, C.byref(v), C.byref(lv), result.ctypes.data) == -1
    assert Lh.cape_host_map_maintain(C.byref(view), C.byref(v), None, result.ctypes.data) == -1


# ---- after a commit the counters and the bits agree -----------------------------------------------------------------------------
def test_after_a_commit_the_counters_name_the_class_the_result_bits_name(ca, L, cov):  # noqa: F811
    """the hand-built update cases of tests/test_map_commit_host.py with counters one step below every threshold: cape_host_map_commit
    writes counters and PROMOTE / DROP / LOST bits; the class decided from the counters is the one the bits name, for every plane,
    and the maintenance executes exactly those"""
    arrays, tracks = _map(ca, L, 6, staged=(2, 3, 4))
    tracks["successive_matched"] = [2, 2, 3, 0, 3, 0]
    tracks["failed_tracking"] = [0, 9, 0, 1, 0, 9]
    bad = np.full((3, 3), np.nan)
    det = [_det(_square(-400 + 3000 * j, 400 + 3000 * j, -400, 400), cov=bad if j in (1, 3) else np.diag([20.0, 20.0, 4.0])) for j in range(6)]
    seen = set()
    for match in ([0, 1, 2, 3, 4, 5], [-1] * 6, [0, -1, 2, -1, -1, 5]):
        new, Tr, result, _ = ca.host_map_commit(arrays, tracks, *_inputs(ca, L, arrays, tracks, match, det), ca.COMMIT_ADD_STAGED, 9, frame=0)
        assert result["flags"] == ca.COMMIT_DONE
        classes = [MC.class_of(ca, t) for t in Tr]
        assert classes == [MC.class_of_result(ca, int(t["result"]), bool(t["flags"] & ca.MAP_TRACK_STAGED)) for t in Tr]
        seen |= set(classes)
        result, _, _ = _both(ca, new, Tr, [True] * len(Tr))
        bits = Tr["result"]
        assert result["n_promoted"] == np.count_nonzero(bits & ca.MAP_RESULT_PROMOTE) and result["n_promote_refused"] == 0
        assert result["n_dropped"] == np.count_nonzero(bits & ca.MAP_RESULT_DROP) and result["n_lost"] == np.count_nonzero(bits & ca.MAP_RESULT_LOST)
    assert {MC.PROMOTED, MC.DROPPED, MC.LOST, MC.KEEP_LOCAL, MC.KEEP_STAGED} <= seen

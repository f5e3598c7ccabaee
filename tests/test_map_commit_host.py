"""cape_host_map_commit -- the host twin of cape_map_commit: a frame's Kalman, measurement and union results written into the map --
against cape_host_map_update itself, fed the rows of the other twins (cape_host_map_kalman, cape_host_map_union_cut and measurement
rows of the update's own algebra).  The commit has no arithmetic, so every comparison is on bytes: planes, rings, vertices and
tracks.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from map_union_cut_cases import CUT_HOLES, PIECES
from map_union_hole_cases import CAPACITY, TABLES
from test_map_union_host import L, _measurement_rows, _one_plane_map, _world, ca  # noqa: F401
from test_map_update_host import D, POSE, _det, _map, _square

W = 128
T = np.eye(4)


def _rows(ca, L, det):  # noqa: F811
    """the measurement rows of tests/test_map_union_host.py with the staged plane's normal: one more normalisation, which leaves the
    axis-aligned unit normals of these cases as they are"""
    rows = _measurement_rows(ca, L, det)
    for r in rows:
        n = r["normal"]
        norm = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        r["staged_normal"] = n / norm if norm > 0 else n
    return rows


def _slab(ca, rows, polygons):
    """a frame's slab from the polygons the union twin returns: every served polygon's rings back to back at its row's offset"""
    slab = np.zeros((ca.MAP_UNION_FRAME_VERTICES, 2))
    for row, poly in zip(rows, polygons):
        if poly is None:
            continue
        at = int(row["vertex_offset"])
        for ring in (poly if isinstance(poly, list) else [poly]):
            slab[at: at + len(ring)] = ring
            at += len(ring)
    return slab


def _inputs(ca, L, arrays, tracks, match, det, plain=False):  # noqa: F811
    """what the commit reads of a frame: the other twins on the update's own algebra"""
    mrows = _rows(ca, L, det)
    worlds = [_world(np.asarray(d[5], np.float64)) for d in det]
    frame, frows, tres = ca.host_map_kalman(arrays, tracks, match, mrows)
    if plain:
        urows, rings = ca.host_map_union(arrays, match, frows, mrows, worlds)
        return frame, tres, frows, mrows, worlds, urows, None, _slab(ca, urows, rings)
    urows, rrows, polys = ca.host_map_union_cut(arrays, match, frows, mrows, worlds)
    return frame, tres, frows, mrows, worlds, urows, rrows, _slab(ca, urows, polys)


def _same_map(got, want):
    (P, R, V), Tr = got
    (P2, R2, V2), Tr2 = want
    for name, a, b in (("planes", P, P2), ("rings", R, R2), ("vertices", V, V2), ("tracks", Tr, Tr2)):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name


def _against_the_update(ca, L, arrays, tracks, match, det, flags=0, next_id=0, plain=False):  # noqa: F811
    """the twin's map against the update's: bytes.  Returns (the new map, its tracks, the commit's result, next_id)."""
    want = ca.host_map_update(arrays, tracks, match, det, T, POSE, ca.MAP_ADD_STAGED if flags & ca.COMMIT_ADD_STAGED else 0, next_id)
    got = ca.host_map_commit(arrays, tracks, *_inputs(ca, L, arrays, tracks, match, det, plain), flags, next_id, frame=3)
    new, Tr, result, nid = got
    assert result["flags"] == ca.COMMIT_DONE and result["frame"] == 3, f"refused: {result}"
    _same_map((new, Tr), (want[0], want[1]))
    assert nid == want[3] == result["next_id"]
    assert (result["n_planes"], result["n_rings"], result["n_vertices"]) == (len(new[0]), len(new[1]), len(new[2]))
    assert result["n_appended"] == len(new[0]) - len(arrays[0]) and result["n_host_pairs"] == 0 and result["n_fail_polygon"] == 0
    assert result["n_updated"] == int(np.count_nonzero(Tr["result"][:len(arrays[0])] & ca.MAP_RESULT_UPDATED))
    return got


def _refused(ca, L, arrays, tracks, inputs, flags=0, next_id=5):  # noqa: F811
    """a refused frame through the C entry itself: map_out keeps the bytes it had, next_id its value, the counts are the old map's"""
    Lh = ca._host_library()
    src, view = ca._map_arrays(arrays, np.ascontiguousarray(tracks, ca.MAP_TRACK_DTYPE))
    frame, tres, frows, mrows, worlds, urows, rrows, slab = inputs
    H = np.zeros(1, ca.FRAME_MAP_KALMAN_DTYPE)
    H[0] = frame

    def pad(a, dtype):
        out = np.zeros(W, dtype)
        out[:len(a)] = a
        return out

    F, M, U = pad(frows, ca.PLANE_FUSION_DTYPE), pad(mrows, ca.PLANE_MEASUREMENT_DTYPE), pad(urows, ca.PLANE_UNION_DTYPE)
    Q = None if rrows is None else pad(rrows, ca.PLANE_UNION_RINGS_DTYPE)
    Wv = np.ascontiguousarray(np.concatenate(list(worlds) + [np.zeros((1, 2))]))
    R = np.ascontiguousarray(tres, ca.MAP_TRACK_RESULT_DTYPE)
    n = len(arrays[0]) + W
    out = dict(planes=np.full(n, 0x5A, np.uint8).repeat(ca.MAP_PLANE_DTYPE.itemsize).view(ca.MAP_PLANE_DTYPE),
               rings=np.full(9 * n * ca.MAP_RING_DTYPE.itemsize, 0x5A, np.uint8).view(ca.MAP_RING_DTYPE),
               vertices=np.full((len(arrays[2]) + 70000, 2), 7.25), tracks=np.full(n * ca.MAP_TRACK_DTYPE.itemsize, 0x5A, np.uint8).view(ca.MAP_TRACK_DTYPE))
    before = [a.tobytes() for a in out.values()]
    v = ca._view(ca.cape_host_map, out, planes_capacity=len(out["planes"]), rings_capacity=len(out["rings"]), vertices_capacity=len(out["vertices"]),
                 n_planes=-7, n_rings=-7, n_vertices=-7)
    nid, result = C.c_uint64(next_id), np.zeros(1, ca.MAP_COMMIT_RESULT_DTYPE)
    rc = Lh.cape_host_map_commit(C.byref(view), 0, H.ctypes.data, R.ctypes.data, F.ctypes.data, M.ctypes.data, Wv.ctypes.data, U.ctypes.data,
                                 None if Q is None else Q.ctypes.data, slab.ctypes.data, flags, C.byref(nid), C.byref(v), result.ctypes.data)
    assert rc == 0 and not result[0]["flags"] & ca.COMMIT_DONE
    assert [a.tobytes() for a in out.values()] == before and (v.n_planes, v.n_rings, v.n_vertices) == (-7, -7, -7), "map_out was written"
    assert nid.value == next_id == result[0]["next_id"]
    assert (result[0]["n_planes"], result[0]["n_rings"], result[0]["n_vertices"]) == (len(arrays[0]), len(arrays[1]), len(arrays[2]))
    return result[0]


# ---- the twin equals the update -------------------------------------------------------------------------------------------------
def test_the_hand_built_cases_of_the_update(ca, L):  # noqa: F811
    # a matched plane: parameters, covariance and polygon; through the cut mode's rows and through the plain union's
    arrays, tracks = _map(ca, L, 1)
    det = [_det(_square(0, 1000, -500, 500), d=1010.0)]
    for plain in (False, True):
        (P, R, V), Tr, result, _ = _against_the_update(ca, L, arrays, tracks, [0], det, plain=plain)
        assert result["n_updated"] == 1 and Tr[0]["id"] == 100 and 1000.0 < P[0]["d"] < 1010.0
    # counters and the used rule: planes 0, 1 local, 2, 3 staged; 1 and 3 take a detection whose covariance is invalid
    arrays, tracks = _map(ca, L, 4, staged=(2, 3))
    tracks["successive_matched"] = [2, 2, 3, 0]
    tracks["failed_tracking"] = [0, 9, 0, 1]
    bad = np.full((3, 3), np.nan)
    det = [_det(_square(-400, 400, -400, 400)), _det(_square(2600, 3400, -400, 400), cov=bad),
           _det(_square(5600, 6400, -400, 400)), _det(_square(8600, 9400, -400, 400), cov=bad), _det(_square(0, 10, 0, 10))]
    for match in ([0, 1, 2, 3], [-1, -1, -1, -1], [2, -1, 0, 4]):
        for flags in (0, ca.COMMIT_ADD_STAGED):
            _against_the_update(ca, L, arrays, tracks, match, det, flags, next_id=9)
    # failed updates that leave the plane as it was: a detection covariance that is not valid, the map plane's own
    arrays, tracks = _map(ca, L, 1)
    ring = _square(-400, 400, -400, 400)
    _, Tr, result, _ = _against_the_update(ca, L, arrays, tracks, [0], [_det(ring, cov=np.full((3, 3), np.inf))])
    assert Tr[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_DETECTION and result["n_updated"] == 0
    broken = tracks.copy()
    broken[0]["covariance"] = -np.eye(4)
    _, Tr, _, _ = _against_the_update(ca, L, arrays, broken, [0], [_det(ring)])
    assert Tr[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_STATE
    # a map plane with a hole: the hole survives a detection beside it, a detection over it fills it
    hole = _square(-100, 100, -100, 100)[::-1]
    arrays, tracks = _map(ca, L, 1, holes=[hole])
    (P, _, _), _, _, _ = _against_the_update(ca, L, arrays, tracks, [0], [_det(_square(300, 1200, -500, 500))])
    assert P[0]["ring_count"] == 2
    (P, _, _), _, _, _ = _against_the_update(ca, L, arrays, tracks, [0], [_det(_square(-300, 300, -300, 300))])
    assert P[0]["ring_count"] == 1


def test_the_unions_overflow_is_the_hosts(ca, L):  # noqa: F811
    """the update keeps the old polygon with CAPE_MAP_RESULT_OVERFLOW; the union twin hands the pair over, the commit refuses the frame"""
    arrays, tracks = _map(ca, L, 1)
    t = np.linspace(0, 2 * np.pi, 1100, endpoint=False)
    r = np.where(np.arange(1100) % 2 == 0, 760.0, 720.0)
    comb = np.stack([r * np.cos(-t), r * np.sin(-t)], 1)
    inputs = _inputs(ca, L, arrays, tracks, [0], [_det(comb, d=1010.0)])
    assert inputs[5][0]["flags"] == ca.UNION_HOST_CAPACITY
    result = _refused(ca, L, arrays, tracks, inputs)
    assert result["flags"] == ca.COMMIT_HOST_PAIR and result["n_host_pairs"] == 1 and result["n_fail_polygon"] == 0


SERVED_ROWS = [(name, rings_a, b) for name, rings_a, b, outcome in TABLES + CUT_HOLES if outcome != CAPACITY]
CAPACITY_ROWS = [(name, rings_a, b) for name, rings_a, b, outcome in TABLES + CUT_HOLES if outcome == CAPACITY]


@pytest.mark.parametrize("case", SERVED_ROWS, ids=[c[0] for c in SERVED_ROWS])
@pytest.mark.parametrize("d", [D, 1010.0], ids=["same plane", "fused plane"])
def test_every_served_table_row_as_a_one_plane_map(ca, L, case, d):  # noqa: F811
    """unions that gain, keep, drop and cut holes (tests/map_union_hole_cases.py, tests/map_union_cut_cases.py)"""
    name, rings_a, b = case
    arrays, tracks = _one_plane_map(ca, L, rings_a[0], rings_a[1:])
    (P, R, V), _, result, _ = _against_the_update(ca, L, arrays, tracks, [0], [_det(b, d=d)])
    assert result["n_updated"] == 1 and P[0]["ring_count"] == len(R)


def test_the_tables_hold_every_kind_of_hole_change():
    assert len(SERVED_ROWS) >= 20 and len(CAPACITY_ROWS) >= 1 and len(PIECES) >= 3
    assert any(len(rings_a) == 1 for _, rings_a, _ in SERVED_ROWS) and any(len(rings_a) > 1 for _, rings_a, _ in SERVED_ROWS)


def _five_planes(ca, L):  # noqa: F811
    """five planes, local and staged in turn, with the counters of tests/test_gpu_map_kalman.py::_tracks: one short of promote (4
    successive matches), of lost (10 failures) and of drop (2 failures)"""
    arrays, tracks = _map(ca, L, 5, staged=(0, 2, 4))
    kinds = ((3, 0), (5, 9), (0, 1), (2, 0), (3, 0))
    for j, (s, f) in enumerate(kinds):
        tracks[j]["successive_matched"], tracks[j]["failed_tracking"] = s, f
    det = [_det(_square(-400, 600, -400, 400), d=1004.0), _det(_square(5800, 6700, -450, 400), d=997.0), _det(_square(11800, 12400, -300, 300)),
           _det(_square(20000, 20500, 0, 500))]
    return arrays, tracks, [0, -1, 1, -1, 2], det


def test_a_five_plane_map_with_unmatched_planes_and_every_counter_kind(ca, L):  # noqa: F811
    arrays, tracks, match, det = _five_planes(ca, L)
    _, Tr, result, _ = _against_the_update(ca, L, arrays, tracks, match, det)
    res = Tr["result"]
    assert res[0] & ca.MAP_RESULT_PROMOTE and res[1] & ca.MAP_RESULT_LOST and res[2] & ca.MAP_RESULT_UPDATED and not res[3]
    assert result["n_updated"] == 3 and Tr["id"].tolist() == [100, 101, 102, 103, 104]
    # every plane unmatched: the staged plane one failure short drops
    _, Tr, _, _ = _against_the_update(ca, L, arrays, tracks, [-1] * 5, det)
    assert Tr[2]["result"] == ca.MAP_RESULT_DROP and Tr[1]["result"] == ca.MAP_RESULT_LOST


def test_add_staged_appends_the_stageable_unused_detections(ca, L):  # noqa: F811
    arrays, tracks = _map(ca, L, 1)
    bad = np.full((3, 3), np.nan)
    det = [_det(_square(-400, 400, -400, 400)), _det(_square(2000, 2500, 0, 500), cov=bad), _det(_square(-3000, -2500, 0, 400)),
           _det(_square(4000, 4700, 0, 400))]
    (P, _, _), Tr, result, nid = _against_the_update(ca, L, arrays, tracks, [0], det, 0, next_id=40)
    assert len(P) == 1 and nid == 40 and result["n_appended"] == 0
    (P, R, V), Tr, result, nid = _against_the_update(ca, L, arrays, tracks, [0], det, ca.COMMIT_ADD_STAGED, next_id=40)
    assert len(P) == 3 and nid == 42 and result["n_appended"] == 2 and result["next_id"] == 42
    assert Tr["id"].tolist() == [100, 40, 41] and Tr["flags"][1:].tolist() == [ca.MAP_TRACK_STAGED] * 2
    assert Tr["result"][1:].tolist() == [ca.MAP_RESULT_APPENDED] * 2 and not Tr["successive_matched"][1:].any() and not Tr["failed_tracking"][1:].any()
    assert R["vertex_count"][1:].tolist() == [4, 4]  # detections 2 and 3; detection 1's covariance is not valid


def test_the_same_frame_five_times_in_a_row(ca, L):  # noqa: F811
    """each step's output feeds the next, both ways: equal after every step (the polygons grow in the first step and stay)"""
    arrays, tracks, match, det = _five_planes(ca, L)
    next_id = 500
    for step in range(5):
        new, Tr, result, nid = _against_the_update(ca, L, arrays, tracks, match + [-1] * (len(arrays[0]) - 5), det,
                                                   ca.COMMIT_ADD_STAGED if step == 0 else 0, next_id)
        assert result["n_appended"] == (1 if step == 0 else 0), step
        arrays, tracks, next_id = new, Tr, nid
    assert len(arrays[0]) == 6 and next_id == 501
    assert tracks["successive_matched"][:3].tolist() == [8, 0, 5] and tracks["failed_tracking"][[1, 3]].tolist() == [14, 5]


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CAPACITY_ROWS, ids=[c[0] for c in CAPACITY_ROWS])
def test_a_capacity_row_of_the_tables_is_a_host_pair(ca, L, case):  # noqa: F811
    name, rings_a, b = case
    arrays, tracks = _one_plane_map(ca, L, rings_a[0], rings_a[1:])
    inputs = _inputs(ca, L, arrays, tracks, [0], [_det(b, d=1010.0)])
    assert inputs[5][0]["flags"] == ca.UNION_HOST_CAPACITY
    result = _refused(ca, L, arrays, tracks, inputs, ca.COMMIT_ADD_STAGED)
    assert result["flags"] == ca.COMMIT_HOST_PAIR and result["n_host_pairs"] == 1 and result["n_updated"] == 0


def test_a_fusion_row_without_its_frame_fails_the_polygon(ca, L):  # noqa: F811
    arrays, tracks = _map(ca, L, 2)
    det = [_det(_square(-400, 400, -400, 400)), _det(_square(2600, 3400, -400, 400))]
    frame, tres, frows, mrows, worlds, _, _, _ = _inputs(ca, L, arrays, tracks, [0, 1], det)
    frows = frows.copy()
    frows[1]["flags"] &= ~np.uint32(ca.FUSION_FRAME)
    frows[1]["x_axis"] = frows[1]["y_axis"] = frows[1]["center"] = 0
    urows, rrows, polys = ca.host_map_union_cut(arrays, [0, 1], frows, mrows, worlds)
    assert urows[0]["flags"] & ca.UNION_SERVED and urows[1]["map_plane"] == -1
    result = _refused(ca, L, arrays, tracks, (frame, tres, frows, mrows, worlds, urows, rrows, _slab(ca, urows, polys)))
    assert result["flags"] == ca.COMMIT_FAIL_POLYGON and result["n_fail_polygon"] == 1 and result["n_updated"] == 1 and result["n_host_pairs"] == 0


def test_a_full_map_and_one_stageable_detection_is_capacity(ca, L):  # noqa: F811
    arrays, tracks = _map(ca, L, ca.MAP_MAX_PLANES)
    det = [_det(_square(-9000, -8000, 5000, 6000))]
    match = [-1] * ca.MAP_MAX_PLANES
    inputs = _inputs(ca, L, arrays, tracks, match, det)
    result = _refused(ca, L, arrays, tracks, inputs, ca.COMMIT_ADD_STAGED)
    assert result["flags"] == ca.COMMIT_CAPACITY and result["n_appended"] == 1 and result["n_planes"] == ca.MAP_MAX_PLANES
    # without the append the full map commits
    new, Tr, result, _ = ca.host_map_commit(arrays, tracks, *inputs, 0, 0)
    assert result["flags"] == ca.COMMIT_DONE and len(new[0]) == ca.MAP_MAX_PLANES and np.all(Tr["failed_tracking"] == 1)


def test_the_frames_header_refuses_the_frame(ca, L):  # noqa: F811
    arrays, tracks = _map(ca, L, 1)
    inputs = list(_inputs(ca, L, arrays, tracks, [0], [_det(_square(-400, 400, -400, 400))]))
    for bit, want in ((ca.KALMAN_BAD_POSE_COV, ca.COMMIT_BAD_POSE_COV), (ca.MATCH_EXACT_OVERFLOW, ca.COMMIT_FRAME_OVERFLOW)):
        frame = np.array(inputs[0]).copy()
        frame["flags"] |= bit
        assert _refused(ca, L, arrays, tracks, [frame] + inputs[1:])["flags"] & want


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_argument_checks(ca, L):  # noqa: F811
    arrays, tracks = _map(ca, L, 2)
    det = [_det(_square(-400, 400, -400, 400))]
    inputs = _inputs(ca, L, arrays, tracks, [0, -1], det)
    ca.host_map_commit(arrays, tracks, *inputs)
    with pytest.raises(ca.CapeError):
        ca.host_map_commit(arrays, tracks, *inputs, flags=2)  # unknown flag
    with pytest.raises(ca.CapeError):
        ca.host_map_commit(arrays, tracks, *inputs, frame=-1)
    with pytest.raises(ca.CapeError):
        ca.host_map_commit(arrays, tracks[:1], *inputs)  # one track per plane
    with pytest.raises(ca.CapeError):
        ca.host_map_commit(arrays, tracks, inputs[0], inputs[1][:1], *inputs[2:])  # one track result per plane
    with pytest.raises(ca.CapeError):
        ca.host_map_commit(arrays, tracks, *inputs[:4], [], *inputs[5:])  # a world ring per kept plane
    Lh = ca._host_library()
    src, view = ca._map_arrays(arrays, tracks)
    H, out, result, nid = np.zeros(1, ca.FRAME_MAP_KALMAN_DTYPE), ca.cape_host_map(), np.zeros(1, ca.MAP_COMMIT_RESULT_DTYPE), C.c_uint64(0)
    R = np.zeros(2, ca.MAP_TRACK_RESULT_DTYPE)
    R["kept_plane"] = -1
    ok = (C.byref(view), 0, H.ctypes.data, R.ctypes.data, None, None, None, None, None, None, 0, C.byref(nid), C.byref(out), result.ctypes.data)
    assert Lh.cape_host_map_commit(*ok) == ca.CAPE_ERR_CAPACITY and (out.n_planes, out.n_rings, out.n_vertices) == (2, 2, 8)  # no room in map_out
    for k in (0, 2, 3, 11, 12, 13):
        assert Lh.cape_host_map_commit(*(ok[:k] + (None,) + ok[k + 1:])) == -1, k
    H[0]["n_cur"] = 1  # a kept plane needs its rows
    assert Lh.cape_host_map_commit(*ok) == -1

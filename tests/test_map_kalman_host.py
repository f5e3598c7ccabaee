"""cape_host_map_kalman -- the host twin of cape_map_kalman: the state half of cape_host_map_update (Kalman step, triple
normalisation, the frame of the polygon step, counters, decisions, the used rule) on measurement rows instead of detections --
against cape_host_map_update itself on the hand-built cases of tests/test_map_update_host.py, each failure class and each counter
threshold once, the algebra against numpy, and the layout of the three new structs.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_map_update_host import (CTR, D, N, PCC, POSE, X, Y, _c, _det, _map, _p, _pose, _rel, _spd, _square, _unit, np_kalman)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cape_map_upload_tracks", "cape_map_kalman", "cape_copy_map_kalman", "cape_device_map_kalman")


@pytest.fixture(scope="module")
def ca(host_binaries):
    import cape_amd

    cape_amd._host_library()
    return cape_amd


@pytest.fixture(scope="module")
def L(ca):
    L = ca._host_library()
    vp = C.c_void_p
    L.cape_host_covariance_valid.argtypes = [vp, C.c_int]
    L.cape_host_plane_covariance.argtypes = [vp, C.c_double, vp, vp]
    L.cape_host_world_plane_covariance.argtypes = [vp, C.c_double, vp, vp, vp, vp]
    L.cape_host_kalman_update.argtypes = [vp, vp, vp, vp, vp, vp]
    return L


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rows(ca, L, det, T, S):
    """The measurement rows of a frame's detections from the update's own host algebra: cape_host_plane_covariance,
    cape_host_world_plane_covariance, plane_to_world, with cape_map_measure's flags.  The polygon step is to_world_space's: it passes
    when the pose's rotation keeps the polygon's axes unit and orthogonal (every hand-built pose here is either a rotation or far
    from one)."""
    rows = np.zeros(len(det), ca.PLANE_MEASUREMENT_DTYPE)
    T = _c(T)
    for r, d in zip(rows, det):
        n, dd, cov = _c(d[0]), float(d[1]), _c(d[7])
        r["flags"] = ca.MEASURE_KEPT
        if not L.cape_host_covariance_valid(_p(_c(S)), 3):
            r["flags"] |= ca.MEASURE_BAD_POSE_COV
            continue
        planeCov, worldCov, z = np.zeros(16), np.zeros(16), np.zeros(4)
        if not L.cape_host_plane_covariance(_p(n), dd, _p(cov), _p(planeCov)):
            r["flags"] |= ca.MEASURE_FAIL_PLANE_COV
            continue
        if not L.cape_host_world_plane_covariance(_p(n), dd, _p(T), _p(planeCov), _p(_c(S)), _p(worldCov)):
            r["flags"] |= ca.MEASURE_FAIL_WORLD_COV
            continue
        L.cape_host_plane_to_world(_p(n), dd, _p(T), _p(z))
        r["normal"], r["d"], r["covariance"] = z[:3], z[3], worldCov.reshape(4, 4)
        R = T[:3, :3]
        r["flags"] |= ca.MEASURE_STAGEABLE if np.allclose(R @ R.T, np.eye(3), atol=1e-12) else ca.MEASURE_FAIL_POLYGON
    return rows


def _against_the_update(ca, L, arrays, tracks, match, det, T, S):
    """the twin on rows of the host algebra against cape_host_map_update: the new plane and covariance bit for bit, the result bits
    other than OVERFLOW, the counters, used_out.  Returns the twin's (frame, rows, track results)."""
    (P, _, _), Tr, used, _ = ca.host_map_update(arrays, tracks, match, det, T, S)
    frame, rows, res = ca.host_map_kalman(arrays, tracks, match, _rows(ca, L, det, T, S))
    n_map = len(arrays[0])
    assert frame["n_map"] == n_map and frame["n_cur"] == len(det) and frame["flags"] == 0
    assert np.array_equal(res["result"], Tr["result"][:n_map] & ~np.uint32(ca.MAP_RESULT_OVERFLOW))
    assert np.array_equal(res["successive_matched"], Tr["successive_matched"][:n_map])
    assert np.array_equal(res["failed_tracking"], Tr["failed_tracking"][:n_map])
    assert np.array_equal(res["kept_plane"], np.asarray(match, np.int32))
    assert [bool(r["flags"] & ca.FUSION_USED) for r in rows] == used.tolist()
    assert frame["n_updated"] == int(np.count_nonzero(res["result"] & ca.MAP_RESULT_UPDATED))
    for j, i in enumerate(match):
        if i < 0:
            continue
        row = rows[i]
        assert row["map_plane"] == j
        if row["flags"] & ca.FUSION_STATE:
            assert np.array_equal(_bits(row["normal"]), _bits(P[j]["normal"])) and np.array_equal(_bits(row["d"]), _bits(P[j]["d"]))
            assert np.array_equal(_bits(row["covariance"]), _bits(Tr[j]["covariance"]))
        else:
            # nothing changed on the host, nothing is reported here
            assert P[j].tobytes() == arrays[0][j].tobytes() and np.array_equal(Tr[j]["covariance"], tracks[j]["covariance"])
            assert not row["normal"].any() and row["d"] == 0 and not row["covariance"].any() and not row["x_axis"].any()
    assert all(rows[i]["map_plane"] == -1 and rows[i]["flags"] == 0 for i in range(len(det)) if i not in match)
    return frame, rows, res


# ---- the twin against the update on the hand-built cases ---------------------------------------------------------------------
def test_a_matched_plane_equals_the_update(ca, L):
    arrays, tracks = _map(ca, L, 1)
    det = [_det(_square(0, 1000, -500, 500), d=1010.0)]
    frame, rows, res = _against_the_update(ca, L, arrays, tracks, [0], det, np.eye(4), POSE)
    assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED and frame["n_updated"] == 1
    assert rows[0]["flags"] == ca.FUSION_USED | ca.FUSION_STATE | ca.FUSION_FRAME
    assert 1000.0 < rows[0]["d"] < 1010.0
    # the frame the union projects into is the updated map polygon's (the update projects its polygon there)
    (P, _, _), _, _, _ = ca.host_map_update(arrays, tracks, [0], det, np.eye(4), POSE)
    for k in ("x_axis", "y_axis", "center"):
        assert np.array_equal(_bits(rows[0][k]), _bits(P[0][k])), k


def test_the_overflowing_union_is_the_hosts_alone(ca, L):
    arrays, tracks = _map(ca, L, 1)
    t = np.linspace(0, 2 * np.pi, 1100, endpoint=False)
    r = np.where(np.arange(1100) % 2 == 0, 760.0, 720.0)
    comb = np.stack([r * np.cos(-t), r * np.sin(-t)], 1)
    det = [_det(comb, d=1010.0)]
    (_, _, _), Tr, _, _ = ca.host_map_update(arrays, tracks, [0], det, np.eye(4), POSE)
    assert Tr[0]["result"] & ca.MAP_RESULT_OVERFLOW
    _, _, res = _against_the_update(ca, L, arrays, tracks, [0], det, np.eye(4), POSE)
    assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED


def test_counters_and_the_used_rule_equal_the_update(ca, L):
    arrays, tracks = _map(ca, L, 4, staged=(2, 3))
    tracks["successive_matched"] = [2, 2, 3, 0]
    tracks["failed_tracking"] = [0, 9, 0, 1]
    bad = np.full((3, 3), np.nan)
    det = [_det(_square(-400, 400, -400, 400)), _det(_square(2600, 3400, -400, 400), cov=bad),
           _det(_square(5600, 6400, -400, 400)), _det(_square(8600, 9400, -400, 400), cov=bad), _det(_square(0, 10, 0, 10))]
    _, rows, res = _against_the_update(ca, L, arrays, tracks, [0, 1, 2, 3], det, np.eye(4), POSE)
    assert res["result"].tolist() == [ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED,
                                      ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_DETECTION | ca.MAP_RESULT_LOST,
                                      ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED | ca.MAP_RESULT_PROMOTE,
                                      ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_DETECTION | ca.MAP_RESULT_DROP]
    # staged 3 -> 4 promotes, staged failed 1 -> 2 drops, local failed 9 -> 10 is lost
    assert res["successive_matched"].tolist() == [3, 1, 4, -1] and res["failed_tracking"].tolist() == [0, 10, 0, 2]
    # a staged plane marks its detection used when the step failed, a local plane does not
    assert [bool(r["flags"] & ca.FUSION_USED) for r in rows] == [True, False, True, True, False]
    _, rows, res = _against_the_update(ca, L, arrays, tracks, [-1, -1, -1, -1], det, np.eye(4), POSE)
    assert res["result"].tolist() == [0, ca.MAP_RESULT_LOST, 0, ca.MAP_RESULT_DROP] and res["kept_plane"].tolist() == [-1] * 4
    # a permuted match: the rows follow the kept planes, the results the map planes
    _against_the_update(ca, L, arrays, tracks, [2, -1, 0, 4], det, np.eye(4), POSE)


def test_a_translated_pose_equals_the_update(ca, L):
    arrays, tracks = _map(ca, L, 2, staged=(1,))
    rng = np.random.default_rng(2)
    T = np.eye(4)
    T[:3, 3] = [10.0, -20.0, 5.0]
    det = [_det(_square(2600, 3400, -400, 400), cov=_spd(rng, 3, 2.0), d=1003.0), _det(_square(-400, 400, -400, 400), d=996.0)]
    _, rows, res = _against_the_update(ca, L, arrays, tracks, [1, 0], det, T, _spd(rng, 3, 1e-3))
    assert np.all(res["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED)
    assert not np.array_equal(_bits(rows[0]["normal"]), _bits(rows[1]["normal"]))


# ---- each failure class once -----------------------------------------------------------------------------------------------------
def test_failure_classes(ca, L):
    arrays, tracks = _map(ca, L, 1)
    ring = _square(-400, 400, -400, 400)
    FAILS = ca.MAP_RESULT_FAIL_DETECTION | ca.MAP_RESULT_FAIL_STATE | ca.MAP_RESULT_FAIL_SINGULAR | ca.MAP_RESULT_FAIL_KALMAN

    def one(tr, row_edit=None, det=None, T=np.eye(4)):
        rows = _rows(ca, L, det or [_det(ring)], T, POSE)
        if row_edit:
            row_edit(rows[0])
        return ca.host_map_kalman(arrays, tr, [0], rows)

    # an asymmetric track covariance
    bad = tracks.copy()
    bad[0]["covariance"][0, 1] += 1e-3
    _, rows, res = one(bad)
    assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_STATE and rows[0]["flags"] == 0
    _against_the_update(ca, L, arrays, bad, [0], [_det(ring)], np.eye(4), POSE)
    # a measurement row with each CAPE_MEASURE_FAIL_* bit that means "no detection"
    for bit in (ca.MEASURE_FAIL_PLANE_COV, ca.MEASURE_FAIL_WORLD_COV, ca.MEASURE_BAD_POSE_COV):
        def edit(r, bit=bit):
            r["flags"] = ca.MEASURE_KEPT | bit
        frame, rows, res = one(tracks, edit)
        assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_DETECTION, hex(bit)
        assert res[0]["failed_tracking"] == 1 and res[0]["successive_matched"] == -1 and rows[0]["flags"] == 0
        assert frame["flags"] == (ca.KALMAN_BAD_POSE_COV if bit == ca.MEASURE_BAD_POSE_COV else 0)
    # ... as the update's own algebra produces them
    _against_the_update(ca, L, arrays, tracks, [0], [_det(ring, cov=np.full((3, 3), np.inf))], np.eye(4), POSE)
    asym = PCC.copy()
    asym[0, 1] = 5.0
    _, _, res = _against_the_update(ca, L, arrays, tracks, [0], [_det(ring, cov=asym)], np.eye(4), POSE)
    assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_DETECTION
    # a NaN in R: the Kalman step refuses its input (KALMAN_INVALID_INPUT), which the update maps to FAIL_KALMAN
    def nan_r(r):
        r["covariance"][2, 2] = np.nan
    _, rows, res = one(tracks, nan_r)
    assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_KALMAN and rows[0]["flags"] == 0
    # a row with FAIL_POLYGON: the state is still updated
    def no_polygon(r):
        r["flags"] = ca.MEASURE_KEPT | ca.MEASURE_FAIL_POLYGON
    _, rows, res = one(tracks, no_polygon)
    assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_POLYGON and not res[0]["result"] & FAILS
    assert rows[0]["flags"] == ca.FUSION_STATE | ca.FUSION_FRAME and res[0]["failed_tracking"] == 1
    assert not np.array_equal(rows[0]["covariance"], tracks[0]["covariance"]) and rows[0]["covariance"].any()
    # ... as the update reports a pose whose rotation is not orthogonal
    T = np.eye(4)
    T[0, 1] = 0.3
    _, _, res = _against_the_update(ca, L, arrays, tracks, [0], [_det(ring)], T, POSE)
    assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_POLYGON
    # a singular innovation: tiny valid covariances on both sides
    tiny = tracks.copy()
    tiny[0]["covariance"] = 1e-6 * np.eye(4)
    def tiny_r(r):
        r["covariance"] = 1e-6 * np.eye(4)
    _, rows, res = one(tiny, tiny_r)
    assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_SINGULAR and rows[0]["flags"] == 0


def test_a_nan_in_z_follows_the_updates_statements(ca, L):
    """A NaN in z.  kalman_update (host/map_tracking.cpp) validates the two covariances and never looks at x or z, and the new
    covariance does not depend on z: the step returns KALMAN_OK with a NaN state, exactly as inside cape_host_map_update.  So this case
    is NOT FAIL_KALMAN (that class is a NaN in R, above): the NaN normal survives normalize3, fails Polygon::project's unit check and
    the pair ends as FAIL_POLYGON with the (NaN) state reported and no frame."""
    arrays, tracks = _map(ca, L, 1)
    rows = _rows(ca, L, [_det(_square(-400, 400, -400, 400))], np.eye(4), POSE)
    rows[0]["normal"][1] = np.nan
    xo, Po = np.zeros(4), np.zeros(16)
    x = _c(np.append(N, D))
    z = _c(np.append(rows[0]["normal"], rows[0]["d"]))
    assert L.cape_host_kalman_update(_p(x), _p(_c(tracks[0]["covariance"])), _p(z), _p(_c(rows[0]["covariance"])), _p(xo), _p(Po)) == 0
    _, out, res = ca.host_map_kalman(arrays, tracks, [0], rows)
    assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_POLYGON
    assert out[0]["flags"] == ca.FUSION_STATE and np.isnan(out[0]["normal"]).any() and not out[0]["x_axis"].any()
    assert np.array_equal(_bits(out[0]["covariance"]), _bits(Po.reshape(4, 4)))
    assert res[0]["failed_tracking"] == 1 and res[0]["successive_matched"] == -1


# ---- counters at each threshold ------------------------------------------------------------------------------------------------
def test_counter_thresholds(ca, L):
    arrays, tracks = _map(ca, L, 6, staged=(0, 1, 2, 3))
    tracks["successive_matched"] = [3, 2, 0, 0, 5, 5]
    tracks["failed_tracking"] = [0, 0, 1, 0, 9, 8]
    det = [_det(_square(-400, 400, -400, 400) + [3000 * j, 0]) for j in range(2)]
    rows = _rows(ca, L, det, np.eye(4), POSE)
    _, out, res = ca.host_map_kalman(arrays, tracks, [0, 1, -1, -1, -1, -1], rows)
    U, M = ca.MAP_RESULT_UPDATED, ca.MAP_RESULT_MATCHED
    assert res["result"].tolist() == [M | U | ca.MAP_RESULT_PROMOTE, M | U, ca.MAP_RESULT_DROP, 0, ca.MAP_RESULT_LOST, 0]
    assert res["successive_matched"].tolist() == [4, 3, -1, -1, 4, 4] and res["failed_tracking"].tolist() == [0, 0, 2, 1, 10, 9]
    # a staged plane whose step fails still uses its detection; a local plane does not
    arrays, tracks = _map(ca, L, 2, staged=(0,))
    rows["flags"] = ca.MEASURE_KEPT | ca.MEASURE_FAIL_WORLD_COV
    _, out, res = ca.host_map_kalman(arrays, tracks, [0, 1], rows)
    assert [int(r["flags"]) for r in out] == [ca.FUSION_USED, 0]
    assert np.all(res["result"] & ca.MAP_RESULT_FAIL_DETECTION)


# ---- the algebra against numpy ---------------------------------------------------------------------------------------------------
def np_plane_frame(n):
    dist = np.abs(n)
    res = dist.min()
    r = None
    for k in range(3):
        if abs(res - dist[k]) <= 0.1:
            r = np.eye(3)[k]
            break
    if r is None:
        r = np.array([n[2], n[0], n[1]]) / np.linalg.norm(n)
    x = np.cross(n, r)
    x /= np.linalg.norm(x)
    y = np.cross(n, x)
    return x, y / np.linalg.norm(y)


def test_the_state_algebra_matches_numpy(ca, L):
    rng = np.random.default_rng(11)
    arrays, tracks = _map(ca, L, 1)
    P0 = arrays[0].copy()
    for _ in range(200):
        n = _unit(rng)
        x = np.append(n, rng.uniform(-3000, 3000))
        z = x + np.append(rng.normal(scale=0.01, size=3), rng.normal(scale=5))
        P, R = _spd(rng, 4, rng.uniform(1e-3, 1)), _spd(rng, 4, rng.uniform(1e-3, 1))
        P0[0]["normal"], P0[0]["d"] = x[:3], x[3]
        tracks[0]["covariance"] = P
        rows = np.zeros(1, ca.PLANE_MEASUREMENT_DTYPE)
        rows[0]["normal"], rows[0]["d"], rows[0]["covariance"], rows[0]["flags"] = z[:3], z[3], R, ca.MEASURE_KEPT | ca.MEASURE_STAGEABLE
        _, out, res = ca.host_map_kalman((P0, arrays[1], arrays[2]), tracks, [0], rows)
        assert res[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED
        xr, Pr = np_kalman(x, P, z, R)
        nr = xr[:3] / np.linalg.norm(xr[:3])
        assert _rel(out[0]["normal"], nr) < 1e-12 and abs(out[0]["d"] - xr[3]) <= 1e-12 * abs(xr[3])
        assert _rel(out[0]["covariance"], Pr) < 1e-12
        ax, ay = np_plane_frame(out[0]["normal"])
        assert _rel(out[0]["x_axis"], ax) < 1e-12 and _rel(out[0]["y_axis"], ay) < 1e-12
        assert _rel(out[0]["center"], -out[0]["normal"] * out[0]["d"]) < 1e-12
        # an orthonormal, right-handed frame (x, y, n) ... whichever way: y = n x x
        assert abs(ax @ ay) < 1e-12 and abs(out[0]["x_axis"] @ out[0]["normal"]) < 1e-12


def test_the_plane_frame_hook_follows_each_branch(ca, L):
    out = np.zeros(6)
    for n in ([0.05, 0.7, 0.712], [0.7, 0.05, 0.712], [0.7, 0.712, 0.05], [0.5, 0.62, 0.6], [0.0, 0.0, -1.0]):
        n = _c(n) / np.linalg.norm(n)
        assert L.cape_host_plane_frame(_p(n), _p(out)) == 1
        ax, ay = np_plane_frame(n)
        assert _rel(out[:3], ax) < 1e-12 and _rel(out[3:], ay) < 1e-12
    assert L.cape_host_plane_frame(_p(_c([0.0, 0.0, 1.0 + 1e-8])), _p(out)) == 0
    assert L.cape_host_plane_frame(_p(_c([np.nan, 0.0, 1.0])), _p(out)) == 0


def test_argument_checks(ca, L):
    arrays, tracks = _map(ca, L, 2)
    rows = _rows(ca, L, [_det(_square(-400, 400, -400, 400))], np.eye(4), POSE)
    for match in ([0, 1], [0, -2]):
        with pytest.raises(ca.CapeError, match=r"cape_host_map_kalman failed \(-1\)"):
            ca.host_map_kalman(arrays, tracks, match, rows)
    with pytest.raises(ca.CapeError):
        ca.host_map_kalman(arrays, tracks[:1], [0, -1], rows)
    with pytest.raises(ca.CapeError, match=r"cape_host_map_kalman failed \(-1\)"):
        ca.host_map_kalman(arrays, tracks, [-1, -1], np.zeros(129, ca.PLANE_MEASUREMENT_DTYPE))
    # an empty map: a header and unmatched rows
    frame, out, res = ca.host_map_kalman(ca.pack_map([]), np.zeros(0, ca.MAP_TRACK_DTYPE), [], rows)
    assert frame["n_map"] == 0 and frame["n_cur"] == 1 and len(res) == 0 and out[0]["map_plane"] == -1


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
class _FrameMapKalman(C.Structure):
    _fields_ = [("n_map", C.c_int32), ("n_cur", C.c_int32), ("flags", C.c_uint32), ("n_updated", C.c_int32)]


class _PlaneFusion(C.Structure):
    _fields_ = [("normal", C.c_double * 3), ("d", C.c_double), ("covariance", C.c_double * 16), ("x_axis", C.c_double * 3),
                ("y_axis", C.c_double * 3), ("center", C.c_double * 3), ("map_plane", C.c_int32), ("flags", C.c_uint32)]


class _MapTrackResult(C.Structure):
    _fields_ = [("result", C.c_uint32), ("successive_matched", C.c_int32), ("failed_tracking", C.c_uint32), ("kept_plane", C.c_int32)]


class _MapTrack(C.Structure):
    _fields_ = [("covariance", C.c_double * 16), ("successive_matched", C.c_int32), ("failed_tracking", C.c_uint32), ("flags", C.c_uint32),
                ("result", C.c_uint32), ("id", C.c_uint64)]


def _code(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, *path)).read(), flags=re.S)


def test_the_structs_mirror_the_header(hip_library):
    import cape_amd

    code = _code(("include", "cape_hip.h"))
    want = {"cape_frame_map_kalman": ["int32_t n_map, n_cur", "uint32_t flags", "int32_t n_updated"],
            "cape_plane_fusion": ["double normal[3], d", "double covariance[16]", "double x_axis[3], y_axis[3], center[3]", "int32_t map_plane",
                                  "uint32_t flags"],
            "cape_map_track_result": ["uint32_t result", "int32_t successive_matched", "uint32_t failed_tracking", "int32_t kept_plane"],
            "cape_map_track": ["double covariance[16]", "int32_t successive_matched", "uint32_t failed_tracking", "uint32_t flags",
                               "uint32_t result", "uint64_t id"]}
    for name, fields in want.items():
        body = re.search(rf"typedef struct {name}\s*\{{(.*?)\}}\s*{name};", code, re.S).group(1)
        assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == fields, name
    for dt, mirror, size in ((cape_amd.FRAME_MAP_KALMAN_DTYPE, _FrameMapKalman, 16), (cape_amd.PLANE_FUSION_DTYPE, _PlaneFusion, 240),
                             (cape_amd.MAP_TRACK_RESULT_DTYPE, _MapTrackResult, 16), (cape_amd.MAP_TRACK_DTYPE, _MapTrack, 152)):
        assert dt.itemsize == C.sizeof(mirror) == size
        assert dt.names == tuple(name for name, _ in mirror._fields_)
        for name, _ in mirror._fields_:
            assert dt.fields[name][1] == getattr(mirror, name).offset, name
    # the track and its enums moved to the library's header; the host header only uses them
    host = _code(("rgb-d-slam_amd", "host", "cape_host_map.h"))
    assert "typedef struct cape_map_track" not in host and "CAPE_MAP_RESULT_MATCHED" not in host and "cape_map_track* tracks" in host
    assert re.search(r"#define CAPE_ABI_VERSION 2\b", code)
    for bit, name in enumerate(("MATCHED", "UPDATED", "FAIL_DETECTION", "FAIL_STATE", "FAIL_SINGULAR", "FAIL_KALMAN", "FAIL_POLYGON", "OVERFLOW",
                                "PROMOTE", "DROP", "LOST", "APPENDED")):
        assert re.search(rf"CAPE_MAP_RESULT_{name}\s*=\s*1u << {bit}\b", code), name
        assert getattr(cape_amd, f"MAP_RESULT_{name}") == 1 << bit
    for bit, name in enumerate(("USED", "STATE", "FRAME")):
        assert re.search(rf"CAPE_FUSION_{name}\s*=\s*1u << {bit}\b", code) and getattr(cape_amd, f"FUSION_{name}") == 1 << bit
    assert re.search(r"CAPE_KALMAN_BAD_POSE_COV\s*=\s*1u << 8\b", code) and cape_amd.KALMAN_BAD_POSE_COV == 1 << 8
    for value, name in ((11, "KALMAN"), (12, "PLANE_FRAME")):
        assert re.search(rf"CAPE_DEBUG_{name} = {value}\b", code) and cape_amd.DEBUG_OPS[name.lower()] == value


def test_the_entry_points_are_declared_exported_and_check_their_arguments(hip_library):
    import cape_amd

    flat = re.sub(r"\s+", " ", _code(("include", "cape_hip.h")))
    assert "int cape_map_upload_tracks(cape_handle h, const cape_map_track* tracks, int32_t n);" in flat
    assert "int cape_map_kalman(cape_handle h, int32_t n_frames, void* stream);" in flat
    assert ("int cape_copy_map_kalman(cape_handle h, int32_t n_frames, cape_frame_map_kalman* frames, cape_plane_fusion* rows, "
            "cape_map_track_result* track_results);") in flat
    assert ("int cape_device_map_kalman(cape_handle h, cape_frame_map_kalman** frames, cape_plane_fusion** rows, "
            "cape_map_track_result** track_results);") in flat
    lib = cape_amd.load_library()
    assert set(NAMES) <= set(cape_amd.EXPORTED_SYMBOLS)
    # a NULL handle and a negative count are refused before anything touches a device
    assert lib.cape_map_upload_tracks(None, None, 0) == -1
    assert lib.cape_map_kalman(None, 1, None) == -1
    assert lib.cape_copy_map_kalman(None, 0, None, None, None) == -1
    assert lib.cape_device_map_kalman(None, None, None, None) == -1
    ex = object.__new__(cape_amd.Extractor)  # (what a failed cape_create leaves: the library, no handle)
    ex.L, ex.h, ex.max_batch, ex.map_size = lib, None, 1, 0
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_kalman failed \(-1\)"):
        ex.map_kalman(1)
    with pytest.raises(cape_amd.CapeError, match=r"cape_map_upload_tracks failed \(-1\)"):
        ex.upload_tracks(np.zeros(0, cape_amd.MAP_TRACK_DTYPE))
    with pytest.raises(cape_amd.CapeError, match=r"cape_copy_map_kalman failed \(-1\)"):
        ex.map_kalman_rows(1)

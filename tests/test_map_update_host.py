"""cape_host_map_update -- Feature_Map::update_map for one frame on the host class (MapPlane::update_with_match: covariance,
Kalman step and polygon union; the update_matched / update_unmatched counters; the staged appends) -- and its covariance and
Kalman algebra against an independent numpy restatement of the reference's Eigen expressions.  CPU only."""
import ctypes as C

import numpy as np
import pytest


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


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _c(a):
    return np.ascontiguousarray(a, np.float64)


# --- numpy restatement (covariances.cpp:96-226, covariances.hpp:55-64, kalman_filter.hpp) ---------------------------------
def _lower(S):
    return np.tril(S) + np.tril(S, -1).T


def np_propagate(S, J, eps=0.0):
    return _lower(J @ _lower(S) @ J.T) + eps * np.eye(J.shape[0])


def np_plane_covariance(n, d, pcc):
    a, b, c = n * d
    s = a * a + b * b + c * c
    div, com = s ** 1.5, 1 / np.sqrt(s)
    J = np.array([[com - a * a / div, -a * b / div, -a * c / div], [-a * b / div, com - b * b / div, -b * c / div],
                  [-a * c / div, -b * c / div, com - c * c / div], [-a / div, -b / div, -c / div]])
    return np_propagate(pcc, J, 0.01)


def np_world_plane_covariance(n, d, T, planeCov, pose):
    J = np.array([[d, 0, 0, n[0]], [0, d, 0, n[1]], [0, 0, d, n[2]]])
    pcc = np_propagate(planeCov, J, 0.01)
    world = np_propagate(pcc, T[:3, :3]) + pose
    nw, dw = np_plane_to_world(n, d, T)
    return np_plane_covariance(nw, dw, world)


def np_plane_to_world(n, d, T):
    R, t = T[:3, :3], T[:3, 3]
    M = np.eye(4)
    M[:3, :3] = R
    M[3, :3] = -t @ R
    v = M @ np.append(n, d)
    return v[:3] / np.linalg.norm(v[:3]), v[3]


def np_kalman(x, P, z, R):
    E = _lower(P) + 1e-6 * np.eye(4)
    S = E + R
    K = E @ np.linalg.inv(S)
    xn = x + K @ (z - x)
    Pn = _lower((np.eye(4) - K) @ E)
    return xn, Pn


def _spd(rng, n, scale):
    A = rng.normal(size=(n, n))
    return scale * (A @ A.T + n * np.eye(n))


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _rot(rng, max_angle):
    ax = _unit(rng)
    t = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _pose(rng):
    T = np.eye(4)
    T[:3, :3] = _rot(rng, 0.6)
    T[:3, 3] = rng.uniform(-500, 500, 3)
    return T


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def test_covariance_algebra_matches_numpy(L):
    rng = np.random.default_rng(3)
    for _ in range(200):
        n, d = _unit(rng), rng.uniform(300, 4000) * rng.choice([-1, 1])
        pcc = _c(_spd(rng, 3, rng.uniform(0.1, 30)))
        out = np.zeros(16)
        assert L.cape_host_plane_covariance(_p(n), d, _p(pcc), _p(out)) == 1
        assert _rel(out.reshape(4, 4), np_plane_covariance(n, d, pcc)) < 1e-12
        T, pose = _c(_pose(rng)), _c(_spd(rng, 3, 1e-3))
        w = np.zeros(16)
        assert L.cape_host_world_plane_covariance(_p(n), d, _p(T), _p(out), _p(pose), _p(w)) == 1
        assert _rel(w.reshape(4, 4), np_world_plane_covariance(n, d, T, out.reshape(4, 4), pose)) < 1e-12
        # the 0.01 diagonal keeps every eigenvalue >= 0.01: an innovation with this as measurement noise is never singular
        assert np.linalg.eigvalsh(w.reshape(4, 4)).min() > 0.01 - 1e-12


def test_kalman_step_matches_numpy(L):
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = _unit(rng)
        x = _c(np.append(n, rng.uniform(-3000, 3000)))
        z = _c(x + np.append(rng.normal(scale=0.01, size=3), rng.normal(scale=5)))
        P, R = _c(_spd(rng, 4, rng.uniform(1e-4, 1))), _c(_spd(rng, 4, rng.uniform(1e-4, 1)))
        xo, Po = np.zeros(4), np.zeros(16)
        assert L.cape_host_kalman_update(_p(x), _p(P), _p(z), _p(R), _p(xo), _p(Po)) == 0
        xr, Pr = np_kalman(x, P, z, R)
        assert _rel(xo, xr) < 1e-12
        assert _rel(Po.reshape(4, 4), Pr) < 1e-12
        assert np.array_equal(Po.reshape(4, 4), Po.reshape(4, 4).T)  # the final selfadjointView<Lower>


def test_covariance_validity(L):
    rng = np.random.default_rng(7)
    for n in (3, 4):
        A = _c(_spd(rng, n, 1.0))
        assert L.cape_host_covariance_valid(_p(A), n) == 1
        B = A.copy()
        B[0, 1] += 1e-3  # not symmetric
        assert L.cape_host_covariance_valid(_p(_c(B)), n) == 0
        C_ = A.copy()
        C_[n - 1, n - 1] = -5.0  # indefinite
        assert L.cape_host_covariance_valid(_p(_c(C_)), n) == 0
        D = A.copy()
        D[1, 1] = np.nan
        assert L.cape_host_covariance_valid(_p(_c(D)), n) == 0
        assert L.cape_host_covariance_valid(_p(_c(np.zeros((n, n)))), n) == 0  # an all-zero diagonal: NumericalIssue
    x, z = _c([0, 0, 1, -1000.0]), _c([0, 0, 1, -990.0])
    xo, Po = np.full(4, 7.0), np.full(16, 7.0)
    # a measurement covariance that is not valid (negative definite): KALMAN_INVALID_INPUT
    P, R = _c(np.eye(4)), _c(-1e-6 * np.eye(4))
    assert L.cape_host_kalman_update(_p(x), _p(P), _p(z), _p(R), _p(xo), _p(Po)) == 1
    # valid but tiny covariances: the innovation 3e-6 I has a determinant of 8.1e-23, 0 within DBL_EPSILON, where the reference
    # takes a pseudo-inverse -- KALMAN_SINGULAR, and nothing is written
    P, R = _c(1e-6 * np.eye(4)), _c(1e-6 * np.eye(4))
    assert L.cape_host_covariance_valid(_p(P), 4) == 1 and L.cape_host_covariance_valid(_p(R), 4) == 1
    assert L.cape_host_kalman_update(_p(x), _p(P), _p(z), _p(R), _p(xo), _p(Po)) == 2
    assert np.all(xo == 7.0) and np.all(Po == 7.0)
    # the same innovation scaled by 1e3 is far from singular
    P, R = _c(1e-3 * np.eye(4)), _c(1e-3 * np.eye(4))
    assert L.cape_host_kalman_update(_p(x), _p(P), _p(z), _p(R), _p(xo), _p(Po)) == 0


# --- the update loop on hand-built maps ----------------------------------------------------------------------------------
N, D = np.array([0.0, 0.0, -1.0]), 1000.0  # the plane z = 1000 mm, seen head-on from the origin
X, Y, CTR = np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1000.0])
PCC = np.diag([20.0, 20.0, 4.0])
POSE = 1e-4 * np.eye(3)


def _square(x0, x1, y0, y1):
    return np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]], np.float64)


def _map(ca, L, n_planes, staged=(), holes=()):
    cov = np.zeros(16)
    assert L.cape_host_plane_covariance(_p(N), D, _p(_c(PCC)), _p(cov)) == 1
    planes = [(N, D, X, Y, CTR, _square(-500, 500, -500, 500) + [3000 * j, 0], list(holes)) for j in range(n_planes)]
    tracks = np.zeros(n_planes, ca.MAP_TRACK_DTYPE)
    for j in range(n_planes):
        tracks[j]["covariance"] = cov.reshape(4, 4)
        tracks[j]["id"] = 100 + j
        tracks[j]["flags"] = ca.MAP_TRACK_STAGED if j in staged else 0
    return ca.pack_map(planes), tracks


def _det(ring, cov=PCC, d=D):
    return (N, d, X, Y, CTR, ring, None, np.asarray(cov, np.float64))


def _area(ring):
    x, y = ring[:, 0], ring[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def test_matched_plane_fuses_parameters_covariance_and_polygon(ca, L):
    arrays, tracks = _map(ca, L, 1)
    det = [_det(_square(0, 1000, -500, 500), d=1010.0)]
    (P, R, V), Tr, used, nid = ca.host_map_update(arrays, tracks, [0], det, np.eye(4), POSE, 0, next_id=7)
    assert len(P) == 1 and nid == 7 and used.tolist() == [True]
    assert Tr[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED
    assert Tr[0]["successive_matched"] == 1 and Tr[0]["failed_tracking"] == 0 and Tr[0]["id"] == 100
    assert 1000.0 < P[0]["d"] < 1010.0  # the Kalman step moves d toward the detection
    assert abs(np.linalg.norm(P[0]["normal"]) - 1) < 1e-15
    assert np.all(np.diag(Tr[0]["covariance"]) < np.diag(tracks[0]["covariance"]))  # the fused estimate is surer
    # the merged outline: the union of the two squares, 1.5 m^2, in the new plane's frame
    outer = V[R[P[0]["ring_first"]]["vertex_offset"]:][: R[P[0]["ring_first"]]["vertex_count"]]
    assert P[0]["ring_count"] == 1
    assert abs(_area(outer) - 1.5e6) < 1e-3
    assert np.allclose(P[0]["center"], -P[0]["normal"] * P[0]["d"], rtol=0, atol=1e-9)
    # the result is a valid map: it matches the detection again
    m, _ = ca.host_match_map((P, R, V), [d[:7] for d in det], flags=ca.MATCH_ALLOW_INDEX0)
    assert m.tolist() == [0]


def test_counters_and_the_used_rule(ca, L):
    # planes 0, 1 local, 2, 3 staged; plane 0 and 2 take a detection they can use, plane 1 and 3 one whose covariance is invalid
    arrays, tracks = _map(ca, L, 4, staged=(2, 3))
    tracks["successive_matched"] = [2, 2, 3, 0]
    tracks["failed_tracking"] = [0, 9, 0, 1]
    bad = np.full((3, 3), np.nan)
    det = [_det(_square(-400, 400, -400, 400)), _det(_square(2600, 3400, -400, 400), cov=bad),
           _det(_square(5600, 6400, -400, 400)), _det(_square(8600, 9400, -400, 400), cov=bad), _det(_square(0, 10, 0, 10))]
    (P, R, V), Tr, used, _ = ca.host_map_update(arrays, tracks, [0, 1, 2, 3], det, np.eye(4), POSE)
    res = Tr["result"]
    assert res[0] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED
    assert res[1] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_DETECTION | ca.MAP_RESULT_LOST
    assert res[2] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED | ca.MAP_RESULT_PROMOTE
    assert res[3] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_DETECTION | ca.MAP_RESULT_DROP
    assert Tr["successive_matched"].tolist() == [3, 1, 4, -1]
    assert Tr["failed_tracking"].tolist() == [0, 10, 0, 2]
    # a local plane uses its detection only on success, a staged plane either way (feature_map.hpp:790-797)
    assert used.tolist() == [True, False, True, True, False]
    # a failed update changes neither the plane nor its polygon
    assert P[1].tobytes() == arrays[0][1].tobytes()
    assert np.array_equal(Tr[1]["covariance"], tracks[1]["covariance"])
    # an unmatched plane only counts
    (P2, _, _), Tr2, _, _ = ca.host_map_update(arrays, tracks, [-1, -1, -1, -1], det, np.eye(4), POSE)
    assert Tr2["result"].tolist() == [0, ca.MAP_RESULT_LOST, 0, ca.MAP_RESULT_DROP]
    assert Tr2["failed_tracking"].tolist() == [1, 10, 1, 2] and Tr2["successive_matched"].tolist() == [1, 1, 2, -1]
    assert P2.tobytes() == arrays[0].tobytes()


def test_staged_appends(ca, L):
    arrays, tracks = _map(ca, L, 1)
    T = np.eye(4)
    T[:3, 3] = [10.0, -20.0, 5.0]
    det = [_det(_square(-400, 400, -400, 400)), _det(_square(2000, 2500, 0, 500)), _det(_square(-3000, -2500, 0, 400))]
    for flags in (0, ca.MAP_ADD_STAGED):
        (P, R, V), Tr, used, nid = ca.host_map_update(arrays, tracks, [0], det, T, POSE, flags, next_id=40)
        assert used.tolist() == [True, False, False]
        if not flags:
            assert len(P) == 1 and nid == 40
            continue
        assert len(P) == 3 and nid == 42
        assert Tr["id"].tolist() == [100, 40, 41]
        assert Tr["flags"][1:].tolist() == [ca.MAP_TRACK_STAGED] * 2
        assert Tr["result"][1:].tolist() == [ca.MAP_RESULT_APPENDED] * 2
        assert Tr["successive_matched"][1:].tolist() == [0, 0] and Tr["failed_tracking"][1:].tolist() == [0, 0]
        for k, i in ((1, 1), (2, 2)):
            # StagedMapPlane: world parameters and covariance of the detection
            nw, dw = np_plane_to_world(N, D, T)
            assert np.allclose(P[k]["normal"], nw, atol=1e-15) and abs(P[k]["d"] - dw) < 1e-9
            planeCov = np_plane_covariance(N, D, PCC)
            assert _rel(Tr[k]["covariance"], np_world_plane_covariance(N, D, T, planeCov, POSE)) < 1e-12
            ring = V[R[P[k]["ring_first"]]["vertex_offset"]:][: R[P[k]["ring_first"]]["vertex_count"]]
            assert abs(_area(ring) - _area(det[i][5])) < 1e-6
            assert np.allclose(P[k]["center"], CTR + T[:3, 3])


def test_failed_updates(ca, L):
    arrays, tracks = _map(ca, L, 1)
    ring = _square(-400, 400, -400, 400)
    # a singular detection covariance: the plane covariance is still regularised by the 0.01 diagonal, a NaN one is not
    (_, _, _), Tr, _, _ = ca.host_map_update(arrays, tracks, [0], [_det(ring, cov=np.full((3, 3), np.inf))], np.eye(4), POSE)
    assert Tr[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_DETECTION
    # a non-symmetric point-cloud covariance
    asym = PCC.copy()
    asym[0, 1] = 5.0
    (_, _, _), Tr, _, _ = ca.host_map_update(arrays, tracks, [0], [_det(ring, cov=asym)], np.eye(4), POSE)
    assert Tr[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_DETECTION
    # the map plane's own covariance is invalid
    bad = tracks.copy()
    bad[0]["covariance"] = -np.eye(4)
    (P, _, _), Tr, _, _ = ca.host_map_update(arrays, bad, [0], [_det(ring)], np.eye(4), POSE)
    assert Tr[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_STATE
    assert P.tobytes() == arrays[0].tobytes()
    # a pose whose rotation is not orthogonal: to_world_space refuses the detected polygon after the Kalman step
    # (update_boundary_polygon throws inside track: the parameters are updated, the update reports failure)
    T = np.eye(4)
    T[0, 1] = 0.3
    (P, R, V), Tr, used, _ = ca.host_map_update(arrays, tracks, [0], [_det(ring)], T, POSE)
    assert Tr[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_FAIL_POLYGON
    assert Tr[0]["failed_tracking"] == 1 and used.tolist() == [False]
    assert not np.array_equal(Tr[0]["covariance"], tracks[0]["covariance"])


def test_ring_overflow_keeps_the_old_polygon(ca, L):
    arrays, tracks = _map(ca, L, 1)
    # a star of 1 100 vertices around the map polygon: simplify keeps every spike, beyond CAPE_MAP_MAX_RING
    t = np.linspace(0, 2 * np.pi, 1100, endpoint=False)
    r = np.where(np.arange(1100) % 2 == 0, 760.0, 720.0)
    comb = np.stack([r * np.cos(-t), r * np.sin(-t)], 1)
    (P, R, V), Tr, used, _ = ca.host_map_update(arrays, tracks, [0], [_det(comb, d=1010.0)], np.eye(4), POSE)
    assert Tr[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED | ca.MAP_RESULT_OVERFLOW
    assert used.tolist() == [True]
    assert P[0]["d"] != arrays[0][0]["d"]  # the parameters follow the detection
    for k in ("x_axis", "y_axis", "center"):
        assert np.array_equal(P[0][k], arrays[0][0][k])
    assert R[0]["vertex_count"] == 4 and abs(_area(V) - 1e6) < 1e-6


def test_holes_survive_a_disjoint_update(ca, L):
    hole = _square(-100, 100, -100, 100)[::-1]
    arrays, tracks = _map(ca, L, 1, holes=[hole])
    # a detection that overlaps the outline but not the hole: the hole stays
    (P, R, V), Tr, _, _ = ca.host_map_update(arrays, tracks, [0], [_det(_square(300, 1200, -500, 500))], np.eye(4), POSE)
    assert Tr[0]["result"] == ca.MAP_RESULT_MATCHED | ca.MAP_RESULT_UPDATED
    assert P[0]["ring_count"] == 2
    # a detection that covers the hole fills it
    (P, R, V), Tr, _, _ = ca.host_map_update(arrays, tracks, [0], [_det(_square(-300, 300, -300, 300))], np.eye(4), POSE)
    assert P[0]["ring_count"] == 1


def test_argument_checks(ca, L):
    arrays, tracks = _map(ca, L, 2)
    det = [_det(_square(-400, 400, -400, 400))]
    with pytest.raises(ca.CapeError):
        ca.host_map_update(arrays, tracks, [0, 1], det, np.eye(4), POSE)  # match beyond the kept planes
    with pytest.raises(ca.CapeError):
        ca.host_map_update(arrays, tracks, [0, -2], det, np.eye(4), POSE)
    with pytest.raises(ca.CapeError):
        ca.host_map_update(arrays, tracks, [0, -1], det, np.eye(4), -np.eye(3))  # invalid pose covariance
    with pytest.raises(ca.CapeError):
        ca.host_map_update(arrays, tracks[:1], [0, -1], det, np.eye(4), POSE)  # one track per plane
    with pytest.raises(ca.CapeError):
        ca.host_map_update(arrays, tracks, [0, -1], det, np.eye(4), POSE, flags=8)  # unknown flag
    with pytest.raises(ca.CapeError):
        ca.host_map_update(arrays, tracks, [0, -1], [_det(_square(0, 1, 0, 1)[:2])], np.eye(4), POSE)  # a 2-vertex ring
    P, R, V = arrays
    R2 = R.copy()
    R2[1]["vertex_offset"] = 10 ** 6
    with pytest.raises(ca.CapeError):
        ca.host_map_update((P, R2, V), tracks, [0, -1], det, np.eye(4), POSE)

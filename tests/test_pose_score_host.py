"""cape_host_pose_score, the host twin of cape_map_pose_score, against a numpy restatement of the reference's plane cost function
(PlaneOptimizationFeature, map_primitive.cpp:15-85) written here: plane_to_camera, get_signed_distance through angle_distance,
is_inlier with the float thresholds widened to double, get_reduced_signed_distance, the LM residual and the score, in pair order.
Everything but the three angle parts must agree bit for bit (Python floats are IEEE doubles without contraction); the angle parts go
through the same C library from both sides and get two ulp.  CPU only."""
import math

import numpy as np
import pytest

WP = 128
THR_ANGLE = float(np.float32(0.2))     # parameters.hpp:27-30: constexpr float, widened to double where is_inlier compares
THR_DISTANCE = float(np.float32(50.0))
THIRD = 1.0 / 3


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _bits_nan(a):
    """bit patterns with every NaN as one pattern (which NaN an invalid operation generates is the hardware's choice)"""
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return b


def _ulps(a, b):
    """distance in representable doubles between same-signed finite values (0 for equal bits, +0 and -0 included)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia[ia < 0] = np.int64(-2**63) - ia[ia < 0]
    ib[ib < 0] = np.int64(-2**63) - ib[ib < 0]
    return np.abs(ia - ib)


def plane_to_camera(T, n, d):
    """plane_coordinates.cpp:20-24 as the project states it (utils::plane_to_camera): the rotated normal, normalised; d through the
    last row -t^T R of the plane matrix"""
    T = [float(v) for v in np.asarray(T, np.float64).reshape(16)]
    n0, n1, n2 = (float(v) for v in n)
    r = [(T[4 * i] * n0 + T[4 * i + 1] * n1) + T[4 * i + 2] * n2 for i in range(3)]
    t0, t1, t2 = T[3], T[7], T[11]
    m = [-((t0 * T[k] + t1 * T[4 + k]) + t2 * T[8 + k]) for k in range(3)]
    qd = ((m[0] * n0 + m[1] * n1) + m[2] * n2) + float(d)
    nn = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if nn > 0:
        r = [v / nn for v in r]
    return r, qd


def restate(planes, cov_diag, match, detected, poses, frame_flags=0):
    """the reference's statements for one frame: (scores as dicts, pairs [(j, i)], residuals[h][k] = signed[4] + reduced[3])"""
    pairs = [] if frame_flags & 1 else [(j, int(i)) for j, i in enumerate(match) if i >= 0]
    n_invalid = 0
    for j, i in pairs:
        vals = list(detected[i]) + list(planes[j])
        std = [math.sqrt(v) if v >= 0 else float("nan") for v in cov_diag[j]]
        if any(math.isnan(v) for v in vals) or any(math.isnan(s) or s < 0 for s in std):
            n_invalid += 1
    scores, residuals = [], []
    for T in poses:
        score = sum_sq = 0.0
        n_inliers, words, rows = 0, [0, 0, 0, 0], []
        for j, i in pairs:
            cn, cd = [float(v) for v in detected[i][:3]], float(detected[i][3])
            qn, qd = plane_to_camera(T, planes[j][:3], planes[j][3])
            signed = [math.atan2(math.sin(cn[c] - qn[c]), math.cos(cn[c] - qn[c])) for c in range(3)] + [cd - qd]
            reduced = [cd * cn[c] - qd * qn[c] for c in range(3)]
            for c in range(3):
                r = reduced[c] * 1.0 / 3.0
                sum_sq += r * r
            if all(abs(signed[c]) <= THR_ANGLE for c in range(3)) and abs(signed[3]) <= THR_DISTANCE:
                n_inliers += 1
                score += THIRD
                words[i >> 5] |= 1 << (i & 31)
            rows.append(signed + reduced)
        scores.append(dict(n_pairs=len(pairs), n_inliers=n_inliers, n_invalid=n_invalid, flags=(frame_flags & 1) | (256 if n_invalid else 0),
                           score=score, sum_sq=sum_sq, inlier_words=words))
        residuals.append(rows)
    return scores, pairs, residuals


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _pose(rng, angle=0.3, shift=500.0):
    """a rigid world-to-camera matrix: a rotation of up to `angle` rad about a random axis, a translation of up to `shift` mm"""
    k, a = _unit(rng), rng.uniform(-angle, angle)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    T[:3, 3] = rng.uniform(-shift, shift, 3)
    return T


def _map(rng, n):
    """n map planes (normal, d), their tracks with a positive covariance diagonal, as host_pose_score takes them"""
    import cape_amd

    planes = np.array([[*_unit(rng), rng.uniform(-4000, 4000)] for _ in range(n)]).reshape(n, 4)
    P = np.zeros(n, cape_amd.MAP_PLANE_DTYPE)
    P["normal"], P["d"] = planes[:, :3], planes[:, 3]
    tracks = np.zeros(n, cape_amd.MAP_TRACK_DTYPE)
    for j in range(n):
        tracks[j]["covariance"] = np.diag(rng.uniform(1e-6, 4.0, 4))
        tracks[j]["id"] = 1000 + 7 * j
    arrays = (P, np.zeros(0, cape_amd.MAP_RING_DTYPE), np.zeros((0, 2)))
    return planes, arrays, tracks


def _cov_diag(tracks):
    return [[float(t["covariance"][c, c]) for c in range(4)] for t in tracks]


def check_against_restatement(scores, features, residuals, want_scores, pairs, want_res, planes, tracks, detected, angle_ulps=2):
    """the twin's (or the device's) three outputs of one frame against restate()'s; returns the worst ulp distance of an angle part"""
    worst = 0
    n_pairs = len(pairs)
    for k, (j, i) in enumerate(pairs):
        F = features[k]
        assert (F["map_index"], F["kept_plane"], F["map_id"]) == (j, i, tracks[j]["id"])
        assert np.array_equal(_bits(F["matched"]), _bits(detected[i])) and np.array_equal(_bits(F["map_plane"]), _bits(planes[j]))
        with np.errstate(invalid="ignore"):
            std = np.sqrt(np.array([tracks[j]["covariance"][c, c] for c in range(4)]))
        assert np.array_equal(_bits_nan(F["stddev"]), _bits_nan(std))
    assert not features[n_pairs:].view(np.uint8).any(), "rows beyond n_pairs"
    for h, want in enumerate(want_scores):
        S = scores[h]
        for name in ("n_pairs", "n_inliers", "n_invalid", "flags"):
            assert int(S[name]) == want[name], f"hypothesis {h}: {name} {int(S[name])} != {want[name]}"
        assert list(S["inlier_words"]) == want["inlier_words"], f"hypothesis {h}"
        assert _bits(S["score"]) == _bits(want["score"]), f"hypothesis {h}: score"
        nan = math.isnan(want["sum_sq"])
        assert (math.isnan(S["sum_sq"]) if nan else _bits(S["sum_sq"]) == _bits(want["sum_sq"])), f"hypothesis {h}: sum_sq"
        if residuals is not None and n_pairs:
            got, ref = residuals[h, :n_pairs], np.array(want_res[h]).reshape(n_pairs, 7)
            fin = np.isfinite(ref)
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            assert np.array_equal(_bits(got[:, 3:])[fin[:, 3:]], _bits(ref[:, 3:])[fin[:, 3:]]), f"hypothesis {h}: signed[3] / reduced"
            if fin[:, :3].any():
                u = _ulps(got[:, :3][fin[:, :3]], ref[:, :3][fin[:, :3]])
                worst = max(worst, int(u.max()))
                assert u.max() <= angle_ulps, f"hypothesis {h}: an angle part is {int(u.max())} ulp from the restatement"
            assert not residuals[h, n_pairs:].any()
    return worst


@pytest.fixture(scope="module")
def host(host_binaries):
    import cape_amd

    return cape_amd


def test_a_detection_that_is_its_map_plane_has_zero_distances(host):
    rng = np.random.default_rng(3)
    n = 23
    planes, arrays, tracks = _map(rng, n)
    T = _pose(rng)
    detected = np.array([[*q, d] for q, d in (plane_to_camera(T, p[:3], p[3]) for p in planes)])
    match = np.arange(n, dtype=np.int32)
    scores, features, res = host.host_pose_score(arrays, tracks, match, detected, T[None])
    assert not res[0, :n].any() and np.array_equal(_bits(res[0, :n]), np.zeros((n, 7), np.uint64)), "signed == 0 and reduced == 0, to the bit"
    want = 0.0
    for _ in range(n):
        want += THIRD
    S = scores[0]
    assert S["n_pairs"] == S["n_inliers"] == n and S["n_invalid"] == 0 and S["flags"] == 0 and S["sum_sq"] == 0.0
    assert _bits(S["score"]) == _bits(want)
    assert list(S["inlier_words"]) == [(1 << n) - 1, 0, 0, 0]
    ws, pairs, wr = restate(planes, _cov_diag(tracks), match, detected, T[None])
    check_against_restatement(scores, features, res, ws, pairs, wr, planes, tracks, detected)


@pytest.mark.parametrize("part", range(4))
def test_each_threshold_is_straddled(host, part):
    """signed[part] at thr (1 -+ 1e-9): below is an inlier, above an outlier; the other three parts are exactly 0"""
    rng = np.random.default_rng(40 + part)
    planes, arrays, tracks = _map(rng, 1)
    T = _pose(rng)
    qn, qd = plane_to_camera(T, planes[0][:3], planes[0][3])
    thr = THR_DISTANCE if part == 3 else THR_ANGLE
    assert thr == (50.0 if part == 3 else 0.20000000298023224)
    seen = []
    for sign in (1.0, -1.0):
        for side in (-1e-9, 1e-9):
            det = np.array([[*qn, qd]])
            det[0, part] += sign * thr * (1 + side)
            scores, _, res = host.host_pose_score(arrays, tracks, np.zeros(1, np.int32), det, T[None])
            value = res[0, 0, part]
            assert abs(abs(value) / thr - (1 + side)) < 1e-12 and np.sign(value) == sign, value
            assert not res[0, 0, [c for c in range(4) if c != part]].any()
            inlier = side < 0
            assert scores[0]["n_inliers"] == int(inlier) and list(scores[0]["inlier_words"]) == [int(inlier), 0, 0, 0]
            assert _bits(scores[0]["score"]) == _bits(THIRD if inlier else 0.0)
            ws, pairs, wr = restate(planes, _cov_diag(tracks), [0], det, T[None])
            check_against_restatement(scores, _, res, ws, pairs, wr, planes, tracks, det)
            seen.append(inlier)
    assert seen == [True, False, True, False]


def test_invalid_features_are_flagged_and_still_scored(host):
    rng = np.random.default_rng(5)
    n = 6
    planes, arrays, tracks = _map(rng, n)
    poses = np.stack([_pose(rng, 0.02, 30.0) for _ in range(3)])
    detected = np.array([[*q, d] for q, d in (plane_to_camera(poses[0], p[:3], p[3]) for p in planes)])
    match = np.array([2, -1, 0, 5, -1, 1], np.int32)
    base, _, base_res = host.host_pose_score(arrays, tracks, match, detected, poses)
    assert base[0]["n_invalid"] == 0 and base[0]["n_pairs"] == 4 and not base["flags"].any()
    cases = [("matched", c) for c in range(4)] + [("map", c) for c in range(4)] + [("cov_nan", c) for c in range(4)] + [("cov_neg", c) for c in range(4)]
    for kind, c in cases:
        P, tr, det = arrays[0].copy(), tracks.copy(), detected.copy()
        pl = planes.copy()
        if kind == "matched":
            det[5, c] = np.nan  # kept plane 5 is matched to map plane 3
        elif kind == "map":
            pl[3, c] = np.nan
            P["normal"], P["d"] = pl[:, :3], pl[:, 3]
        else:
            tr[3]["covariance"][c, c] = np.nan if kind == "cov_nan" else -1e-3
        scores, features, res = host.host_pose_score((P, arrays[1], arrays[2]), tr, match, det, poses)
        assert np.all(scores["n_invalid"] == 1) and np.all(scores["flags"] == host.POSE_SCORE_INVALID_FEATURE), (kind, c)
        assert np.all(scores["n_pairs"] == 4), "the invalid pair is still a pair"
        ws, pairs, wr = restate(pl, _cov_diag(tr), match, det, poses)
        check_against_restatement(scores, features, res, ws, pairs, wr, pl, tr, det)
        if kind.startswith("cov"):  # the standard deviations enter no distance: every figure is the valid frame's
            for name in ("n_inliers", "score", "sum_sq", "inlier_words"):
                assert np.array_equal(scores[name], base[name]), (kind, c, name)
            assert np.array_equal(_bits(res), _bits(base_res))
            assert np.isnan(features[2]["stddev"][c]) and features[2]["map_index"] == 3
        else:  # the NaN makes the pair an outlier under every pose; the other pairs keep their residual rows
            assert not np.any(scores["inlier_words"][:, 0] & (1 << 5))
            keep = [k for k in range(4) if k != 2]
            assert np.array_equal(_bits(res[:, keep]), _bits(base_res[:, keep]))
            assert np.isnan(res[:, 2]).any()


def test_pair_order_follows_the_map_not_the_kept_planes(host):
    rng = np.random.default_rng(8)
    n = 40
    planes, arrays, tracks = _map(rng, n)
    poses = np.stack([_pose(rng, 0.05, 80.0) for _ in range(5)])
    perm = rng.permutation(n).astype(np.int32)
    detected = np.zeros((n, 4))
    for j in range(n):
        q, d = plane_to_camera(poses[0], planes[j][:3], planes[j][3])
        detected[perm[j]] = [*q, d]
    match = perm.copy()
    match[::5] = -1
    scores, features, res = host.host_pose_score(arrays, tracks, match, detected, poses)
    ws, pairs, wr = restate(planes, _cov_diag(tracks), match, detected, poses)
    check_against_restatement(scores, features, res, ws, pairs, wr, planes, tracks, detected)
    k = len(pairs)
    assert list(features[:k]["map_index"]) == sorted(features[:k]["map_index"]) and list(features[:k]["kept_plane"]) == [i for _, i in pairs]
    assert list(features[:k]["kept_plane"]) != sorted(features[:k]["kept_plane"])
    # summed in kept-plane order the squares give other bits: the order is observable
    differs = 0
    for h in range(1, len(poses)):
        by_kept = 0.0
        for kk in np.argsort(features[:k]["kept_plane"]):
            for c in range(3):
                r = wr[h][kk][4 + c] * 1.0 / 3.0
                by_kept += r * r
        differs += int(np.float64(by_kept).tobytes() != np.float64(scores[h]["sum_sq"]).tobytes())
    assert differs >= 1
    assert 0 < scores[1]["n_inliers"] and any(s["n_inliers"] < k for s in scores), "inliers and outliers both occur"


def test_a_flagged_frame_an_empty_map_and_the_argument_checks(host):
    import ctypes as C

    rng = np.random.default_rng(9)
    planes, arrays, tracks = _map(rng, 4)
    poses = np.stack([_pose(rng) for _ in range(3)])
    detected = np.array([[*_unit(rng), 100.0 * k] for k in range(4)])
    match = np.arange(4, dtype=np.int32)
    scores, features, res = host.host_pose_score(arrays, tracks, match, detected, poses, frame_flags=host.MATCH_EXACT_OVERFLOW)
    assert np.all(scores["flags"] == host.MATCH_EXACT_OVERFLOW) and not features.view(np.uint8).any() and not res.any()
    for name in ("n_pairs", "n_inliers", "n_invalid", "score", "sum_sq", "inlier_words"):
        assert not np.any(scores[name]), name
    _, empty, no_tracks = _map(rng, 0)
    scores, features, res = host.host_pose_score(empty, no_tracks, np.zeros(0, np.int32), detected, poses)
    assert not scores.view(np.uint8).any() and not features.view(np.uint8).any() and not res.any() and len(scores) == 3
    # no kept plane at all
    scores, _, _ = host.host_pose_score(arrays, tracks, np.full(4, -1, np.int32), np.zeros((0, 4)), poses)
    assert not scores.view(np.uint8).any()
    with pytest.raises(host.CapeError, match=r"\(-1\)"):
        host.host_pose_score(arrays, tracks, np.array([0, 1, 2, 4], np.int32), detected, poses)  # a match out of range
    with pytest.raises(host.CapeError, match=r"\(-1\)"):
        host.host_pose_score(arrays, tracks, match, detected, poses, frame_flags=2)  # an unknown frame flag
    with pytest.raises(host.CapeError, match=r"\(-1\)"):
        host.host_pose_score(arrays, tracks, match, detected, np.zeros((0, 4, 4)))  # no hypothesis
    with pytest.raises(host.CapeError, match=r"\(-1\)"):
        host.host_pose_score(arrays, tracks, np.full(4, -1, np.int32), np.zeros((129, 4)), poses)  # more than 128 kept planes
    assert host._host_library().cape_host_pose_score(None, None, None, 0, 1, None, None, None, None) == -1
    assert C.sizeof(C.c_double) == 8

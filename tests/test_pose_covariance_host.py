"""cape_host_pose_covariance and cape_host_pose_draw_deviates, the host twins of cape_map_pose_covariance and cape_pose_draw_deviates,
without a device, and the single statements of csrc/cape_pose_covariance.h they are made of.

Philox4x32-10 is held to the published known answers and to an independent numpy restatement written here (the uniforms must be equal;
the normals go through two different log / cos / sin and agree within NORMALS_MEASURED, measured with this file, asserted at twice
that).  The variation is compared with numpy at 1e-15 relative.  Eigen is not on the test machines, so eulerAngles(0, 1, 2) is pinned by
what it promises: Rx(a) Ry(b) Rz(c) gives the matrix back to 1e-12, and the range is [0, pi] x [-pi, pi] x [-pi, pi].  The reduction is
compared with np.cov(ddof=1) + 0.001 I on the twin's own pose vectors, and its edges are forced through a table of deviates: a sample
FAILS where its first pair gets a distance deviate of 1e200 (the residuals' squares overflow: CAPE_POSE_SOLVE_NOT_FINITE, no NaN
standard deviation involved), and a sample that maxfev ends (status 5 > 0) counts as a success, as in the reference.  The statistical
test compares the position block with the first-order propagation of the map planes' noise.  CPU only."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
from test_pose_solve_host import planes_to_camera, pose_of, residuals, words_of

# the largest difference between the twin's normals and numpy's over DRAW_SHAPE deviates (measured with this file on the host;
# printed by test_uniforms_and_normals_against_numpy before it asserts)
NORMALS_MEASURED = 2.3e-16
DRAW_SHAPE = (64, 128, 4)

KNOWN_ANSWERS = [  # (counter, key) -> output
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.fixture(scope="module")
def host(host_binaries):
    import cape_amd

    return cape_amd


# ---- Philox ---------------------------------------------------------------------------------------------------------------------------
def philox_numpy(counter, key):
    """Philox4x32-10 on arrays of counters (4, ...) and one key (2,), uint64 arithmetic masked to 32 bits"""
    mask = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, np.uint64) for v in counter]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def uniforms_numpy(seed, frame, n_iterations):
    it, slot = np.meshgrid(np.arange(n_iterations, dtype=np.uint64), np.arange(128, dtype=np.uint64), indexing="ij")
    u = np.empty((n_iterations, 128, 4))
    for block in (0, 1):
        w = philox_numpy((np.full_like(it, frame), it, slot, np.full_like(it, block)), (seed & 0xFFFFFFFF, seed >> 32))
        for half in (0, 1):
            bits = ((w[2 * half] << np.uint64(32)) | w[2 * half + 1]) >> np.uint64(11)
            u[..., 2 * block + half] = (bits.astype(np.float64) + 1.0) * 2.0 ** -53
    return u


def normals_numpy(u):
    z = np.empty_like(u)
    for b in (0, 1):
        radius, angle = np.sqrt(-2.0 * np.log(u[..., 2 * b])), 2.0 * math.pi * u[..., 2 * b + 1]
        z[..., 2 * b], z[..., 2 * b + 1] = radius * np.cos(angle), radius * np.sin(angle)
    return z


def test_philox_known_answers(host):
    for counter, key, want in KNOWN_ANSWERS:
        got = host.host_philox4x32_10(counter, key)
        assert [int(v) for v in got] == list(want), [f"{int(v):08x}" for v in got]
        # (the restatement of this file is held to them too, before it serves as a reference)
        assert [int(v) for v in philox_numpy([np.uint64(v) for v in counter], key)] == list(want)


def test_uniforms_and_normals_against_numpy(host):
    seed, frame = 0x0123456789ABCDEF, 7
    u = host.host_pose_draw_deviates(seed, frame, DRAW_SHAPE[0], uniforms=True)
    z = host.host_pose_draw_deviates(seed, frame, DRAW_SHAPE[0])
    want_u = uniforms_numpy(seed, frame, DRAW_SHAPE[0])
    assert u.shape == DRAW_SHAPE and u.tobytes() == want_u.tobytes(), "the uniforms are the same words"
    assert u.min() > 0.0 and u.max() <= 1.0
    d = float(np.abs(z - normals_numpy(want_u)).max())
    print(f"normals, twin against numpy over {z.size} deviates: at most {d:.3e} apart; mean {z.mean():+.4f}, variance {z.var():.4f}, |z| <= {np.abs(z).max():.2f}")
    assert d <= 2 * NORMALS_MEASURED
    # standard normal to what 32 768 deviates can show (five standard errors of the mean and of the variance)
    assert abs(z.mean()) < 5 / math.sqrt(z.size) and abs(z.var() - 1.0) < 5 * math.sqrt(2.0 / z.size)
    # another seed, frame or iteration is another stream
    assert not np.array_equal(u, host.host_pose_draw_deviates(seed + 1, frame, DRAW_SHAPE[0], uniforms=True))
    assert not np.array_equal(u, host.host_pose_draw_deviates(seed, frame + 1, DRAW_SHAPE[0], uniforms=True))
    assert len(np.unique(u)) == u.size
    # the first known answer through the uniforms: seed 0, frame 0, iteration 0, slot 0, block 0
    first = host.host_pose_draw_deviates(0, 0, 1, uniforms=True)[0, 0]
    assert first[0] == (((0x6627E8D5 << 32 | 0xE169C58D) >> 11) + 1) * 2.0 ** -53 and first[1] == (((0xBC57AC4C << 32 | 0x9B00DBD8) >> 11) + 1) * 2.0 ** -53


# ---- the variation ----------------------------------------------------------------------------------------------------------------------
def test_variation_against_numpy(host):
    rng = np.random.default_rng(500)
    worst = 0.0
    for _ in range(500):
        n = rng.normal(size=3)
        plane = np.array([*(n / np.linalg.norm(n)), rng.uniform(500.0, 4000.0)])
        stddev, z = np.array([*rng.uniform(0.0, 0.05, 3), rng.uniform(0.0, 5.0)]), rng.normal(size=4)
        got = host.host_pose_vary_plane(plane, stddev, z)
        moved = plane[:3] + z[:3] * stddev[:3]
        want = np.array([*(moved / math.sqrt((moved[0] * moved[0] + moved[1] * moved[1]) + moved[2] * moved[2])), plane[3] + z[3] * stddev[3]])
        worst = max(worst, float(np.abs(got / want - 1.0).max()))
    print(f"variation against numpy: at most {worst:.3e} relative")
    assert worst <= 1e-15


def test_variation_edges(host):
    # stddev = 0: the plane's bytes after the normalise (a division per component by the square root of the ordered sum)
    plane = np.array([0.6, 0.0, 0.8, 1500.0])
    norm = math.sqrt((0.6 * 0.6 + 0.0 * 0.0) + 0.8 * 0.8)
    got = host.host_pose_vary_plane(plane, np.zeros(4), [0.3, -1.2, 2.0, -0.7])
    assert got.tobytes() == np.array([0.6 / norm, 0.0 / norm, 0.8 / norm, 1500.0]).tobytes()
    # a variation that zeroes the normal is left unnormalised (s == 0)
    got = host.host_pose_vary_plane([0.0, 0.0, 1.0, 800.0], [0.5, 0.5, 0.5, 2.0], [0.0, 0.0, -2.0, 1.0])
    assert got.tolist() == [0.0, 0.0, 0.0, 802.0]


# ---- the Euler angles -------------------------------------------------------------------------------------------------------------------
def _rx_ry_rz(a, b, c):
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]])
    Ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    Rz = np.array([[cc, -sc, 0.0], [sc, cc, 0.0], [0.0, 0.0, 1.0]])
    return Rx @ Ry @ Rz


def test_euler_angles_rebuild_the_matrix_and_keep_their_range(host):
    rng = np.random.default_rng(510)
    cases = [_rx_ry_rz(a, b, c) for a in (-3.0, -1e-9, 0.0, 1e-9, 0.4, 3.0) for b in (-1.2, 0.0, 0.7) for c in (-2.5, 0.0, 1.9)]
    # c2 -> 0: the second angle at and next to +-pi/2, where the first row's first two entries vanish
    cases += [_rx_ry_rz(a, s * (math.pi / 2 - e), c) for a in (-0.8, 0.3) for s in (-1.0, 1.0) for e in (0.0, 1e-12, 1e-8, 1e-4) for c in (-1.1, 0.6)]
    worst, below, above = 0.0, 0, 0
    for R in cases:
        ang = host.host_euler_angles_012(R)
        worst = max(worst, float(np.abs(_rx_ry_rz(*ang) - R).max()))
        # the range convention of Eigen 3.4: [0, pi] x [-pi, pi] x [-pi, pi]
        assert 0.0 <= ang[0] <= math.pi and -math.pi <= ang[1] <= math.pi and -math.pi <= ang[2] <= math.pi, ang
    # the fold: rotations about x by -1e-9 and +1e-9 are 2e-9 apart, their first angles almost pi
    lo, hi = host.host_euler_angles_012(_rx_ry_rz(-1e-9, 0.2, 0.1)), host.host_euler_angles_012(_rx_ry_rz(1e-9, 0.2, 0.1))
    assert abs(abs(hi[0] - lo[0]) - math.pi) < 1e-8, (lo, hi)
    # ... and through x: the matrix the rules header builds of the three coefficients, on both sides of the fold
    for _ in range(2000):
        x = np.concatenate([rng.normal(size=3), rng.normal(size=3) * rng.choice([0.01, 1.0, 30.0])])
        v, R = host.host_pose_vector(x)
        assert np.array_equal(v[:3], x[:3]) and np.abs(R @ R.T - np.eye(3)).max() < 1e-14
        worst = max(worst, float(np.abs(_rx_ry_rz(*v[3:]) - R).max()))
        below, above = below + (v[3] < 0.5), above + (v[3] > math.pi - 0.5)
        assert 0.0 <= v[3] <= math.pi
    print(f"Euler angles: Rx Ry Rz of them differs from the matrix by at most {worst:.3e}; {below} first angles near 0, {above} near pi")
    assert worst <= 1e-12 and below > 50 and above > 50


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
X_TRUE = np.array([120.0, -80.0, 45.0, 0.6, 0.5, -0.3])  # (its first Euler angle is 1.2: well away from the fold)


def frame_of(host, seed, n, stddev_normal, stddev_d, x_true=X_TRUE):
    """n map planes, all matched, seen from x_true with the noise of make_frame; the tracks' covariance diag(stddev^2)"""
    rng = np.random.default_rng(seed)
    normals = rng.normal(size=(n, 3))
    planes = np.column_stack([normals / np.linalg.norm(normals, axis=1)[:, None], rng.uniform(500.0, 4000.0, n)])
    P = np.zeros(n, host.MAP_PLANE_DTYPE)
    P["normal"], P["d"] = planes[:, :3], planes[:, 3]
    tracks = np.zeros(n, host.MAP_TRACK_DTYPE)
    tracks["covariance"] = np.diag([stddev_normal ** 2] * 3 + [stddev_d ** 2])
    tracks["id"] = 1000 + 7 * np.arange(n)
    arrays = (P, np.zeros(0, host.MAP_RING_DTYPE), np.zeros((0, 2)))
    qn, qd = planes_to_camera(pose_of(x_true), planes)
    qn = qn + rng.normal(scale=1e-3, size=qn.shape)
    detected = np.column_stack([qn / np.linalg.norm(qn, axis=1)[:, None], qd + rng.normal(scale=2.0, size=n)])
    return planes, arrays, tracks, detected, np.arange(n, dtype=np.int32)


@pytest.fixture(scope="module")
def frame39(host):
    """a 39-pair frame and its optimised x"""
    planes, arrays, tracks, detected, match = frame_of(host, 520, 39, 2e-4, 0.5)
    words = words_of(range(39))
    sol, _, _ = host.host_pose_solve(arrays, tracks, match, detected, X_TRUE[None] + [[5.0, -4.0, 3.0, 0.01, -0.01, 0.005]], np.array([words], np.uint32))
    assert sol[0]["status"] in (1, 2, 3)
    return dict(planes=planes, arrays=arrays, tracks=tracks, detected=detected, match=match, words=words, x=sol[0]["x"].copy())


def _run(host, f, n_iterations, **kw):
    return host.host_pose_covariance(f["arrays"], f["tracks"], f["match"], f["detected"], n_iterations, kw.pop("x", f["x"]), kw.pop("subset", f["words"]), **kw)


def _table(n_iterations, seed, fail=()):
    """a table of standard normals; the iterations of `fail` get 1e200 as the distance deviate of pair slot 0"""
    z = np.random.default_rng(seed).normal(size=(n_iterations, 128, 4))
    for i in fail:
        z[i, 0, 3] = 1e200
    return z


def _expected(vectors, ok):
    v = vectors[ok]
    return v.mean(axis=0), np.cov(v.T, ddof=1) + 0.001 * np.eye(6)


def test_reduction_against_numpy(host, frame39):
    for mode, kw in (("Philox", dict(seed=77, frame_index=3)), ("table", dict(deviates=_table(100, 530)))):
        row, samples, vectors = _run(host, frame39, 100, **kw)
        ok = samples["status"] > 0
        mean, cov = _expected(vectors, ok)
        d_mean, d_cov = float(np.abs(row["mean"] / mean - 1.0).max()), float(np.abs(row["covariance"] - cov).max() / np.abs(cov).max())
        print(f"{mode}: status {row['status']}, n_ok {row['n_ok']}, nfev {row['nfev_min']}..{row['nfev_max']} (sum {row['nfev_sum']}); "
              f"mean {d_mean:.2e}, covariance {d_cov:.2e} relative from numpy; diagonal {np.diag(row['covariance']).tolist()}")
        assert row["status"] == host.POSE_COVARIANCE_VALID and row["n_ok"] == 100 == row["n_iterations"] and ok.all() and row["flags"] == 0
        assert d_mean <= 1e-12 and d_cov <= 1e-12
        assert (row["nfev_min"], row["nfev_max"], row["nfev_sum"]) == (samples["nfev"].min(), samples["nfev"].max(), samples["nfev"].sum())
        assert np.array_equal(row["covariance"], row["covariance"].T) and (np.diag(row["covariance"])[:3] > 0.0011).all()
        # the pose vector of a sample is the position of its x and the angles of its rotation
        for s, v in zip(samples[:5], vectors[:5]):
            assert np.array_equal(v, host.host_pose_vector(s["x"])[0])
    # the same seed gives the same bytes; another seed or frame index other samples
    a, b = _run(host, frame39, 20, seed=5, frame_index=2), _run(host, frame39, 20, seed=5, frame_index=2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert _run(host, frame39, 20, seed=6, frame_index=2)[1].tobytes() != a[1].tobytes() != _run(host, frame39, 20, seed=5, frame_index=3)[1].tobytes()
    # Philox through the twin's own table is Philox on the fly, bit for bit
    drawn = _run(host, frame39, 20, deviates=host.host_pose_draw_deviates(5, 2, 20))
    assert drawn[0].tobytes() == a[0].tobytes() and drawn[1].tobytes() == a[1].tobytes()


@pytest.mark.parametrize("n_iterations, fail, status, n_ok", [
    (1, (), "invalid", 1),               # 0 / 0: "invalid values"
    (2, (1,), "invalid", 1),             # one success of two: n_ok = 1 is not below 2 / 2
    (2, (0, 1), "failed", 0),
    (3, (0,), "valid", 2),
    (3, (0, 2), "invalid", 1),           # 3 / 2 = 1: one success is enough to go on, and divides by zero
    (10, (1, 2, 5, 6, 8, 9), "failed", 4),   # iterations / 2 - 1
    (10, (1, 2, 5, 8, 9), "valid", 5),       # iterations / 2
    (10, (), "valid", 10),
    (11, (0, 1, 2, 3, 4, 5), "valid", 5),    # 11 / 2 = 5
    (11, (0, 1, 2, 3, 4, 5, 6), "failed", 4),
])
def test_reduction_edges(host, frame39, n_iterations, fail, status, n_ok):
    want = {"valid": host.POSE_COVARIANCE_VALID, "invalid": host.POSE_COVARIANCE_INVALID, "failed": host.POSE_COVARIANCE_TOO_MANY_FAILED}[status]
    row, samples, vectors = _run(host, frame39, n_iterations, deviates=_table(n_iterations, 540 + n_iterations, fail))
    print(f"{n_iterations} iterations, failing {fail}: sample statuses {samples['status'].tolist()}, row status {row['status']}, n_ok {row['n_ok']}")
    assert [i for i in range(n_iterations) if samples[i]["status"] <= 0] == list(fail)
    assert (samples["status"][list(fail)] == host.POSE_SOLVE_NOT_FINITE).all()
    assert row["status"] == want and row["n_ok"] == n_ok and row["n_iterations"] == n_iterations
    if status == "valid":
        mean, cov = _expected(vectors, samples["status"] > 0)
        assert np.abs(row["mean"] / mean - 1.0).max() <= 1e-12 and np.abs(row["covariance"] - cov).max() <= 1e-12 * np.abs(cov).max()
    elif status == "invalid":
        assert np.isnan(row["covariance"]).all() and np.array_equal(row["mean"], vectors[samples["status"] > 0][0])
    else:
        assert not row["mean"].any() and not row["covariance"].any()


def test_samples_that_maxfev_ends_count(host, frame39):
    """maxfev = 8 ends every sample with info 5 after the first trial point: status > 0, a success by the reference's rule; the iterations
    of `fail` overflow and do not count"""
    params = host.pose_solve_params(maxfev=8)
    row, samples, vectors = _run(host, frame39, 10, deviates=_table(10, 550, fail=(3, 7)), params=params)
    print(f"maxfev = 8: sample statuses {samples['status'].tolist()}, nfev {samples['nfev'].tolist()}")
    assert samples["status"].tolist() == [5, 5, 5, -6, 5, 5, 5, -6, 5, 5] and row["n_ok"] == 8 and row["status"] == host.POSE_COVARIANCE_VALID
    mean, cov = _expected(vectors, samples["status"] > 0)
    assert np.abs(row["covariance"] - cov).max() <= 1e-12 * np.abs(cov).max()


def test_identical_samples_give_the_diagonal_alone(host):
    """stddev = 0: every sample is the same minimisation.  Two of them have an exact mean ((v + v) / 2 = v): the covariance is exactly
    0.001 I -- the "perfect covariance" the reference adds the 0.001 for -- and valid.  Among 64 the running sum k v rounds, the mean is
    v to within 64 half-ulps of the sum, and every entry stays within (64 x 2^-52 x max |v|)^2 of that"""
    planes, arrays, tracks, detected, match = frame_of(host, 560, 39, 0.0, 0.0)
    f = dict(arrays=arrays, tracks=tracks, match=match, detected=detected, words=words_of(range(39)), x=X_TRUE)
    row, samples, vectors = _run(host, f, 2, seed=9)
    assert samples[0].tobytes() == samples[1].tobytes() and samples[0]["status"] > 0
    assert row["status"] == host.POSE_COVARIANCE_VALID and row["covariance"].tobytes() == (0.001 * np.eye(6)).tobytes()
    assert np.array_equal(row["mean"], vectors[0])
    row, samples, vectors = _run(host, f, 64, seed=9)
    bound = (64 * 2.0 ** -52 * np.abs(vectors[0]).max()) ** 2
    assert len({s.tobytes() for s in samples}) == 1 and row["status"] == host.POSE_COVARIANCE_VALID
    assert np.abs(row["covariance"] - 0.001 * np.eye(6)).max() <= bound < 1e-20


def test_a_normal_varied_to_zero_goes_through_the_solvers_guards(host, frame39):
    """pair slot 0's map plane becomes (0, 0, 1) with a standard deviation of 0.5 per component; the deviate (0, 0, -2) of iteration 1
    zeroes its normal, which stays unnormalised.  What becomes of the sample is the solver's to decide, and its guards let it run:
    utils::plane_to_camera leaves a zero vector alone as Eigen's normalized() does, so the pair's residual is cd x cn, a constant that no
    pose reduces, and the minimiser converges on the other 38 pairs -- a success whose fnorm is at least that constant, no NaN
    anywhere.  (Measured on the twin: status 3 where the unvaried iterations end with 1.)"""
    f = dict(frame39)
    P, rings, vertices = f["arrays"]
    P = P.copy()
    P[0]["normal"] = [0.0, 0.0, 1.0]
    tracks = f["tracks"].copy()
    tracks[0]["covariance"] = np.diag([0.25, 0.25, 0.25, 1.0])
    f["arrays"], f["tracks"] = (P, rings, vertices), tracks
    z = np.zeros((4, 128, 4))
    z[1, 0] = [0.0, 0.0, -2.0, 0.0]
    assert host.host_pose_vary_plane([0.0, 0.0, 1.0, P[0]["d"]], [0.5, 0.5, 0.5, 1.0], z[1, 0]).tolist() == [0.0, 0.0, 0.0, P[0]["d"]]
    row, samples, vectors = _run(host, f, 4, deviates=z)
    print(f"a zeroed normal: sample statuses {samples['status'].tolist()}, fnorm {samples['fnorm'].tolist()}")
    assert samples[0].tobytes() == samples[2].tobytes() == samples[3].tobytes() != samples[1].tobytes()
    assert (samples["status"] > 0).all() and np.isfinite(samples[1]["x"]).all() and np.isfinite(vectors).all() and row["n_ok"] == 4
    # the constant residual of the pair: cd x cn / 3 in each of its three rows
    d0 = f["detected"][0]
    assert samples[1]["fnorm"] >= np.linalg.norm(d0[3] * d0[:3] / 3.0) * (1 - 1e-12)


def test_refusals_are_the_frames(host, frame39):
    f = frame39
    for kw, want in ((dict(subset=words_of([0, 1])), host.POSE_SOLVE_TOO_FEW_PAIRS), (dict(x=np.array([np.nan, 0, 0, 1, 0, 0.0])), host.POSE_SOLVE_BAD_START),
                     (dict(frame_flags=host.MATCH_EXACT_OVERFLOW), host.POSE_SOLVE_OVERFLOW)):
        if "frame_flags" in kw:  # (a flagged frame comes without matches, as the device's)
            row, samples, _ = host.host_pose_covariance(f["arrays"], f["tracks"], np.full(39, -1, np.int32), f["detected"], 5, f["x"], f["words"], **kw)
        else:
            row, samples, _ = _run(host, f, 5, **kw)
        assert row["status"] == want and row["n_ok"] == 0 and row["nfev_sum"] == 0 and not samples["nfev"].any() and not row["covariance"].any()
    bad = f["tracks"].copy()
    bad[3]["covariance"][2, 2] = -1e-6
    row, _, _ = host.host_pose_covariance(f["arrays"], bad, f["match"], f["detected"], 5, f["x"], f["words"])
    assert row["status"] == host.POSE_SOLVE_INVALID_FEATURE and row["flags"] == host.POSE_SCORE_INVALID_FEATURE
    # from the refit's row and its selection
    sol, sel = np.zeros(1, host.POSE_SOLUTION_DTYPE), np.zeros(1, host.POSE_SELECTION_DTYPE)
    sol["x"], sol["status"], sel["inlier_words"], sel["best"] = f["x"], 2, f["words"], 0
    direct = _run(host, f, 8, seed=3)
    via = host.host_pose_covariance(f["arrays"], f["tracks"], f["match"], f["detected"], 8, solution=sol[0], selection=sel[0], seed=3)
    assert via[0].tobytes() == direct[0].tobytes() and via[1].tobytes() == direct[1].tobytes() and direct[0]["status"] == host.POSE_COVARIANCE_VALID
    for status, want in ((host.POSE_SOLVE_NO_SELECTION, host.POSE_SOLVE_NO_SELECTION), (host.POSE_SOLVE_NOT_FINITE, host.POSE_SOLVE_NOT_FINITE),
                         (0, host.POSE_COVARIANCE_NO_SOLUTION)):
        sol["status"] = status
        row, _, _ = host.host_pose_covariance(f["arrays"], f["tracks"], f["match"], f["detected"], 8, solution=sol[0], selection=sel[0], seed=3)
        assert row["status"] == want and row["n_ok"] == 0


def test_a_match_entry_out_of_range_is_an_invalid_argument(host, frame39):
    """the pair builder the three twins share checks the match against the detected planes: an entry >= detected->n"""
    f = frame39
    for entry in (39, 128, 2 ** 31 - 1):
        match = f["match"].copy()
        match[20] = entry
        with pytest.raises(host.CapeError, match=r"cape_host_pose_covariance failed \(-1\)"):  # CAPE_ERR_INVALID_ARGUMENT
            host.host_pose_covariance(f["arrays"], f["tracks"], match, f["detected"], 5, f["x"], f["words"])


# ---- statistical sanity: the position block against first-order propagation ------------------------------------------------------------
N_SAMPLES = 500
BOUND = 6.0 * math.sqrt(2.0 / (N_SAMPLES - 1))  # six standard errors of a sample variance, relative


def _vary_numpy(planes, stddev, z):
    moved = planes[:, :3] + z[:, :3] * stddev[:3]
    return np.column_stack([moved / np.linalg.norm(moved, axis=1)[:, None], planes[:, 3] + z[:, 3] * stddev[3]])


@pytest.fixture(scope="module")
def propagated(frame39):
    """(J^T J)^-1 J^T Sigma J (J^T J)^-1 at the optimised x: J the residuals' Jacobian in x, Sigma = Jp diag(stddev^2) Jp^T the
    residuals' covariance under the map planes' noise, Jp their Jacobian in the deviates -- both by central differences in numpy"""
    f = frame39
    planes, det, x = f["planes"], f["detected"], f["x"]
    stddev = np.sqrt(np.diag(f["tracks"][0]["covariance"]))
    J = np.empty((3 * 39, 6))
    for j in range(6):
        h = 1e-6 * max(1.0, abs(x[j]))
        e = np.zeros(6)
        e[j] = h
        J[:, j] = (residuals(x + e, planes, det) - residuals(x - e, planes, det)) / (2 * h)
    Jp = np.zeros((3 * 39, 4 * 39))
    for k in range(39):
        for c in range(4):
            z = np.zeros((39, 4))
            z[k, c] = 1e-3  # (in units of the standard deviation: 2e-7 in a normal, 5e-4 mm in a distance)
            Jp[:, 4 * k + c] = (residuals(x, _vary_numpy(planes, stddev, z), det) - residuals(x, _vary_numpy(planes, stddev, -z), det)) / 2e-3
    A = np.linalg.solve(J.T @ J, J.T)
    return A @ (Jp @ Jp.T) @ A.T  # (the deviates are standard normal: their covariance is the identity)


def test_numpy_alone_stays_inside_the_sampling_bound(frame39, propagated):
    """the reference alone, before the twin is looked at: numpy draws its own normals, varies the planes and minimises with MINPACK's
    lmdif (scipy) from the optimised x; the variances of the end positions agree with the first-order propagation within BOUND.
    Measured here: +0.028, +0.014, +0.065 relative at stddev (2e-4, 0.5 mm) and n = 500 (the twin's own samples: +0.007, +0.064, -0.049)
    -- no linearisation bias shows beside BOUND = 0.380, so the standard deviations were not reduced."""
    from scipy.optimize import leastsq

    f = frame39
    stddev = np.sqrt(np.diag(f["tracks"][0]["covariance"]))
    rng = np.random.default_rng(570)
    ends = np.array([leastsq(residuals, f["x"], args=(_vary_numpy(f["planes"], stddev, rng.normal(size=(39, 4))), f["detected"]))[0] for _ in range(N_SAMPLES)])
    rel = np.var(ends[:, :3], axis=0, ddof=1) / np.diag(propagated)[:3] - 1.0
    print(f"numpy alone, {N_SAMPLES} samples: variances {np.var(ends[:, :3], axis=0, ddof=1).tolist()} against {np.diag(propagated)[:3].tolist()}: {rel.tolist()} relative; bound {BOUND:.3f}")
    assert np.abs(rel).max() <= BOUND


def test_position_block_against_first_order_propagation(host, frame39, propagated):
    row, samples, _ = _run(host, frame39, N_SAMPLES, seed=2026, frame_index=1)
    got = np.diag(row["covariance"])[:3] - 0.001
    rel = got / np.diag(propagated)[:3] - 1.0
    print(f"twin, {N_SAMPLES} samples: position variances {got.tolist()} against {np.diag(propagated)[:3].tolist()}: {rel.tolist()} relative; bound {BOUND:.3f}")
    assert row["status"] == host.POSE_COVARIANCE_VALID and row["n_ok"] == N_SAMPLES
    assert np.abs(rel).max() <= BOUND
    # (the 0.001 is not what is being compared: the variances themselves are several times it)
    assert (np.diag(propagated)[:3] > 0.002).all()


# ---- the stand-alone program under the host sanitizers, and the ABI ---------------------------------------------------------------------
def test_rules_header_under_the_host_sanitizers(tmp_path):
    """tests/host/pose_covariance_check.cpp: the rules header in a stand-alone program built with AddressSanitizer and UBSan"""
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host_dir = os.path.join(root, "rgb-d-slam_amd", "host")
    exe = str(tmp_path / "pose_covariance_check.exe")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + host_dir, "-I" + os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "host", "pose_covariance_check.cpp"),
                            os.path.join(host_dir, "boundary_polygon.cpp"), os.path.join(host_dir, "map_tracking.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and "sanitizer" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("the sanitizer runtimes are not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "0 expectations missed" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def test_abi(hip_library, host):
    import ctypes as C
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    public = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "cape_hip.h")).read(), flags=re.S)
    for name in ("cape_map_pose_covariance", "cape_copy_pose_covariance", "cape_copy_pose_covariance_samples", "cape_pose_covariance_device",
                 "cape_pose_draw_deviates", "cape_set_pose_covariance_budget"):
        assert re.search(r"int %s\(cape_handle h" % name, public) and name in host.EXPORTED_SYMBOLS
    # the result row: 368 bytes, a multiple of 16, and where its members lie
    D = host.POSE_COVARIANCE_DTYPE
    assert D.itemsize == 368 and D.itemsize % 16 == 0
    assert {k: D.fields[k][1] for k in D.names} == dict(mean=0, covariance=48, n_ok=336, n_iterations=340, status=344, flags=348, nfev_min=352, nfev_max=356,
                                                        nfev_sum=360)
    struct = re.search(r"typedef struct cape_pose_covariance\s*\{(.*?)\} cape_pose_covariance;", public, flags=re.S).group(1)
    assert [m for m in re.findall(r"(\w+)(?:\[\d+\])?[;,]", struct)] == ["mean", "covariance", "n_ok", "n_iterations", "status", "flags", "nfev_min", "nfev_max", "nfev_sum"]
    assert (host.POSE_COVARIANCE_VALID, host.POSE_COVARIANCE_TOO_MANY_FAILED, host.POSE_COVARIANCE_INVALID, host.POSE_COVARIANCE_NO_SOLUTION) == (1, -16, -17, -18)
    for name, value in (("DEVICE_INPUT", 0), ("FROM_SOLUTION", 1), ("TABLE", 2), ("KEEP_SAMPLES", 3)):
        assert re.search(r"CAPE_POSE_COVARIANCE_%s = 1u << %d" % (name, value), public) and getattr(host, "POSE_COVARIANCE_" + name) == 1 << value
    # the argument checks in front of the handle
    L = host.load_library()
    x, w, z = np.zeros(6), np.zeros(4, np.uint32), np.zeros((1, 128, 4))
    xp, wp, zp = (a.ctypes.data_as(C.c_void_p) for a in (x, w, z))
    assert L.cape_map_pose_covariance(None, 1, 1, xp, wp, None, 0, 0, None, 0, None) == -1 and b"null handle" in L.cape_last_error()
    assert L.cape_map_pose_covariance(None, 1, 0, xp, wp, None, 0, 0, None, 0, None) == -1 and b"n_iterations" in L.cape_last_error()
    assert L.cape_map_pose_covariance(None, 1, 1, xp, wp, None, 0, 0, None, 1 << 4, None) == -1 and b"unknown pose-covariance flag" in L.cape_last_error()
    assert L.cape_map_pose_covariance(None, 1, 1, xp, wp, None, 0, 0, None, host.POSE_COVARIANCE_TABLE, None) == -1 and b"null table" in L.cape_last_error()
    assert L.cape_map_pose_covariance(None, 1, 1, xp, wp, zp, 0, 0, None, host.POSE_COVARIANCE_TABLE, None) == -1 and b"null handle" in L.cape_last_error()
    bad = host.pose_solve_params(maxfev=0)
    assert L.cape_map_pose_covariance(None, 1, 1, xp, wp, None, 0, 0, bad.ctypes.data_as(C.c_void_p), 0, None) == -1 and b"parameter" in L.cape_last_error()
    assert L.cape_copy_pose_covariance(None, 1, None) == -1 and L.cape_copy_pose_covariance_samples(None, 1, None) == -1
    assert L.cape_pose_covariance_device(None, None) == -1 and L.cape_pose_draw_deviates(None, 0, 0, 1, zp, 0) == -1
    assert L.cape_set_pose_covariance_budget(None, 0) == -1
    for name in ("map_pose_covariance", "pose_covariance", "pose_covariance_samples", "pose_covariance_device", "pose_draw_deviates", "set_pose_covariance_budget"):
        assert callable(getattr(host.Extractor, name))
    assert callable(host.host_pose_covariance) and callable(host.host_pose_draw_deviates)

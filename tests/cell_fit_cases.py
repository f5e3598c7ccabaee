"""Input families for the per-cell eigen-solver and plane fit (cape_device.h: self_adjoint_eigen3, fit_plane), shared by the CPU tests
(test_cell_fit_cases.py: do the families reach the branches they are named for, is the oracle right on them) and the GPU tests
(test_gpu_math.py: is the device equal to the oracle on them).  Every family is a function of a seed, so both sides see the same bits.

Solver families return an (N, 6) array of lower triangles (m00 m10 m11 m20 m21 m22), the operand order of debug_eval("eigen3").
fit_plane families return an (N, 10) array: the nine sums Sx Sy Sz Sxs Sys Szs Sxy Syz Szx and the count, the operands of
debug_eval("fit_plane").  The sums are free inputs: where a family needs an exact covariance it passes Sx = Sy = Sz = 0 with n = 1, so
that the Huygens terms are the second-order sums themselves."""
import numpy as np

SEED = 20  # the seed at which the CPU tests assert each family's trace and the GPU tests compare the device with the oracle
EPS = np.finfo(np.float64).eps
DBL_MIN = np.finfo(np.float64).tiny


def full(m6):
    """The symmetric 3x3 matrix of one lower triangle."""
    m00, m10, m11, m20, m21, m22 = m6
    return np.array([[m00, m10, m20], [m10, m11, m21], [m20, m21, m22]], np.float64)


def _sym_normal(rng, n):
    """n lower triangles of G + G^T, G standard normal: dense, indefinite, entries of order 1."""
    g = rng.standard_normal((n, 3, 3))
    a = g + g.transpose(0, 2, 1)
    return np.stack([a[:, 0, 0], a[:, 1, 0], a[:, 1, 1], a[:, 2, 0], a[:, 2, 1], a[:, 2, 2]], axis=1)


# ---- solver families -----------------------------------------------------------------------------------------------------------

def dense(seed, n=256):
    """test_eigen3_bitwise_vs_oracle's construction: scatter matrices of 400 anisotropic points, every seventh without a z extent."""
    rng = np.random.default_rng(seed)
    mats = np.zeros((n, 6))
    for i in range(n):
        p = rng.standard_normal((400, 3)) * rng.uniform(0.01, 100, 3)
        if i % 7 == 0:
            p[:, 2] = 0.0
        c = p.T @ p
        mats[i] = [c[0, 0], c[1, 0], c[1, 1], c[2, 0], c[2, 1], c[2, 2]]
    return mats


def x_decoupled(seed, n=256):
    """m10 = m20 = 0 and m21 != 0: s0 is zero from the start, the only block is [1,2].  Even rows indefinite, odd rows positive definite."""
    rng = np.random.default_rng(seed)
    mats = np.zeros((n, 6))
    g = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    mats[:, 0], mats[:, 2], mats[:, 4], mats[:, 5] = rng.standard_normal(n), g[:, 0], g[:, 1], g[:, 2]
    b = rng.standard_normal((n, 2, 2))
    pd = b @ b.transpose(0, 2, 1) + 1e-3 * np.eye(2)
    odd = np.arange(n) % 2 == 1
    mats[odd, 0] = np.abs(mats[odd, 0]) + 1e-3
    mats[odd, 2], mats[odd, 4], mats[odd, 5] = pd[odd, 0, 0], pd[odd, 1, 0], pd[odd, 1, 1]
    assert np.all(mats[:, 4] != 0.0)
    return mats


def rank1(seed, n=256):
    """v v^T: two eigenvalues are zero up to rounding, so which subdiagonal deflates first is decided by rounding noise.  Where s0
    goes first, block [0,2] is followed by block [1,2].  Thirds: v standard normal, v of small integers (v v^T exact, zeros among its
    entries), v anisotropic over four decades."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v[1::3] = rng.integers(-9, 10, v[1::3].shape)
    v[2::3] *= 10.0 ** rng.uniform(-2, 2, v[2::3].shape)
    return np.stack([v[:, 0] * v[:, 0], v[:, 1] * v[:, 0], v[:, 1] * v[:, 1], v[:, 2] * v[:, 0], v[:, 2] * v[:, 1], v[:, 2] * v[:, 2]], axis=1)


def tiny_m20(seed, n=256):
    """m20 / scale between 1e-170 and 1e-140: its square falls on both sides of DBL_MIN, the test that skips the tridiagonalisation."""
    rng = np.random.default_rng(seed)
    mats = _sym_normal(rng, n)
    scale = np.abs(mats[:, [0, 1, 2, 4, 5]]).max(axis=1)
    mats[:, 3] = scale * 10.0 ** rng.uniform(-170, -140, n) * rng.choice([-1.0, 1.0], n)
    return mats


def near_isotropic(seed, n=256):
    rng = np.random.default_rng(seed)
    mats = 1e-8 * _sym_normal(rng, n)
    mats[:, [0, 2, 5]] += 1.0
    return mats


def scale_lo(seed, n=256):
    return _sym_normal(np.random.default_rng(seed), n) * 1e-300


def scale_hi(seed, n=256):
    return _sym_normal(np.random.default_rng(seed), n) * 1e300


def repeated(seed, n=256):
    """diag(2,2,2), diag(2,2,3), diag(1,2,2), the zero matrix; then the same patterns at random magnitudes and signs."""
    rng = np.random.default_rng(seed)
    mats = np.zeros((n, 6))
    fixed = [(2, 2, 2), (2, 2, 3), (1, 2, 2), (0, 0, 0)]
    for i in range(n):
        if i < len(fixed):
            d = fixed[i]
        else:
            a, b = rng.standard_normal(2) * 10.0 ** rng.uniform(-6, 6)
            d = [(a, a, a), (a, a, b), (a, b, b), (a, b, a)][i % 4]
        mats[i, 0], mats[i, 2], mats[i, 5] = d
    return mats


def shift_underflow(seed, n=256):
    """(1, 0, a, 0, e, 0) in block [1,2] (even rows) and (a, e, 0, 0, 0, 1) in block [0,1] (odd rows), with |e| < 1.5e-162 so that e * e
    is zero, and |a| < (e / eps)^2 so that the deflation test keeps e: the Wilkinson shift takes its e2 == 0 branch."""
    rng = np.random.default_rng(seed)
    e = 10.0 ** rng.uniform(-166, -163, n)
    a = (e / EPS) ** 2 * 10.0 ** rng.uniform(-3, -0.5, n)
    assert np.all(e * e == 0.0) and np.all(a > DBL_MIN) and np.all((e / EPS) ** 2 > a)
    e *= rng.choice([-1.0, 1.0], n)
    a *= rng.choice([-1.0, 1.0], n)
    mats = np.zeros((n, 6))
    even = np.arange(n) % 2 == 0
    mats[even, 0], mats[even, 2], mats[even, 4] = 1.0, a[even], e[even]
    mats[~even, 0], mats[~even, 1], mats[~even, 5] = a[~even], e[~even], 1.0
    mats[0] = [1, 0, 1e-305, 0, 1e-165, 0]
    mats[1] = [1e-305, 1e-165, 0, 0, 0, 1]
    return mats


def td_zero(seed, n=256):
    """(a, 0, b, 0, c, b): the active block [1,2] has an equal diagonal, so td == 0 in its first Wilkinson shift."""
    rng = np.random.default_rng(seed)
    mats = np.zeros((n, 6))
    mats[:, 0] = rng.standard_normal(n)
    mats[:, 2] = mats[:, 5] = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    mats[:, 4] = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    mats[0] = [1, 0, 1, 0, 1, 1]
    assert np.all(mats[:, 4] != 0.0)
    return mats


def non_finite(seed, n=288):
    """One NaN, +Inf or -Inf at each of the six positions of a dense indefinite matrix."""
    rng = np.random.default_rng(seed)
    mats = _sym_normal(rng, n)
    bad = [np.nan, np.inf, -np.inf]
    for i in range(n):
        mats[i, i % 6] = bad[(i // 6) % 3]
    return mats


SOLVER_FAMILIES = dict(dense=dense, x_decoupled=x_decoupled, rank1=rank1, tiny_m20=tiny_m20, near_isotropic=near_isotropic,
                       scale_lo=scale_lo, scale_hi=scale_hi, repeated=repeated, shift_underflow=shift_underflow, td_zero=td_zero,
                       non_finite=non_finite)
FINITE_SOLVER_FAMILIES = [k for k in SOLVER_FAMILIES if k != "non_finite"]


# ---- fit_plane families --------------------------------------------------------------------------------------------------------

def sums_of(points):
    """The nine sums of a (k, 3) point set in float64.  Exact for integer-valued coordinates below 2^26."""
    p = np.asarray(points, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.array([x.sum(), y.sum(), z.sum(), (x * x).sum(), (y * y).sum(), (z * z).sum(), (x * y).sum(), (y * z).sum(), (x * z).sum()])


def covariance_sums(xx, xy, yy, xz, yz, zz):
    """Sums with Sx = Sy = Sz = 0, to go with n = 1: fit_plane's covariance is then exactly the given matrix."""
    return [0.0, 0.0, 0.0, xx, yy, zz, xy, yz, xz]


def huygens(rows):
    """fit_plane's covariance of (N, 10) rows, in its own float64 operation order: lower triangles (N, 6) = xx xy yy xz yz zz."""
    rows = np.asarray(rows, np.float64)
    S, inv = rows[:, :9].T, 1.0 / rows[:, 9]
    xx = np.maximum(0.0, S[3] - (S[0] * S[0]) * inv)
    yy = np.maximum(0.0, S[4] - (S[1] * S[1]) * inv)
    zz = np.maximum(0.0, S[5] - (S[2] * S[2]) * inv)
    xy = S[6] - S[0] * S[1] * inv
    xz = S[8] - S[0] * S[2] * inv
    yz = S[7] - S[1] * S[2] * inv
    return np.stack([xx, xy, yy, xz, yz, zz], axis=1)


def determinant(tri):
    """Matrix3d::determinant's first-row expansion of lower triangles xx xy yy xz yz zz, in float64."""
    xx, xy, yy, xz, yz, zz = np.asarray(tri, np.float64).T
    return xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz)


NOISY_PLANE_COUNTS = (1, 2, 3, 200, 280, 400, 307200)


def noisy_plane(seed, n=280):
    """400 float32 points of a tilted plane about 1.5 m away plus noise; the first k of them for k <= 400, all of them 768 times over for
    k = 307200.  The second-order sums are float32 products widened to double, like stage A1's."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 10))
    for i in range(n):
        k = NOISY_PLANE_COUNTS[i % len(NOISY_PLANE_COUNTS)]
        xy = rng.uniform(-200, 200, (400, 2))
        a, b = rng.uniform(-0.5, 0.5, 2)
        z = a * xy[:, 0] + b * xy[:, 1] + rng.uniform(800, 3000) + rng.standard_normal(400) * rng.uniform(0.5, 5)
        p = np.column_stack([xy, z]).astype(np.float32)[:min(k, 400)]
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        s = np.array([v.astype(np.float64).sum() for v in (x, y, z, x * x, y * y, z * z, x * y, y * z, x * z)])
        rows[i, :9] = s * 768.0 if k > 400 else s
        rows[i, 9] = k
    return rows


def det_edge(seed, n=256):
    """|det| from 0.25 eps to 4 eps around the `<= eps` return, on both signs, |det| == eps exactly included; exactly coplanar and
    collinear integer point sets, whose determinant is an exact zero."""
    rng = np.random.default_rng(seed)
    rows = []
    t = np.concatenate([[0.25, 0.5, 1.0, 2.0, 4.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2)], 2.0 ** rng.uniform(-2, 2, n // 4)])
    for v in t:
        # diag(1, 1, v eps): det = v eps exactly
        rows.append(covariance_sums(1.0, 0.0, 1.0, 0.0, 0.0, v * EPS) + [1])
        # xx = yy = 1, zz = 0, yz = 2^-26 sqrt(v): det = -(yz * yz), which is -eps exactly at v = 1
        rows.append(covariance_sums(1.0, 0.0, 1.0, 0.0, 2.0 ** -26 * np.sqrt(v), 0.0) + [1])
    # one covariance of eight integer points, the coordinates scaled so that det = s^6 det0 sweeps the same window
    cube = np.array([[i, j, k] for i in (-3, 2) for j in (-1, 4) for k in (-2, 1)], np.float64) + rng.integers(-1, 2, (8, 3))
    det0 = determinant(huygens([list(sums_of(cube)) + [8]]))[0]
    assert det0 > 1.0
    for v in 2.0 ** rng.uniform(-2, 2, n // 4):
        s = (v * EPS / det0) ** (1.0 / 6.0)
        rows.append(list(sums_of(cube * s)) + [8])
    while len(rows) < n:
        k = 2 ** rng.integers(2, 7)
        p = rng.integers(-60, 61, (k, 3)).astype(np.float64)
        if len(rows) % 2:
            p[:, 2] = rng.integers(-1000, 1001)  # coplanar: zz = 0 exactly (k is a power of two, every term is an integer)
        else:
            p = np.outer(rng.integers(-60, 61, k), rng.integers(-5, 6, 3)).astype(np.float64) + rng.integers(-100, 101, 3)  # collinear
        rows.append(list(sums_of(p)) + [k])
    return np.array(rows, np.float64)


def huygens_clamp(seed, n=256):
    """One coordinate constant near 1e7: Sxs - Sx^2 / n cancels to zero or to rounding noise just below or above it."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 10))
    for i in range(n):
        k = int(rng.integers(3, 401))
        p = rng.integers(-50, 51, (k, 3)).astype(np.float64)
        p[:, i % 3] = 1e7 + rng.integers(0, 1000)
        rows[i, :9], rows[i, 9] = sums_of(p), k
    return rows


def d_sign(seed, n=256):
    """Planes on either side of the origin, and point sets mirrored through it: Sx = Sy = Sz = 0 (with either sign of zero), so that
    d is +0 or -0 and `d <= 0` decides on a zero."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 10))
    for i in range(n):
        k = 64
        xy = rng.integers(-100, 101, (k, 2))
        a, b = rng.uniform(-0.4, 0.4, 2)
        z = np.rint(a * xy[:, 0] + b * xy[:, 1] + rng.integers(-3, 4, k))
        p = np.column_stack([xy, z]).astype(np.float64)
        kind = i % 4
        if kind < 2:
            p[:, 2] += 1500.0 if kind == 0 else -1500.0
            rows[i, :9], rows[i, 9] = sums_of(p), k
        else:
            rows[i, :9], rows[i, 9] = sums_of(np.concatenate([p, -p])), 2 * k
            assert not rows[i, :3].any()
            if kind == 3:
                rows[i, :3] = rng.choice([0.0, -0.0], 3)
    return rows


def score_clamp(seed, n=256):
    """Rotated diag(ev0, ev1, ev2) with ev0 from 1e-7 to 1e-5, on both sides of the 1e-6 clamp of the score, and ev1 ev2 >= 1."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 10))
    for i in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        ev = np.array([10.0 ** rng.uniform(-7, -5), rng.uniform(1, 10), rng.uniform(10, 1000)])
        c = (q * ev) @ q.T
        rows[i] = covariance_sums(c[0, 0], c[1, 0], c[1, 1], c[2, 0], c[2, 1], c[2, 2]) + [1]
    return rows


def mirrored_x(seed, n=256):
    """Every integer point (x, y, z) with its mirror (-x, y, z): Sx = Sxy = Szx = 0 exactly, so the solver inside fit_plane gets
    m10 = m20 = 0 and works in block [1,2]."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 10))
    for i in range(n):
        k = int(rng.integers(20, 200))
        xy = rng.integers(-100, 101, (k, 2))
        xy[:, 0] = np.abs(xy[:, 0]) + 1
        z = np.rint(rng.uniform(-0.5, 0.5) * xy[:, 1] + rng.integers(800, 3000) + rng.integers(-3, 4, k))
        p = np.column_stack([xy, z]).astype(np.float64)
        rows[i, :9], rows[i, 9] = sums_of(np.concatenate([p, p * [-1, 1, 1]])), 2 * k
    assert not rows[:, [0, 6, 8]].any()
    return rows


FIT_FAMILIES = dict(noisy_plane=noisy_plane, det_edge=det_edge, huygens_clamp=huygens_clamp, d_sign=d_sign, score_clamp=score_clamp,
                    mirrored_x=mirrored_x)

"""The input families of tests/cell_fit_cases.py on the CPU: each reaches the branch of the eigen-solver or of fit_plane that it is named
for (the oracle's trace says so), and the oracle deserves to be the reference on them (numpy agrees).  tests/test_gpu_math.py then
holds the device to the oracle on the same bits."""
import numpy as np
import pytest

import cell_fit_cases as K

SEED = K.SEED
EPS = K.EPS


@pytest.fixture(scope="module")
def solved(oracle_mod):
    """family -> (matrices, eigenvalues, eigenvectors, iterations, traces) of the oracle."""
    out = {}
    for name, make in K.SOLVER_FAMILIES.items():
        mats = make(SEED)
        r = [oracle_mod.eigen3_trace(K.full(m)) for m in mats]
        out[name] = (mats, np.array([x[0] for x in r]), np.array([x[1] for x in r]), np.array([x[2] for x in r]),
                     np.array([x[3] for x in r], np.uint32))
    return out


def _has(trace, bit):
    return (trace & bit) != 0


def test_trace_leaves_the_result_alone(oracle_mod, solved):
    for name, (mats, ev, vec, it, _) in solved.items():
        for i in range(0, len(mats), 5):
            e0, v0, i0 = oracle_mod.eigen3(K.full(mats[i]))
            assert np.array_equal(e0.view(np.uint64), ev[i].view(np.uint64)) and np.array_equal(v0.view(np.uint64), vec[i].view(np.uint64))
            assert i0 == it[i], name


def test_solver_families_have_their_size(solved):
    for name, (mats, *_) in solved.items():
        assert len(mats) >= 256 and mats.shape[1] == 6, name


def test_dense_never_enters_block_12(oracle_mod, solved):
    """What test_eigen3_bitwise_vs_oracle's construction does not reach: block [1,2], the e2 == 0 shift, the td == 0 shift, the cap."""
    tr = solved["dense"][4]
    assert not _has(tr, oracle_mod.TRACE_BLOCK12 | oracle_mod.TRACE_SHIFT_E2_ZERO | oracle_mod.TRACE_SHIFT_TD_ZERO | oracle_mod.TRACE_ITERATION_CAP).any()
    assert _has(tr, oracle_mod.TRACE_BLOCK01).all() and _has(tr, oracle_mod.TRACE_BLOCK02).any()
    assert solved["dense"][3].max() <= 12


def test_block_12_families(oracle_mod, solved):
    for name in ("x_decoupled", "td_zero"):
        tr = solved[name][4]
        assert _has(tr, oracle_mod.TRACE_BLOCK12).all(), name
        assert not _has(tr, oracle_mod.TRACE_BLOCK01 | oracle_mod.TRACE_BLOCK02).any(), name
    assert _has(solved["td_zero"][4], oracle_mod.TRACE_SHIFT_TD_ZERO).all()
    mats = solved["x_decoupled"][0]
    minors = mats[:, 2] * mats[:, 5] - mats[:, 4] ** 2
    assert (minors[0::2] < 0).any() and (mats[1::2, 0] > 0).all() and (minors[1::2] > 0).all()  # indefinite and positive definite


def test_rank1_reaches_every_block(oracle_mod, solved):
    """One matrix cannot visit all three blocks: block [1,2] needs s0 == 0, a subdiagonal that is zero stays zero, and block [0,1]
    needs s0 != 0.  What v v^T gives is block [0,2] followed by [1,2] (s0 deflates first) in some rows and by [0,1] in others."""
    tr = solved["rank1"][4]
    both = oracle_mod.TRACE_BLOCK02 | oracle_mod.TRACE_BLOCK12
    assert ((tr & both) == both).any()
    for bit in (oracle_mod.TRACE_BLOCK01, oracle_mod.TRACE_BLOCK02, oracle_mod.TRACE_BLOCK12):
        assert _has(tr, bit).any()
    assert not ((tr & 7) == 7).any()


def test_shift_underflow_takes_the_e2_zero_branch(oracle_mod, solved):
    tr = solved["shift_underflow"][4]
    assert _has(tr, oracle_mod.TRACE_SHIFT_E2_ZERO).all()
    assert _has(tr[0::2], oracle_mod.TRACE_BLOCK12).all() and _has(tr[1::2], oracle_mod.TRACE_BLOCK01).all()


def test_tiny_m20_takes_both_tridiagonalisations(oracle_mod, solved):
    tr = solved["tiny_m20"][4]
    skipped, reflected = _has(tr, oracle_mod.TRACE_TRIDIAG_SKIPPED), _has(tr, oracle_mod.TRACE_TRIDIAG_REFLECTED)
    assert np.all(skipped ^ reflected) and skipped.mean() > 0.25 and reflected.mean() > 0.25


def test_repeated_eigenvalues_need_no_step(solved):
    mats, ev, vec, it, _ = solved["repeated"]
    assert not it.any()
    want = np.sort(mats[:, [0, 2, 5]], axis=1)
    assert np.all(np.abs(ev - want) <= 2 * EPS * np.abs(want))  # (d / scale) * scale: two roundings
    assert np.array_equal(ev[:4], want[:4])


def test_non_finite_ends_at_the_cap(oracle_mod, solved):
    """A NaN anywhere and an infinite off-diagonal entry run the loop to its cap of 90 steps: 91 counted, eigenvalues left unsorted.
    An infinite DIAGONAL entry does not: the scale is infinite, the other entries become 0 and the diagonal NaN, so both subdiagonals
    deflate at once and no step runs."""
    mats, ev, vec, it, tr = solved["non_finite"]
    diag_inf = np.isinf(mats[:, [0, 2, 5]]).any(axis=1)
    assert diag_inf.sum() >= 6 * 16 - 1 and (~diag_inf).sum() >= 12 * 16
    assert _has(tr[~diag_inf], oracle_mod.TRACE_ITERATION_CAP).all() and (it[~diag_inf] == 91).all()
    assert not _has(tr[diag_inf], oracle_mod.TRACE_ITERATION_CAP).any() and not it[diag_inf].any()
    assert np.isnan(ev).any(axis=1).all()
    for pos in range(6):
        for bad in (np.isnan, np.isposinf, np.isneginf):
            assert bad(mats[:, pos]).sum() >= 16


@pytest.mark.parametrize("name", K.FINITE_SOLVER_FAMILIES)
def test_oracle_solver_against_numpy(solved, name):
    """test_eigen3_against_numpy's bound, 1e-14 of max|A|, on the eigenvalues, the residual and the orthogonality."""
    mats, ev, vec, _, _ = solved[name]
    worst = np.zeros(3)
    for m, e, v in zip(mats, ev, vec):
        a = K.full(m)
        s = np.abs(a).max() or 1.0
        a = a / s  # keeps A V within range at 1e300
        assert np.all(np.diff(e) >= 0)
        worst = np.maximum(worst, [np.abs(e / s - np.linalg.eigvalsh(a)).max(), np.abs(a @ v - v * (e / s)).max(), np.abs(v.T @ v - np.eye(3)).max()])
    print(name, "eigenvalues %.2e residual %.2e orthogonality %.2e" % tuple(worst))
    assert worst.max() < 1e-14


# ---- fit_plane -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fitted(oracle_mod):
    """family -> (rows, the oracle's ten outputs per row)."""
    return {name: (rows, np.array([oracle_mod.fit_plane(r[:9], int(r[9])) for r in rows]))
            for name, rows in ((name, make(SEED)) for name, make in K.FIT_FAMILIES.items())}


def test_fit_families_have_their_size(fitted):
    for name, (rows, out) in fitted.items():
        assert len(rows) >= 256 and rows.shape[1] == 10, name
    assert set(fitted["noisy_plane"][0][:, 9]) == set(K.NOISY_PLANE_COUNTS)


@pytest.mark.parametrize("name", list(K.FIT_FAMILIES))
def test_oracle_fit_plane_against_numpy(fitted, name):
    """The oracle entry's plumbing (order of the sums, of the outputs) against plain numpy.  The centroid and the covariance are checked
    in longdouble; the determinant test, the eigen-decomposition (numpy.linalg.eigh) and what follows from it in float64 on fit_plane's
    own Huygens covariance, since what cancels in it is part of the function.  Bounds: the normal to 1e-9 up to sign where the gap
    ev1 - ev0 exceeds 1e-6 ev2; d, mse and score to 1e-9 relative, to which is added what the 1e-14 max|A| that the solver test allows
    an eigenvalue does to a quantity built on a small one (mse: 1e-14 ev2 / n; score: its relative effect on ev1 and on max(ev0, 1e-6));
    d is a dot product with the centroid, so 'relative' is to max(d, |centroid|)."""
    rows, out = fitted[name]
    S, n = rows[:, :9], rows[:, 9]
    ld = np.longdouble
    Sl, nl = S.astype(ld), n.astype(ld)
    cen = (Sl[:, :3] / nl[:, None]).astype(np.float64)
    assert np.all(np.abs(out[:, 4:7] - cen) <= 2 * EPS * np.abs(cen))
    cov = K.huygens(rows)  # xx xy yy xz yz zz
    pairs = [(3, 0, 0), (6, 0, 1), (4, 1, 1), (8, 0, 2), (7, 1, 2), (5, 2, 2)]
    for col, (s2, i, j) in enumerate(pairs):
        exact = Sl[:, s2] - Sl[:, i] * Sl[:, j] / nl
        if i == j:
            exact = np.maximum(exact, 0)
        bound = 4 * EPS * (np.abs(Sl[:, s2]) + np.abs(Sl[:, i] * Sl[:, j]) / nl)
        assert np.all(np.abs(cov[:, col] - exact) <= bound), (name, col)
    det = K.determinant(cov)
    band = (np.abs(det) >= EPS / 2) & (np.abs(det) <= 2 * EPS)
    planar = out[:, 9] == 1.0
    assert np.array_equal(planar[~band], (np.abs(det) > EPS)[~band])
    assert set(out[:, 9]) <= {0.0, 1.0}
    if name != "det_edge":
        assert band.mean() <= 0.01
    # not planar: the cleared segment's defaults
    assert not out[~planar, 0:4].any() and np.all(out[~planar, 7] == np.finfo(np.float64).max) and not out[~planar, 8].any()

    mats = np.array([K.full(c) for c in cov[planar]])
    w, v = np.linalg.eigh(mats)
    o, c, cnt = out[planar], cen[planar], n[planar]
    wmax = np.abs(w).max(axis=1)
    ev0, ev1 = np.abs(w[:, 0]), np.abs(w[:, 1])
    gap = (w[:, 1] - w[:, 0]) > 1e-6 * wmax
    normal, v0 = o[:, 0:3], v[:, :, 0]
    assert np.all(np.abs(np.linalg.norm(normal, axis=1) - 1) < 1e-15)
    err = np.minimum(np.abs(normal - v0).max(axis=1), np.abs(normal + v0).max(axis=1))
    assert np.all(err[gap] <= 1e-9)
    assert np.all(o[:, 3] >= 0)
    d_ref = np.abs(np.einsum("ij,ij->i", v0, c))
    assert np.all(np.abs(o[:, 3] - d_ref)[gap] <= 1e-9 * np.maximum(d_ref, np.linalg.norm(c, axis=1))[gap])
    # the normal points away from the plane's side of the origin: n . centroid + d = 0
    assert np.all(np.abs(np.einsum("ij,ij->i", normal, c) + o[:, 3])[gap] <= 1e-9 * np.maximum(d_ref, np.linalg.norm(c, axis=1))[gap])
    slack = 1e-14 * wmax
    assert np.all(np.abs(o[:, 7] - ev0 / cnt) <= (1e-9 * ev0 + slack) / cnt)
    floor0 = np.maximum(ev0, 1e-6)
    score = ev1 / floor0
    ok = ev1 > 0
    assert np.all(np.abs(o[:, 8] - score)[ok] <= (score * (1e-9 + slack / ev1 + slack / floor0))[ok])
    # the comparison is not vacuous where the family is made of proper planes
    if name in ("noisy_plane", "d_sign", "score_clamp", "mirrored_x"):
        assert planar.mean() > 0.7 and gap.mean() > 0.7


def test_det_edge_gives_both_outcomes(fitted):
    rows, out = fitted["det_edge"]
    det = K.determinant(K.huygens(rows))
    planar = out[:, 9] == 1.0
    assert planar.sum() >= 32 and (~planar).sum() >= 32
    for sign in (1.0, -1.0):
        assert (det == sign * EPS).any() and not planar[det == sign * EPS].any()  # |det| == eps exactly: `<=` returns
        assert planar[(det * sign > EPS) & (det * sign < 4.5 * EPS)].any() and (~planar[(det * sign > 0) & (det * sign < EPS)]).any()
    assert (det == 0).sum() >= 32  # coplanar and collinear integer points


def test_huygens_clamp_acts(fitted):
    rows, out = fitted["huygens_clamp"]
    S, inv = rows[:, :9], 1.0 / rows[:, 9]
    axis = np.arange(len(rows)) % 3
    raw = S[np.arange(len(rows)), 3 + axis] - (S[np.arange(len(rows)), axis] ** 2) * inv
    assert (raw < 0).sum() >= 16 and (raw == 0).sum() >= 16
    assert np.all(K.huygens(rows)[:, [0, 2, 5]] >= 0)
    assert len(set(out[:, 9])) == 2


def test_d_sign_gives_both_signs_and_a_zero(oracle_mod, fitted):
    """d before the `d <= 0` flip, from the oracle's own eigenvector of fit_plane's covariance: positive, negative and zero; and the
    zero that comes out carries either sign."""
    rows, out = fitted["d_sign"]
    assert np.all(out[:, 9] == 1.0)
    cov, cen = K.huygens(rows), out[:, 4:7]
    raw = np.zeros(len(rows))
    for i, c in enumerate(cov):
        v = oracle_mod.eigen3(K.full(c))[1][:, 0]
        v = v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        raw[i] = -((v[0] * cen[i, 0] + v[1] * cen[i, 1]) + v[2] * cen[i, 2])
    assert (raw > 0).sum() >= 16 and (raw < 0).sum() >= 16 and (raw == 0).sum() >= 64
    zero = out[:, 3] == 0
    assert np.array_equal(zero, raw == 0)
    assert np.signbit(out[zero, 3]).any() and (~np.signbit(out[zero, 3])).any()
    assert np.signbit(out[zero, 4:7]).any()  # a centroid of -0 among them


def test_score_clamp_gives_both_sides(fitted):
    rows, out = fitted["score_clamp"]
    assert np.all(out[:, 9] == 1.0)
    ev0 = out[:, 7] * rows[:, 9]
    assert (ev0 < 1e-6).sum() >= 32 and (ev0 > 1e-6).sum() >= 32


def test_mirrored_x_works_in_block_12(oracle_mod, fitted):
    rows, out = fitted["mirrored_x"]
    cov = K.huygens(rows)
    assert not cov[:, [1, 3]].any() and np.all(cov[:, 4] != 0) and np.all(out[:, 9] == 1.0)
    tr = np.array([oracle_mod.eigen3_trace(K.full(c))[3] for c in cov], np.uint32)
    assert _has(tr, oracle_mod.TRACE_BLOCK12).all() and not _has(tr, oracle_mod.TRACE_BLOCK01 | oracle_mod.TRACE_BLOCK02).any()

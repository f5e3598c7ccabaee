"""The four MINPACK blocks of csrc/cape_pose_solve.h -- lm_rwupdt, lm_qrfac, lm_qrsolv, lm_lmpar -- and the select chains lm_gather /
lm_scatter, each on inputs of its own against numpy and scipy.linalg.  tests/test_pose_solve_host.py compares the whole minimiser with
MINPACK at the end of a solve, where a wrong Newton correction in lmpar or a wrong norm downdate in qrfac costs iterations and not
accuracy; here each block is held to the statement it restates.

tests/host/pose_lm_blocks.cpp wraps the blocks as extern "C" functions; it is compiled once with g++ (no sanitizer) into a shared
object and loaded with ctypes.  Every bound is of residual type, relative to ||J||_F^2, ||A||_F or the like: the largest value over
this file's own seeds was measured once (the *_MEASURED constants, printed by each test before it asserts, `pytest -s`), ten times that
is asserted (the factor's reason: the docstring of tests/test_pose_solve_host.py), and the bound is capped at CAP = 1e-10 so that a
wrong formula cannot hide under it.  The full-rank inputs have condition numbers below 1e4, which keeps numpy's own float64 references
inside the cap: test_the_references_alone checks that against products accumulated in np.longdouble.  CPU only."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1e-10
SEEDS = range(8)

# the largest values over this file's own seeds, each measured by the test named beside it, run on the host (x86-64, the wrapper built
# as the `blocks` fixture builds it: g++ -O2 -ffp-contract=off); the test prints the figure before it asserts
RWUPDT_MEASURED = 2.32e-15  # test_rwupdt_against_numpy: ||R^T R - J^T J||_F / ||J||_F^2, ||R^T qtf - J^T f|| / (||J||_F ||f||), ||diag R| - |diag qr(J)|| / ||J||_F
QRFAC_MEASURED = 3.35e-16   # test_qrfac_against_scipy: |rdiag| and acnorm against scipy / numpy, the Householder product against the stored triangle, over ||A||_F
QRSOLV_MEASURED = 1.67e-15  # test_qrsolv_against_lstsq: ||z - lstsq|| / ||lstsq||, ||S^T S - (R^T R + D^2)||_F / ||.||_F, the residual norms' relative difference
LMPAR_MEASURED = 1.88e-16   # test_lmpar_against_numpy: ||(R^T R + par D^2) P^T x - R^T qtb|| / ((||R||_F^2 + par max D^2) ||x|| + ||R^T qtb||)


def _bound(measured):
    assert 10 * measured <= CAP
    return 10 * measured


@pytest.fixture(scope="module")
def blocks(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    so = str(tmp_path_factory.mktemp("pose_lm_blocks") / "pose_lm_blocks.so")
    build = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", so,
                            os.path.join(ROOT, "tests", "host", "pose_lm_blocks.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    L = C.CDLL(so)
    L.pose_lm_lmpar.restype = C.c_double
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _conditioned(rng, m, cond):
    """m x 6 with singular values from 1 down to 1 / cond"""
    U, _ = np.linalg.qr(rng.normal(size=(m, 6)))
    V, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    return rng.uniform(0.5, 50.0) * (U * np.logspace(0.0, -np.log10(cond), 6)) @ V.T


def _long(a):
    return np.asarray(a, np.longdouble)


# ---- the references alone
def test_the_references_alone():
    """np.linalg.qr in float64 on the full-rank inputs of this file against products accumulated in np.longdouble: the reference's own
    error stays three orders of magnitude inside the cap"""
    worst = 0.0
    for seed in SEEDS:
        rng = np.random.default_rng(1000 + seed)
        for m, cond in ((6, 10.0), (9, 1e2), (384, 1e3), (6, 9e3)):
            J = _conditioned(rng, m, cond)
            assert np.linalg.cond(J) < 1e4
            Q, R = np.linalg.qr(J)
            scale = float(np.linalg.norm(J))
            worst = max(worst, float(np.linalg.norm(_long(Q) @ _long(R) - _long(J))) / scale,
                        float(np.linalg.norm(_long(R).T @ _long(R) - _long(J).T @ _long(J))) / scale ** 2,
                        float(np.linalg.norm(_long(Q).T @ _long(Q) - np.eye(6))))
    print(f"np.linalg.qr against longdouble products: {worst:.2e}")
    assert worst <= 1e-13


# ---- lm_gather / lm_scatter
def test_gather_and_scatter_on_every_permutation(blocks):
    v = np.array([3.0, -1.5, 0.25, 7.0, -11.0, 2.0 ** -40])
    out = np.zeros(6)
    for perm in itertools.permutations(range(6)):
        ipvt = np.array(perm, np.int32)
        blocks.pose_lm_gather(_p(v), _p(ipvt), _p(out))
        assert np.array_equal(out, v[ipvt]), perm
        blocks.pose_lm_scatter(_p(v), _p(ipvt), _p(out))
        want = np.zeros(6)
        want[ipvt] = v
        assert np.array_equal(out, want), perm


# ---- lm_rwupdt
def _rwupdt_inputs():
    """(name, J, f, the leading columns over which R is unique up to its rows' signs: where J^T J is singular the triangular factor
    behind the first dependent column is not, and Givens rotations and Householder reflections choose differently)"""
    for seed in SEEDS:
        rng = np.random.default_rng(2000 + seed)
        for m, cond in ((6, 1e2), (9, 1e3), (384, 5e3)):
            yield f"m={m} seed={seed}", _conditioned(rng, m, cond), rng.normal(size=m) * 30.0, 6
        J = _conditioned(rng, 9, 1e2)
        k = int(rng.integers(6))
        J[:, k] = 0.0
        yield f"zero column seed={seed}", J, rng.normal(size=9), k + 1
        J = _conditioned(rng, 9, 1e2)
        a, b = rng.choice(6, 2, replace=False)
        J[:, a] = J[:, b]
        yield f"equal columns seed={seed}", J, rng.normal(size=9), int(max(a, b)) + 1
        J = _conditioned(rng, 9, 1e2)
        J[rng.integers(9)] = 0.0
        yield f"zero row seed={seed}", J, rng.normal(size=9), 6
        J = _conditioned(rng, 9, 1e2)
        J[0] = 0.0  # (the first row: every rotation of it is the identity and R stays 0)
        yield f"zero first row seed={seed}", J, rng.normal(size=9), 6


def test_rwupdt_against_numpy(blocks):
    worst, where = 0.0, ""
    for name, J, f, unique in _rwupdt_inputs():
        J = np.ascontiguousarray(J)
        R, qtf = np.full((6, 6), np.nan), np.full(6, np.nan)
        blocks.pose_lm_rwupdt(len(J), _p(J), _p(f), _p(R), _p(qtf))
        assert not np.tril(R, -1).any(), f"{name}: R is upper triangular"
        scale = float(np.linalg.norm(J))
        errs = (float(np.linalg.norm(_long(R).T @ _long(R) - _long(J).T @ _long(J))) / scale ** 2,
                float(np.linalg.norm(_long(R).T @ _long(qtf) - _long(J).T @ _long(f))) / (scale * float(np.linalg.norm(f))),
                float(np.abs(np.abs(np.diag(R)) - np.abs(np.diag(np.linalg.qr(J)[1])))[:unique].max()) / scale)
        if max(errs) > worst:
            worst, where = max(errs), name
        if "zero column" in name:
            k = int(np.flatnonzero(~J.any(axis=0))[0])
            assert not R[:, k].any(), f"{name}: a zero column of J is a zero column of R"
    print(f"lm_rwupdt: largest relative residual {worst:.2e} ({where})")
    assert worst <= _bound(RWUPDT_MEASURED)


# ---- lm_qrfac
def _qrfac_inputs():
    for seed in SEEDS:
        rng = np.random.default_rng(3000 + seed)
        yield f"rank 6 seed={seed}", 6, _conditioned(rng, 6, 1e3)
        for rank in (3, 4, 5):
            A = _conditioned(rng, 6, 1e2)
            A[:, rng.choice(6, 6 - rank, replace=False)] = 0.0
            yield f"rank {rank} by zero columns seed={seed}", rank, A
            for kind, factor in (("equal", 1.0), ("nearly equal", 1.0 + 1e-9)):
                A = _conditioned(rng, 6, 1e2)
                cols = rng.permutation(6)
                for k in range(6 - rank):
                    A[:, cols[k]] = A[:, cols[5 - k % rank]] * factor
                yield f"rank {rank} by {kind} columns seed={seed}", rank, A
        # three independent columns, two of them once more scaled by 1 + 1e-9, and a sixth that leaves their span by 1e-9 only: after
        # three pivots the true remaining norms are ~1e-16, ~1e-16 and ~1e-9 of the columns' own, while the downdated norm of a
        # scaled copy is sqrt(a few eps) ~ 1e-8 of its own where it is not 0: only the recomputation picks the sixth column next
        A = np.zeros((6, 6))
        A[:, :3] = _conditioned(rng, 6, 10.0)[:, :3]
        A[:, 3], A[:, 4] = A[:, 0] * (1.0 + 1e-9), A[:, 1] * (1.0 + 1e-9)
        out = np.linalg.qr(A[:, :3], mode="complete")[0][:, 3]
        A[:, 5] = A[:, :3] @ rng.uniform(0.5, 1.0, 3) + 1e-9 * np.linalg.norm(A[:, :3]) * out
        yield f"copies beside a column 1e-9 off the span seed={seed}", 4, A[:, rng.permutation(6)]


def test_qrfac_against_scipy(blocks):
    from scipy.linalg import qr

    worst, where = 0.0, ""
    for name, rank, A in _qrfac_inputs():
        a = np.ascontiguousarray(A).copy()
        ipvt, rdiag, acnorm = np.full(6, -1, np.int32), np.full(6, np.nan), np.full(6, np.nan)
        blocks.pose_lm_qrfac(_p(a), _p(ipvt), _p(rdiag), _p(acnorm))
        scale = float(np.linalg.norm(A))
        assert sorted(ipvt.tolist()) == list(range(6)), f"{name}: ipvt is a permutation"
        want = np.abs(np.diag(qr(A, pivoting=True)[1]))
        # the stored Householder vectors v_j = a[j:, j], H_j = I - v v^T / v[0], applied to the pivoted columns in order
        B = _long(A[:, ipvt])
        for j in range(6):
            v = _long(a[j:, j])
            if v[0] != 0.0:
                B[j:] = B[j:] - np.outer(v, v @ B[j:]) / v[0]
        stored = np.triu(a, 1) + np.diag(rdiag)
        errs = (float(np.abs(np.abs(rdiag) - want).max()) / scale,
                float(np.abs(acnorm - np.sqrt((_long(A) ** 2).sum(axis=0)).astype(np.float64)).max()) / scale,
                float(np.linalg.norm(B - stored)) / scale)
        steps = np.diff(np.abs(rdiag)) / scale
        assert steps.max() <= _bound(QRFAC_MEASURED), f"{name}: |rdiag| is non-increasing, {np.abs(rdiag)}"
        if "zero columns" in name:
            assert not rdiag[rank:].any() and not np.triu(a)[rank:].any(), f"{name}: exactly zero columns give exactly zero rows"
        else:
            assert (np.abs(rdiag[:rank]) > 1e-10 * scale).all() and (np.abs(rdiag[rank:]) <= _bound(QRFAC_MEASURED) * scale).all(), f"{name}: the rank"
        if max(errs) > worst:
            worst, where = max(errs), name
    print(f"lm_qrfac: largest difference over ||A||_F {worst:.2e} ({where})")
    assert worst <= _bound(QRFAC_MEASURED)


# ---- lm_qrsolv
def _stacked_lstsq(R, pdiag, qtb):
    S = np.vstack([np.triu(R), np.diag(pdiag)])
    b = np.concatenate([qtb, np.zeros(6)])
    z = np.linalg.lstsq(S, b, rcond=None)[0]
    return z, float(np.linalg.norm(S @ z - b)), S, b


def _qrsolv(blocks, R, pdiag, qtb):
    r = np.triu(R).copy()
    r += np.tril(np.full((6, 6), np.nan), -1)  # (the strict lower triangle is the block's to write: whatever is there is not read)
    z, sdiag = np.full(6, np.nan), np.full(6, np.nan)
    blocks.pose_lm_qrsolv(_p(r), _p(np.ascontiguousarray(pdiag)), _p(np.ascontiguousarray(qtb)), _p(z), _p(sdiag))
    assert np.array_equal(np.triu(r), np.triu(R)), "the upper triangle comes back as it went in"
    return z, sdiag, np.tril(r, -1).T + np.diag(sdiag)


def test_qrsolv_against_lstsq(blocks):
    from scipy.linalg import qr

    worst, where = 0.0, ""
    for seed in SEEDS:
        rng = np.random.default_rng(4000 + seed)
        # full rank, every pdiag positive; then some of them 0
        for name, zeros in (("full rank", 0), ("full rank, two pdiag 0", 2)):
            R = np.linalg.qr(_conditioned(rng, 9, 1e3))[1]
            pdiag = rng.uniform(0.05, 2.0, 6) * np.abs(R).max()
            pdiag[rng.choice(6, zeros, replace=False)] = 0.0
            qtb = rng.normal(size=6) * 10.0
            z, sdiag, S = _qrsolv(blocks, R, pdiag, qtb)
            ref, res_ref, stacked, b = _stacked_lstsq(R, pdiag, qtb)
            gram = _long(np.triu(R)).T @ _long(np.triu(R)) + np.diag(_long(pdiag) ** 2)
            errs = (float(np.linalg.norm(z - ref) / np.linalg.norm(ref)), float(np.linalg.norm(_long(S).T @ _long(S) - gram) / np.linalg.norm(gram)),
                    abs(float(np.linalg.norm(stacked @ z - b)) - res_ref) / float(np.linalg.norm(b)))
            if max(errs) > worst:
                worst, where = max(errs), f"{name} seed={seed}"
        # singular R = [R11 R12; 0 0] from a pivoted factorisation of a matrix of rank 4, and pdiag = 0: z2 = 0 and z1 = R11^-1 qtb1 is a
        # minimiser of the stacked system (its first block's residual is 0), so the residual norm is lstsq's although z is not its
        # minimum-norm z; with R12 = 0 (zero columns) the same holds for a pdiag that is positive on the leading part
        for name, leading in (("singular, pdiag 0", 0.0), ("singular by zero columns, pdiag 0 behind", 1.0)):
            J = _conditioned(rng, 9, 1e2)
            if leading:
                J[:, [1, 4]] = 0.0
            else:
                J[:, 1], J[:, 4] = J[:, 0], J[:, 2] - J[:, 3]
            R = qr(J, mode="economic", pivoting=True)[1]
            R[4:] = 0.0
            pdiag = np.concatenate([leading * rng.uniform(0.05, 2.0, 4), np.zeros(2)])
            qtb = rng.normal(size=6) * 10.0
            z, sdiag, S = _qrsolv(blocks, R, pdiag, qtb)
            ref, res_ref, stacked, b = _stacked_lstsq(R, pdiag, qtb)
            assert not z[4:].any() and not sdiag[4:].any() and z[:4].all(), f"{name} seed={seed}: the trailing components are 0"
            err = abs(float(np.linalg.norm(stacked @ z - b)) - res_ref) / float(np.linalg.norm(b))
            if err > worst:
                worst, where = err, f"{name} seed={seed}"
    print(f"lm_qrsolv: largest relative difference {worst:.2e} ({where})")
    assert worst <= _bound(QRSOLV_MEASURED)


# ---- lm_lmpar
def _dxnorm(R, pd, qtb, par):
    """||D x|| of the numpy solution of (R^T R + par D^2) z = R^T qtb (pivoted order), through the stacked least-squares system"""
    S = np.vstack([R, np.sqrt(par) * np.diag(pd)])
    z = np.linalg.lstsq(S, np.concatenate([qtb, np.zeros(6)]), rcond=None)[0]
    return float(np.linalg.norm(pd * z))


def _par_at(R, pd, qtb, target):
    """the par at which ||D x(par)|| = target, by bisection on log par (||D x|| decreases in par)"""
    lo, hi = 1e-30, 1e30
    for _ in range(240):
        mid = float(np.sqrt(lo) * np.sqrt(hi))
        if _dxnorm(R, pd, qtb, mid) > target:
            lo = mid
        else:
            hi = mid
    return float(np.sqrt(lo) * np.sqrt(hi))


def _lmpar_inputs():
    from scipy.linalg import qr

    for seed in SEEDS:
        rng = np.random.default_rng(5000 + seed)
        for kind in ("full rank, pivoted", "full rank, ipvt identity", "rank 4 by zero columns", "rank 4 by equal columns"):
            J = _conditioned(rng, 9, 1e2)
            b = rng.normal(size=9) * 20.0
            if "zero columns" in kind:
                J[:, rng.choice(6, 2, replace=False)] = 0.0
            if "equal columns" in kind:
                cols = rng.permutation(6)
                J[:, cols[0]], J[:, cols[1]] = J[:, cols[2]], J[:, cols[3]]
            if "identity" in kind:
                Q, R = np.linalg.qr(J)
                ipvt = np.arange(6, dtype=np.int32)
            else:
                Q, R, piv = qr(J, mode="economic", pivoting=True)
                ipvt = piv.astype(np.int32)
                assert not np.array_equal(ipvt, np.arange(6))
            rank = 4 if "rank 4" in kind else 6
            R[rank:] = 0.0  # (rows that are rounding after a pivoted factorisation of a rank-4 matrix: the block tests its diagonal for 0)
            qtb = Q.T @ b
            diag = np.linalg.norm(J, axis=0) if seed % 2 else rng.uniform(0.5, 2.0, 6)
            diag[diag == 0.0] = 1.0
            pd = diag[ipvt]
            # ||D x|| as par -> 0: the Gauss-Newton step of a full-rank R; of a singular one the least ||D x|| among its minimisers,
            # which no positive par exceeds, so delta stays below it (between it and the basic solution's length the block ends on
            # its exceptional exit, which the 10 % rule does not describe)
            longest = _dxnorm(R, pd, qtb, 1e-26 * float(np.linalg.norm(R)) ** 2)
            for share, par_in in ((0.02, 0.0), (0.3, 0.0), (0.8, 0.0), (0.3, 1e3), (0.3, 1e-9), (1.05, 0.0), (3.0, 1.0)):
                if rank < 6 and share > 1.0:
                    continue
                yield f"{kind}, delta {share} of the longest step, par {par_in} seed={seed}", R, ipvt, diag, qtb, share * longest, par_in, rank


def test_lmpar_against_numpy(blocks):
    worst, where, n_zero, n_positive = 0.0, "", 0, 0
    for name, R, ipvt, diag, qtb, delta, par_in, rank in _lmpar_inputs():
        x = np.full(6, np.nan)
        r = np.ascontiguousarray(np.triu(R)).copy()
        par = blocks.pose_lm_lmpar(_p(r), _p(ipvt), _p(diag), _p(np.ascontiguousarray(qtb)), C.c_double(delta), C.c_double(par_in), _p(x))
        assert np.isfinite(x).all() and par >= 0.0, name
        pd, z = diag[ipvt], x[ipvt]  # (P^T x and P^T D P)
        U = _long(np.triu(R))
        rhs = U.T @ _long(qtb)
        res = float(np.linalg.norm((U.T @ U + par * np.diag(_long(pd) ** 2)) @ _long(z) - rhs))
        err = res / ((float(np.linalg.norm(R)) ** 2 + par * float(pd.max()) ** 2) * float(np.linalg.norm(z)) + float(np.linalg.norm(rhs)))
        if err > worst:
            worst, where = err, name
        dxnorm = float(np.linalg.norm(diag * x))
        if par == 0.0:
            n_zero += 1
            assert dxnorm <= 1.1 * delta * (1 + 1e-12), f"{name}: the Gauss-Newton step is within the bound"
            assert _dxnorm(np.triu(R), pd, qtb, 0.0) <= 1.1 * delta * (1 + 1e-9) or rank < 6, f"{name}: numpy's Gauss-Newton step too"
        else:
            n_positive += 1
            assert abs(dxnorm - delta) <= 0.1 * delta * (1 + 1e-12), f"{name}: ||D x|| {dxnorm} against delta {delta}"
            low, high = _par_at(np.triu(R), pd, qtb, 1.1 * delta), _par_at(np.triu(R), pd, qtb, 0.9 * delta)
            assert low * (1 - 1e-6) <= par <= high * (1 + 1e-6), f"{name}: par {par} outside [{low}, {high}]"
        if rank < 6:
            assert par > 0.0 and not np.array_equal(ipvt, np.arange(6)), name
    print(f"lm_lmpar: largest relative residual of the normal equations {worst:.2e} ({where}); par = 0 in {n_zero} cases, positive in {n_positive}")
    assert n_zero >= len(SEEDS) and n_positive >= 10 * len(SEEDS)
    assert worst <= _bound(LMPAR_MEASURED)

"""cape_host_pose_solve and cape_host_pose_select, the host twins of cape_map_pose_solve and cape_map_pose_select, without a device.

The minimiser (MINPACK's lmstr driver over forward differences, csrc/cape_pose_solve.h) is measured against scipy.optimize.leastsq,
which wraps MINPACK's lmdif with the same tolerances, on a numpy restatement of the residual function written here: the pose of x
(quaternion of the coefficients, normalised, toRotationMatrix, the rigid inverse), plane_to_camera, reduced * 1.0 / 3.0 in pair order.
lmstr folds the Jacobian's rows by Givens rotations where lmdif factors the dense matrix by pivoted Householder reflections, so the two
agree to rounding at every step and to the termination tolerances at the end, not bit for bit: the largest differences over this
file's own problems were measured once (the *_MEASURED constants below) and ten times that is asserted -- ten and not two because the
tail is heavy: reversing the row order in scipy alone, which changes rounding only, moves the end point by a median of 9e-8 mm but by
up to 6.5e-4 mm.  The exact cases (statuses, refusals, the pivoted qrfac branch, the selection rule) are asserted as such.

Off the default path the same comparison runs per parameter set (mode = 2, gtol, zero and loose tolerances, epsfcn, a step bound that
binds) under three camera bases, with the stop codes MINPACK itself ends on; the two rank-deficient problems are compared with
MINPACK in fnorm and in the coordinates that must not move; CAPE_POSE_SOLVE_NOT_FINITE is reached at both of its sites.  Every
assertion on scipy alone stands in a test of its own, in front of the test that looks at the twin.  The blocks of the minimiser have
tests/test_pose_lm_blocks_host.py.  CPU only."""
import math

import numpy as np
import pytest

EPS = float(np.sqrt(np.finfo(np.float64).eps))
SIZES = (3, 3, 3, 3, 3, 3, 4, 4, 5, 5, 39, 128)  # subset sizes of one frame's problems: half of them three pairs
FRAMES = 8

# the largest differences between the twin and scipy over problems() below (measured with this file on the host; printed by
# test_twin_against_scipy before it asserts)
POSITION_MEASURED = 2.11e-3    # mm (on a three-pair problem whose minimum lies 3.2 m from its start)
COEFFICIENT_MEASURED = 7.80e-10
FNORM_MEASURED = 3.26e-11      # relative


def pose_of(x, C=np.eye(3)):
    """the world-to-camera matrix of x as csrc/cape_pose_solve.h states it"""
    alpha = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]
    divider = 1.0 / (alpha + 1)
    q = np.array([2.0 * x[3] * divider, 2.0 * x[4] * divider, 2.0 * x[5] * divider, (1 - alpha) * divider])
    qw, qx, qy, qz = q / math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    tx, ty, tz = 2.0 * qx, 2.0 * qy, 2.0 * qz
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
    R = np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])
    # (ordered sums, no BLAS: the figures below do not depend on the machine's matrix kernels)
    M = np.array([[(C[r, 0] * R[0, c] + C[r, 1] * R[1, c]) + C[r, 2] * R[2, c] for c in range(3)] for r in range(3)])
    pw = [(C[r, 0] * x[0] + C[r, 1] * x[1]) + C[r, 2] * x[2] for r in range(3)]
    T = np.eye(4)
    T[:3, :3] = M.T
    T[:3, 3] = [-((M[0, r] * pw[0] + M[1, r] * pw[1]) + M[2, r] * pw[2]) for r in range(3)]
    return T


def planes_to_camera(T, planes):
    """utils::plane_to_camera on rows (normal, d)"""
    n0, n1, n2 = planes[:, 0], planes[:, 1], planes[:, 2]
    r = np.column_stack([(T[i, 0] * n0 + T[i, 1] * n1) + T[i, 2] * n2 for i in range(3)])
    m = [-((T[0, 3] * T[0, k] + T[1, 3] * T[1, k]) + T[2, 3] * T[2, k]) for k in range(3)]
    qd = ((m[0] * n0 + m[1] * n1) + m[2] * n2) + planes[:, 3]
    return r / np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])[:, None], qd


def residuals(x, map_rows, det_rows, C=np.eye(3)):
    """the LM functor: reduced[c] * 1.0 / 3.0, pair after pair"""
    qn, qd = planes_to_camera(pose_of(x, C), map_rows)
    return ((det_rows[:, 3:4] * det_rows[:, :3] - qd[:, None] * qn) * 1.0 / 3.0).reshape(-1)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def make_frame(seed, n=128, C=np.eye(3)):
    """a seeded synthetic map of n planes, all matched, seen under the camera basis C: (planes, map arrays, tracks, detections, the true
    x, the generator)"""
    import cape_amd

    rng = np.random.default_rng(seed)
    planes = np.array([[*_unit(rng), rng.uniform(500.0, 4000.0)] for _ in range(n)])
    P = np.zeros(n, cape_amd.MAP_PLANE_DTYPE)
    P["normal"], P["d"] = planes[:, :3], planes[:, 3]
    tracks = np.zeros(n, cape_amd.MAP_TRACK_DTYPE)
    for j in range(n):
        tracks[j]["covariance"] = np.diag(rng.uniform(1e-6, 4.0, 4))
        tracks[j]["id"] = 1000 + 7 * j
    arrays = (P, np.zeros(0, cape_amd.MAP_RING_DTYPE), np.zeros((0, 2)))
    x_true = np.concatenate([rng.uniform(-300.0, 300.0, 3), np.array([1.0, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, 3)])
    qn, qd = planes_to_camera(pose_of(x_true, C), planes)
    qn = qn + rng.normal(scale=1e-3, size=qn.shape)
    detected = np.column_stack([qn / np.linalg.norm(qn, axis=1)[:, None], qd + rng.normal(scale=2.0, size=n)])
    return planes, arrays, tracks, detected, x_true, rng


def words_of(kept_planes):
    w = [0, 0, 0, 0]
    for i in kept_planes:
        w[i >> 5] |= 1 << (i & 31)
    return w


@pytest.fixture(scope="module")
def host(host_binaries):
    import cape_amd

    return cape_amd


@pytest.fixture(scope="module")
def problems(host):
    """FRAMES seeded frames x len(SIZES) problems, each solved once by scipy and once by the twin"""
    from scipy.optimize import leastsq

    out = []
    for f in range(FRAMES):
        planes, arrays, tracks, detected, x_true, rng = make_frame(100 + f)
        n = len(planes)
        match = np.arange(n, dtype=np.int32)
        starts, subsets, picks = [], [], []
        for size in SIZES:
            pick = np.sort(rng.choice(n, size, replace=False))
            step = _unit(rng) * rng.uniform(20.0, 60.0)
            starts.append(x_true + np.concatenate([step, rng.uniform(-0.02, 0.02, 3)]))
            subsets.append(words_of(pick))
            picks.append(pick)
        solutions, poses, _ = host.host_pose_solve(arrays, tracks, match, detected, np.array(starts), np.array(subsets, np.uint32))
        for i, pick in enumerate(picks):
            ref = leastsq(residuals, starts[i], args=(planes[pick], detected[pick]), full_output=True, ftol=EPS, xtol=EPS, gtol=0.0,
                          maxfev=400, epsfcn=None, factor=100)
            out.append(dict(frame=f, size=len(pick), x0=starts[i], x_ref=ref[0], fnorm_ref=float(np.linalg.norm(ref[2]["fvec"])),
                            nfev_ref=int(ref[2]["nfev"]), ier=int(ref[4]), row=solutions[i], pose=poses[i]))
    return out


def test_scipy_converges_on_every_problem(problems):
    # (the reference alone, before the twin is looked at)
    assert all(p["ier"] in (1, 2, 3) for p in problems), sorted({p["ier"] for p in problems})
    assert sum(p["size"] == 3 for p in problems) * 2 == len(problems)
    travel = [float(np.linalg.norm(p["x_ref"][:3] - p["x0"][:3])) for p in problems]
    print(f"scipy: nfev {min(p['nfev_ref'] for p in problems)}..{max(p['nfev_ref'] for p in problems)}, travel {min(travel):.1f}..{max(travel):.1f} mm")
    assert max(travel) >= 30.0


def test_twin_against_scipy(problems):
    d_pos = max(float(np.abs(p["row"]["x"][:3] - p["x_ref"][:3]).max()) for p in problems)
    d_coef = max(float(np.abs(p["row"]["x"][3:] - p["x_ref"][3:]).max()) for p in problems)
    d_fnorm = max(abs(float(p["row"]["fnorm"]) - p["fnorm_ref"]) / p["fnorm_ref"] for p in problems)
    statuses = sorted({int(p["row"]["status"]) for p in problems})
    nfev = [int(p["row"]["nfev"]) for p in problems]
    print(f"twin vs scipy over {len(problems)} problems: |dposition| {d_pos:.3e} mm, |dcoefficient| {d_coef:.3e}, relative |dfnorm| {d_fnorm:.3e}; "
          f"statuses {statuses}, nfev {min(nfev)}..{max(nfev)}")
    assert set(statuses) <= {1, 2, 3}
    assert d_pos <= 10 * POSITION_MEASURED and d_coef <= 10 * COEFFICIENT_MEASURED and d_fnorm <= 10 * FNORM_MEASURED
    # the bound stays orders of magnitude below what the solver has to travel: one that does not move fails
    assert 10 * POSITION_MEASURED <= 60.0 * 1e-3 and 10 * COEFFICIENT_MEASURED <= 0.02 * 1e-3
    for p in problems:
        row = p["row"]
        assert row["n_pairs_used"] == p["size"] and row["flags"] == 0 and row["iterations"] >= 1
        assert row["fnorm"] <= row["fnorm0"]
        # the pose that goes with the row is the pose of its x, to the bit
        assert np.array_equal(p["pose"], pose_of(row["x"]))
        assert np.array_equal(p["pose"][3], [0, 0, 0, 1])


# ---- off the default path: the camera basis, mode = 2, gtol, the stop codes of zero and of loose tolerances, epsfcn, the step bound
PERMUTATION = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])  # a signed permutation: its products are exact
ROTATED = np.array([[math.cos(0.3), -math.sin(0.3), 0.0], [math.sin(0.3), math.cos(0.3), 0.0], [0.0, 0.0, 1.0]]) @ PERMUTATION  # M = C R rounds
BASES = {"identity": np.eye(3), "permutation": PERMUTATION, "rotated": ROTATED}
OFF_SIZES = (3, 5, 39)
SMALL_FACTOR = 0.01  # (0.1 and 1.0 never bind the first step on these problems: test_scipy_alone_off_the_defaults asserts that this one does)
PARAMETER_SETS = {  # name: what both solvers are given beside the defaults; mode = 2 is scipy's diag = ones
    "defaults": {},
    # (with factor = 100 the step bound never binds on these problems, par stays 0 and the scaling never reaches the step: mode = 2
    # alone gives the default's x and nfev bit for bit.  Under SMALL_FACTOR the bound binds and the scaling decides the step)
    "mode=2": dict(mode=2, factor=SMALL_FACTOR),
    "gtol=1e-3": dict(gtol=1e-3),
    "ftol=xtol=0": dict(ftol=0.0, xtol=0.0),
    "ftol=1e-4, xtol=0": dict(ftol=1e-4, xtol=0.0),
    "ftol=0, xtol=1e-4": dict(ftol=0.0, xtol=1e-4),
    "epsfcn=1e-8": dict(epsfcn=1e-8),
    "small factor": dict(factor=SMALL_FACTOR),
}
CONVERGED = {1, 2, 3}
STATUSES = {"defaults": CONVERGED, "mode=2": CONVERGED, "gtol=1e-3": {4}, "ftol=1e-4, xtol=0": {1}, "ftol=0, xtol=1e-4": {2}, "epsfcn=1e-8": CONVERGED,
            "small factor": CONVERGED}  # ("ftol=xtol=0": the reference's own code, or both among the stringent-tolerance codes 6, 7, 8)
# the two rows that stop early, far from the minimum (see test_twin_against_scipy_off_the_defaults)
EARLY_STOP = ("gtol=1e-3", "ftol=1e-4, xtol=0")
# the largest differences between the twin and scipy per parameter set, over the three bases x 24 problems (measured with this file on
# the host; printed by test_twin_against_scipy_off_the_defaults before it asserts): |dposition| mm, |dcoefficient|, relative |dfnorm|
OFF_DEFAULT_MEASURED = {
    "defaults": (1.212e-04, 4.066e-10, 5.293e-11),
    "mode=2": (1.383e-04, 5.620e-10, 4.190e-12),
    "gtol=1e-3": (2.013e-04, 4.268e-10, 3.856e-10),
    "ftol=xtol=0": (1.212e-04, 3.349e-10, 5.293e-11),
    "ftol=1e-4, xtol=0": (1.121e-04, 3.809e-10, 3.822e-11),
    "ftol=0, xtol=1e-4": (1.121e-04, 3.809e-10, 3.822e-11),
    "epsfcn=1e-8": (1.057e-08, 9.797e-14, 9.680e-14),
    "small factor": (9.817e-05, 4.717e-10, 7.310e-12),
}


def _scipy_arguments(given):
    kw = dict(ftol=EPS, xtol=EPS, gtol=0.0, maxfev=400, epsfcn=None, factor=100)
    kw.update({k: v for k, v in given.items() if k != "mode"})
    if given.get("mode") == 2:
        kw["diag"] = np.ones(6)
    return kw


@pytest.fixture(scope="module")
def off_default_frames():
    """per basis FRAMES seeded frames whose detections were made under that basis, each with one problem per size of OFF_SIZES"""
    out = {}
    for basis, C in BASES.items():
        out[basis] = []
        for f in range(FRAMES):
            planes, arrays, tracks, detected, x_true, rng = make_frame(200 + f, C=C)
            picks = [np.sort(rng.choice(len(planes), size, replace=False)) for size in OFF_SIZES]
            starts = np.array([x_true + np.concatenate([_unit(rng) * rng.uniform(20.0, 60.0), rng.uniform(-0.02, 0.02, 3)]) for _ in OFF_SIZES])
            out[basis].append(dict(planes=planes, arrays=arrays, tracks=tracks, detected=detected, picks=picks, starts=starts))
    return out


@pytest.fixture(scope="module")
def off_default_reference(off_default_frames):
    """scipy alone: {(parameter set, basis): [per problem x, fnorm, nfev, ier, x0]}"""
    from scipy.optimize import leastsq

    out = {}
    for basis, frames in off_default_frames.items():
        for name, given in PARAMETER_SETS.items():
            rows = []
            for fr in frames:
                for pick, x0 in zip(fr["picks"], fr["starts"]):
                    ref = leastsq(residuals, x0, args=(fr["planes"][pick], fr["detected"][pick], BASES[basis]), full_output=True, **_scipy_arguments(given))
                    rows.append(dict(x0=x0, x=ref[0], fnorm=float(np.linalg.norm(ref[2]["fvec"])), nfev=int(ref[2]["nfev"]), ier=int(ref[4])))
            out[name, basis] = rows
    return out


def _twin_rows(host, frames, C, given):
    rows, poses = [], []
    for fr in frames:
        r, p, _ = host.host_pose_solve(fr["arrays"], fr["tracks"], np.arange(len(fr["planes"]), dtype=np.int32), fr["detected"], fr["starts"],
                                       np.array([words_of(pick) for pick in fr["picks"]], np.uint32), params=host.pose_solve_params(camera_basis=C, **given))
        rows.extend(r)
        poses.extend(p)
    return rows, poses


@pytest.fixture(scope="module")
def off_default_twin(host, off_default_frames):
    return {(name, basis): _twin_rows(host, off_default_frames[basis], BASES[basis], given) for basis in BASES for name, given in PARAMETER_SETS.items()}


def test_scipy_alone_off_the_defaults(off_default_reference):
    # (the reference alone, before the twin is looked at: every row of the table holds for MINPACK itself)
    ref = off_default_reference
    for (name, basis), rows in ref.items():
        ier, nfev = sorted({r["ier"] for r in rows}), [r["nfev"] for r in rows]
        print(f"scipy, {name}, {basis}: ier {ier}, nfev {min(nfev)}..{max(nfev)}")
        assert len(rows) == FRAMES * len(OFF_SIZES)
        if name == "ftol=xtol=0":
            assert set(ier) <= {6, 7, 8} and max(nfev) < 400
        else:
            assert set(ier) <= STATUSES[name], (name, basis, ier)
        travel = [float(np.linalg.norm(r["x"][:3] - r["x0"][:3])) for r in rows]
        assert max(travel) >= 30.0
    for basis in BASES:
        # the step bound of SMALL_FACTOR binds: it costs the reference evaluations; and the two early stops end before the default does
        default = [r["nfev"] for r in ref["defaults", basis]]
        assert any(a != b for a, b in zip([r["nfev"] for r in ref["small factor", basis]], default)), basis
        # ... and under that bound the scaling is read: diag = 1 gives another iterate than the columns' norms on every problem
        assert all(not np.array_equal(a["x"], b["x"]) for a, b in zip(ref["mode=2", basis], ref["small factor", basis])), basis
        assert any(a["nfev"] != b["nfev"] for a, b in zip(ref["mode=2", basis], ref["small factor", basis])), basis
        for name in EARLY_STOP:
            assert all(a["nfev"] <= b for a, b in zip(ref[name, basis], default)) and any(a["nfev"] < b for a, b in zip(ref[name, basis], default))


def test_twin_against_scipy_off_the_defaults(off_default_reference, off_default_twin):
    """every parameter set under every basis: the statuses the reference has, distances as test_twin_against_scipy takes them.  The two
    early stops (gtol = 1e-3; ftol = 1e-4 with xtol = 0) end where the iteration is still moving, and still need no more than the
    others: the twin stops at the reference's own evaluation, which is asserted, and the two are compared in full like every row"""
    failures = []
    for name in PARAMETER_SETS:
        d_pos = d_coef = d_fnorm = 0.0
        for basis in BASES:
            ref, (rows, poses) = off_default_reference[name, basis], off_default_twin[name, basis]
            for p, row in zip(ref, rows):
                d_pos = max(d_pos, float(np.abs(row["x"][:3] - p["x"][:3]).max()))
                d_coef = max(d_coef, float(np.abs(row["x"][3:] - p["x"][3:]).max()))
                d_fnorm = max(d_fnorm, abs(float(row["fnorm"]) - p["fnorm"]) / p["fnorm"])
            statuses = sorted({int(r["status"]) for r in rows})
            nfev = [int(r["nfev"]) for r in rows]
            print(f"twin, {name}, {basis}: statuses {statuses}, nfev {min(nfev)}..{max(nfev)}; scipy ier {sorted({p['ier'] for p in ref})}, "
                  f"nfev equal on {sum(int(r['nfev']) == p['nfev'] for p, r in zip(ref, rows))} of {len(rows)}")
            for p, row in zip(ref, rows):
                if name == "ftol=xtol=0":
                    assert row["status"] == p["ier"] or {int(row["status"]), p["ier"]} <= {6, 7, 8}
                    assert row["nfev"] < 400
                else:
                    assert int(row["status"]) in STATUSES[name], (name, basis, int(row["status"]))
                if name in EARLY_STOP:
                    assert row["status"] == p["ier"] and row["nfev"] == p["nfev"]
                assert row["flags"] == 0 and row["fnorm"] <= row["fnorm0"] and row["iterations"] >= 1
        want = OFF_DEFAULT_MEASURED[name]
        print(f"twin vs scipy, {name}: |dposition| {d_pos:.3e} mm, |dcoefficient| {d_coef:.3e}, relative |dfnorm| {d_fnorm:.3e}")
        if not (d_pos <= 10 * want[0] and d_coef <= 10 * want[1] and d_fnorm <= 10 * want[2]):
            failures.append(name)
        # the bound stays orders of magnitude below what the solver has to travel: one that does not move fails
        assert 10 * want[0] <= 60.0 * 1e-3 and 10 * want[1] <= 0.02 * 1e-3
    assert not failures, failures


def test_the_camera_basis_is_read(host, off_default_frames, off_default_twin):
    rows, poses = off_default_twin["defaults", "rotated"]
    for row, pose in zip(rows, poses):
        # the pose that goes with the row is the pose of its x under the basis, to the bit
        assert np.array_equal(pose, pose_of(row["x"], ROTATED)) and not np.array_equal(pose, pose_of(row["x"]))
    # the same inputs under the identity basis: another problem, another result
    other, _ = _twin_rows(host, off_default_frames["rotated"], np.eye(3), {})
    # (the minimum's fnorm is the same up to rounding: every rigid transform has coefficients under either basis)
    assert all(not np.array_equal(a["x"], b["x"]) and a.tobytes() != b.tobytes() for a, b in zip(rows, other))
    # ... and the permutation, whose products are exact, gives the pose of its x too
    rows, poses = off_default_twin["defaults", "permutation"]
    assert all(np.array_equal(pose, pose_of(row["x"], PERMUTATION)) for row, pose in zip(rows, poses))


def test_maxfev_of_seven_ends_with_status_five(host):
    from scipy.optimize import leastsq

    planes, arrays, tracks, detected, x_true, rng = make_frame(7)
    pick = np.array([3, 40, 99])
    x0 = x_true + np.array([30.0, -20.0, 25.0, 0.01, -0.015, 0.02])
    rows, _, _ = host.host_pose_solve(arrays, tracks, np.arange(128, dtype=np.int32), detected, x0[None], np.array([words_of(pick)], np.uint32),
                                      params=host.pose_solve_params(maxfev=7))
    ref = leastsq(residuals, x0, args=(planes[pick], detected[pick]), full_output=True, ftol=EPS, xtol=EPS, gtol=0.0, maxfev=7)
    assert ref[4] == 5 and rows[0]["status"] == 5
    assert rows[0]["nfev"] == 8  # (the start, a Jacobian of six, the first trial point: MINPACK tests maxfev after the trial)


def test_refusals(host):
    planes, arrays, tracks, detected, x_true, rng = make_frame(8)
    match = np.arange(128, dtype=np.int32)
    subsets = np.array([words_of([]), words_of([5]), words_of([5, 77]), words_of([5, 77, 100]), words_of([5, 77, 100])], np.uint32)
    starts = np.tile(x_true, (5, 1))
    starts[4, 4] = np.nan
    rows, poses, _ = host.host_pose_solve(arrays, tracks, match, detected, starts, subsets)
    assert list(rows["status"][:3]) == [host.POSE_SOLVE_TOO_FEW_PAIRS] * 3 and list(rows["n_pairs_used"]) == [0, 1, 2, 3, 3]
    assert rows[3]["status"] in (1, 2, 3)
    assert rows[4]["status"] == host.POSE_SOLVE_BAD_START
    for i in (0, 1, 2):  # a refused problem keeps its start, and its pose is the start's
        assert np.array_equal(rows[i]["x"], starts[i]) and rows[i]["nfev"] == 0 and rows[i]["fnorm"] == 0
        assert np.array_equal(poses[i], pose_of(starts[i]))
    assert np.isnan(rows[4]["x"][4]) and np.array_equal(rows[4]["x"][:4], starts[4][:4])
    # bits of unmatched kept planes are ignored
    unmatched = match.copy()
    unmatched[[9, 10]] = -1
    rows2, _, _ = host.host_pose_solve(arrays, tracks, unmatched, detected, starts[3:4], np.array([words_of([5, 9, 10, 77, 100])], np.uint32))
    assert rows2[0]["n_pairs_used"] == 3 and rows2[0].tobytes() == rows[3].tobytes()
    # a frame with an invalid feature; a frame the wide match flagged
    bad = detected.copy()
    bad[64, 1] = np.nan
    rows3, _, _ = host.host_pose_solve(arrays, tracks, match, bad, starts[3:4], subsets[3:4])
    assert rows3[0]["status"] == host.POSE_SOLVE_INVALID_FEATURE and rows3[0]["flags"] == host.POSE_SCORE_INVALID_FEATURE
    rows4, _, _ = host.host_pose_solve(arrays, tracks, match, detected, starts[3:4], subsets[3:4], frame_flags=host.MATCH_EXACT_OVERFLOW)
    assert rows4[0]["status"] == host.POSE_SOLVE_OVERFLOW and rows4[0]["n_pairs_used"] == 0
    # parameters out of range
    for bad_params in (dict(maxfev=0), dict(mode=3), dict(ftol=-1.0), dict(factor=float("nan"))):
        with pytest.raises(host.CapeError):
            host.host_pose_solve(arrays, tracks, match, detected, starts[3:4], subsets[3:4], params=host.pose_solve_params(**bad_params))


def test_a_match_entry_out_of_range_is_an_invalid_argument(host):
    """the pair builder the three twins share checks the match against the detected planes: an entry >= detected->n"""
    planes, arrays, tracks, detected, x_true, rng = make_frame(8, n=12)
    subsets = np.array([words_of(range(12))], np.uint32)
    rows, _, _ = host.host_pose_solve(arrays, tracks, np.arange(12, dtype=np.int32), detected, x_true[None], subsets)
    assert rows[0]["status"] in (1, 2, 3)  # (the frame itself solves)
    for entry in (12, 128, 2 ** 31 - 1):
        match = np.arange(12, dtype=np.int32)
        match[7] = entry
        with pytest.raises(host.CapeError, match=r"cape_host_pose_solve failed \(-1\)"):  # CAPE_ERR_INVALID_ARGUMENT
            host.host_pose_solve(arrays, tracks, match, detected, x_true[None], subsets)


def test_parallel_planes_take_the_pivoted_qrfac_branch(host):
    """three pairs whose map planes are parallel, seen from a start with the identity rotation: the residuals do not depend on the two
    in-plane coordinates at all, their forward differences are exactly 0, R has zero diagonal entries and lmstr calls qrfac"""
    import cape_amd

    n = 3
    P = np.zeros(n, cape_amd.MAP_PLANE_DTYPE)
    P["normal"], P["d"] = [0.0, 0.0, 1.0], [800.0, 1500.0, 2600.0]
    tracks = np.zeros(n, cape_amd.MAP_TRACK_DTYPE)
    for j in range(n):
        tracks[j]["covariance"] = np.eye(4)
    arrays = (P, np.zeros(0, cape_amd.MAP_RING_DTYPE), np.zeros((0, 2)))
    detected = np.array([[0.0, 0.0, 1.0, 790.0], [0.0, 0.0, 1.0, 1492.0], [0.0, 0.0, 1.0, 2589.0]])
    x0 = np.array([10.0, -20.0, 0.0, 1.0, 0.0, 0.0])
    rows, poses, n_rank_deficient = host.host_pose_solve(arrays, tracks, np.arange(n, dtype=np.int32), detected, x0[None],
                                                         np.array([words_of(range(n))], np.uint32))
    row = rows[0]
    print(f"parallel planes: status {row['status']}, nfev {row['nfev']}, fnorm {row['fnorm0']:.4g} -> {row['fnorm']:.4g}, x {row['x']}")
    assert n_rank_deficient == 1 and row["flags"] & host.POSE_SOLVE_RANK_DEFICIENT
    assert row["status"] > 0 and np.isfinite(row["x"]).all() and np.isfinite(poses).all() and np.isfinite(row["fnorm"])
    assert row["fnorm"] < row["fnorm0"]
    # a full-rank problem does not take the branch
    planes, arrays2, tracks2, det2, x_true, rng = make_frame(9)
    _, _, none = host.host_pose_solve(arrays2, tracks2, np.arange(128, dtype=np.int32), det2, x_true[None], np.array([words_of([1, 2, 3])], np.uint32))
    assert none == 0


def _tilted(a, b, d):
    n = np.array([a, b, 1.0])
    return [*(n / math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])), d]


# three parallel map planes and a start with the identity rotation under the identity basis.  Untilted: the Jacobian's columns of x, y
# and of the first coefficient (the rotation about the common normal) are exactly 0 at the start and stay so: rank 3.  Tilted: the
# detections lean by about 0.01 off the axis, each its own way, so the minimum is not at the start's rotation and the solver leaves
# the exactly degenerate configuration with its first step; x and y stay unobservable (a plane's distance does not depend on them).
PARALLEL_MAP = np.array([[0.0, 0.0, 1.0, 800.0], [0.0, 0.0, 1.0, 1500.0], [0.0, 0.0, 1.0, 2600.0]])
PARALLEL_START = np.array([10.0, -20.0, 0.0, 1.0, 0.0, 0.0])
RANK_DEFICIENT = {
    "untilted": np.array([[0.0, 0.0, 1.0, 790.0], [0.0, 0.0, 1.0, 1492.0], [0.0, 0.0, 1.0, 2589.0]]),
    "tilted": np.array([_tilted(0.01, 0.0, 790.0), _tilted(0.0, 0.01, 1492.0), _tilted(-0.007, -0.007, 2589.0)]),
}


@pytest.fixture(scope="module")
def rank_deficient_reference():
    from scipy.optimize import leastsq

    out = {}
    for name, detected in RANK_DEFICIENT.items():
        ref = leastsq(residuals, PARALLEL_START, args=(PARALLEL_MAP, detected), full_output=True, ftol=EPS, xtol=EPS, gtol=0.0, maxfev=400)
        out[name] = dict(x=ref[0], ier=int(ref[4]), nfev=int(ref[2]["nfev"]), fnorm0=float(np.linalg.norm(residuals(PARALLEL_START, PARALLEL_MAP, detected))),
                         fnorm=float(np.linalg.norm(ref[2]["fvec"])))
    return out


def test_scipy_alone_on_the_rank_deficient_problems(rank_deficient_reference):
    # (the reference alone, before the twin is looked at)
    for name, ref in rank_deficient_reference.items():
        print(f"scipy, {name}: ier {ref['ier']}, nfev {ref['nfev']}, fnorm {ref['fnorm0']:.4g} -> {ref['fnorm']:.4g}, x {ref['x'].tolist()}")
        assert ref["ier"] == 1 and ref["fnorm"] < 0.8 * ref["fnorm0"]
        assert np.array_equal(ref["x"][:2], PARALLEL_START[:2]), "MINPACK gives the unobservable directions a zero step"
    # the tilted problem's minimum is not at the start's rotation, and its iteration is the longer one
    assert np.abs(rank_deficient_reference["tilted"]["x"][3:] - PARALLEL_START[3:]).max() > 1e-3
    assert np.abs(rank_deficient_reference["untilted"]["x"][3:] - PARALLEL_START[3:]).max() < 1e-9
    assert rank_deficient_reference["tilted"]["nfev"] > rank_deficient_reference["untilted"]["nfev"]


@pytest.mark.parametrize("name", list(RANK_DEFICIENT))
def test_rank_deficient_problems_against_scipy(host, rank_deficient_reference, name):
    """x[3:] is not compared: the minimum is a one-parameter family, the rotation about the common normal is free"""
    import cape_amd

    ref = rank_deficient_reference[name]
    P = np.zeros(3, cape_amd.MAP_PLANE_DTYPE)
    P["normal"], P["d"] = PARALLEL_MAP[:, :3], PARALLEL_MAP[:, 3]
    tracks = np.zeros(3, cape_amd.MAP_TRACK_DTYPE)
    tracks["covariance"] = np.eye(4)
    arrays = (P, np.zeros(0, cape_amd.MAP_RING_DTYPE), np.zeros((0, 2)))
    rows, poses, n_rank_deficient = host.host_pose_solve(arrays, tracks, np.arange(3, dtype=np.int32), RANK_DEFICIENT[name], PARALLEL_START[None],
                                                         np.array([words_of(range(3))], np.uint32))
    row = rows[0]
    d_fnorm = abs(float(row["fnorm"]) - ref["fnorm"]) / ref["fnorm"]
    print(f"twin, {name}: status {row['status']}, nfev {row['nfev']}, fnorm {row['fnorm0']:.4g} -> {row['fnorm']:.4g}, x {row['x'].tolist()}; "
          f"relative |dfnorm| {d_fnorm:.3e}, scipy nfev {ref['nfev']}")
    assert n_rank_deficient == 1 and row["flags"] == host.POSE_SOLVE_RANK_DEFICIENT
    assert row["status"] in (1, 2, 3) and row["fnorm0"] == ref["fnorm0"]
    assert d_fnorm <= 10 * OFF_DEFAULT_MEASURED["defaults"][2]
    assert np.array_equal(row["x"][:2], PARALLEL_START[:2]), "the unobservable directions get a zero step"
    assert np.array_equal(poses[0], pose_of(row["x"]))


def test_not_finite_at_the_start_and_at_the_first_trial_point(host):
    """CAPE_POSE_SOLVE_NOT_FINITE has two sites.  The start: x[0] = 1e160 is a finite start (no refusal) whose residuals' squares
    overflow at the very first evaluation.  The trial point: a start of 2e154 in x[2] has a finite fnorm (about 1e154, its square below
    DBL_MAX) and a Jacobian whose coefficient columns are of that order too, and the first step's x + p is not finite, so it is not
    evaluated: nfev = 7.  (Found by a search on the twin over starts of 1e150 .. 2.2e154 in one position coordinate: some tens of
    some thousands of starts ended there, all of them above 1.2e154 and at the first trial point; none ended on a trial fnorm.)"""
    planes, arrays, tracks, detected, x_true, rng = make_frame(400)
    match = np.arange(128, dtype=np.int32)
    starts = np.tile(x_true, (3, 1))
    starts[0, 0], starts[1, 2] = 1e160, 2e154
    subsets = np.array([words_of([3, 40, 99])] * 3, np.uint32)
    rows, poses, _ = host.host_pose_solve(arrays, tracks, match, detected, starts, subsets)
    print(f"not finite: statuses {rows['status'].tolist()}, nfev {rows['nfev'].tolist()}, fnorm0 {rows['fnorm0'].tolist()}, fnorm {rows['fnorm'].tolist()}")
    a, b, c = rows
    assert a["status"] == host.POSE_SOLVE_NOT_FINITE == -6 and a["nfev"] == 1 and a["iterations"] == 0
    assert np.array_equal(a["x"], starts[0]) and np.isposinf(a["fnorm0"]) and a["n_pairs_used"] == 3 and a["flags"] == 0
    assert b["status"] == host.POSE_SOLVE_NOT_FINITE and b["nfev"] == 7 and b["iterations"] == 0
    assert np.array_equal(b["x"], starts[1]) and np.isfinite(b["fnorm0"]) and b["fnorm"] == b["fnorm0"] > 1e153
    assert c["status"] in (1, 2, 3), "the same problem from a start near the minimum converges"
    for row, pose, x0 in zip(rows, poses, starts):
        assert np.array_equal(pose, pose_of(x0 if row["status"] < 0 else row["x"]))


def test_the_slab_frame_of_the_device_test_on_the_host(host, oracle_mod):
    """the `slabs` fixture of tests/test_gpu_pose_solve.py without a device: the oracle's extraction of its depth frame, the polygon
    oracle's outlines, the host map matcher and the twin.  A change to the frame that loses a plane or a pair is found here, and so
    is what the fixture's pose is for: measured on the twin, a full-rank problem whose minimum is the identity pose ends in the
    pivoted branch, the same problem lifted by _slab_pose does not."""
    import polygon_oracle_py as P
    from cape_amd import synth
    from test_gpu_map_match import _w2c
    from test_gpu_pose_score import _det_planes
    from test_gpu_pose_solve import DEGENERATE_START, _slab_map, _slab_pose, _slab_problems, _slabs_and_facets, _starts

    P.build()
    found = oracle_mod.Oracle(640, 480, cylinders=False, **synth.DEFAULT_INTRINSICS).run(_slabs_and_facets())
    det = []
    for k in range(len(found.planes)):
        seg = found.segments[int(found.planes[k][19])]
        normal = np.array(seg[0:3])
        pol = P.Polygon.from_points(np.asarray(found.boundary[k]), normal, normal * (-float(seg[3])))
        assert not pol.threw and pol.valid and pol.boundary_length() >= 3
        det.append((np.array(found.planes[k][0:3]), float(found.planes[k][3]), np.array(pol.x_axis), np.array(pol.y_axis), np.array(pol.center),
                    np.array(pol.ring), float(pol.area)))
    planes, slabs = _slab_map(det)
    assert len(det) == 6 and len(slabs) == 3 == sum(abs(k[0][2]) > 0.999 for k in det)
    assert all(np.array_equal(np.abs(planes[i][0]), [0.0, 0.0, 1.0]) for i in slabs)
    w2c = _w2c(*_slab_pose())
    arrays = host.pack_map(planes)
    match, _ = host.host_match_map(arrays, det, w2c, None, host.MATCH_ALLOW_INDEX0)
    assert sorted(int(v) for v in match) == list(range(6)), "six pairs"
    tracks = np.zeros(6, host.MAP_TRACK_DTYPE)
    tracks["covariance"] = np.eye(4)

    class Frame:
        pass

    s = Frame()
    s.W2C, s.slabs, s.facets = w2c[None], slabs, [i for i in range(6) if i not in slabs]
    x0, subsets = _slab_problems(s, np.random.default_rng(420), 5)
    rows, _, n_rank_deficient = host.host_pose_solve(arrays, tracks, np.asarray(match, np.int32), _det_planes(det), x0[0], subsets[0])
    print(f"slabs on the host: statuses {rows['status'].tolist()}, flags {rows['flags'].tolist()}, nfev {rows['nfev'].tolist()}")
    assert n_rank_deficient == 1 and rows[5]["flags"] == host.POSE_SOLVE_RANK_DEFICIENT and not rows[np.arange(16) != 5]["flags"].any()
    assert rows[5]["status"] > 0 and np.array_equal(rows[5]["x"][:2], DEGENERATE_START[:2]) and np.isin(rows["status"], (1, 2, 3)).all()
    # the three facets alone, their map the exact lift of the detections: full rank, the minimum at the lifting pose.  Lifted by the
    # identity the iterate's position and last two coefficients go to 0, the steps sqrt(eps) |x_j| with them, a column's forward
    # differences come out exactly 0 and the last iterations pivot; lifted by _slab_pose they do not
    facets = np.array([words_of(s.facets)] * 4, np.uint32)
    for name, pose, flagged in (("identity", (np.eye(3), np.zeros(3)), True), ("_slab_pose", _slab_pose(), False)):
        exact, _ = _slab_map(det, pose)
        m, _ = host.host_match_map(host.pack_map(exact), det, _w2c(*pose), None, host.MATCH_ALLOW_INDEX0)
        starts = _starts(np.random.default_rng(421), _w2c(*pose)[None], 4)[0]
        rows, _, _ = host.host_pose_solve(host.pack_map(exact), tracks, np.asarray(m, np.int32), _det_planes(det), starts, facets)
        print(f"facets lifted by {name}: statuses {rows['status'].tolist()}, flags {rows['flags'].tolist()}, fnorm {rows['fnorm'].tolist()}, "
              f"|x| at the end {np.abs(rows['x'][:, [0, 1, 2, 4, 5]]).max(axis=1).tolist()}")
        assert np.isin(rows["status"], (1, 2, 3)).all() and (rows["fnorm"] < 1e-3).all()
        assert ((rows["flags"] == host.POSE_SOLVE_RANK_DEFICIENT) == flagged).all()


def _rows(host, entries, n_pairs):
    """hand-written score and solution rows: entries = [(status, score, n_inliers)]"""
    scores = np.zeros(len(entries), host.POSE_SCORE_DTYPE)
    solutions = np.zeros(len(entries), host.POSE_SOLUTION_DTYPE)
    for h, (status, score, n_inliers) in enumerate(entries):
        scores[h]["n_pairs"], scores[h]["score"], scores[h]["n_inliers"] = n_pairs, score, n_inliers
        scores[h]["inlier_words"] = [h + 1, 0, 0, 0]
        solutions[h]["status"], solutions[h]["x"] = status, np.arange(6) + 10.0 * h
    return scores, solutions


def test_selection_rule_on_hand_written_rows(host):
    # a tie within 0.1 decided by the inlier count: h = 1 has the same score and more inliers; h = 2 is within 0.1 with fewer
    S = host.host_pose_select(*_rows(host, [(1, 2.0, 4), (1, 1.95, 6), (1, 1.9, 5)], n_pairs=20))
    assert (S["best"], S["n_inliers"], S["score"], S["n_scanned"], S["flags"]) == (1, 6, 1.95, 3, 0)
    assert list(S["inlier_words"]) == [2, 0, 0, 0] and np.array_equal(S["x"], np.arange(6) + 10.0)
    # a greater score wins whatever its inlier count
    S = host.host_pose_select(*_rows(host, [(1, 2.0, 6), (1, 2.5, 3)], n_pairs=20))
    assert (S["best"], S["n_inliers"]) == (1, 3)
    # a score of exactly 1.0 is not skipped and is taken on the tie rule; below 1.0 is skipped
    S = host.host_pose_select(*_rows(host, [(1, 1.0 - 2.0 ** -53, 3), (1, 1.0, 3)], n_pairs=20))
    assert (S["best"], S["score"], S["n_inliers"]) == (1, 1.0, 3)
    S = host.host_pose_select(*_rows(host, [(1, 0.99, 3), (0, 3.0, 9), (-1, 3.0, 9), (5, 1.0, 0)], n_pairs=20))
    assert S["best"] == -1 and S["flags"] == host.POSE_SELECT_NO_CONSENSUS and S["n_scanned"] == 4 and S["score"] == 1.0
    assert not S["x"].any() and not S["inlier_words"].any()
    # skipped rows do not trigger the early stop: h = 3 is skipped although bestInliers already exceeds the share, h = 4 stops it
    many = [(1, 6.0, 18), (1, 1.5, 4), (1, 1.5, 4), (0, 9.0, 20), (1, 1.2, 3), (1, 9.0, 20)]
    S = host.host_pose_select(*_rows(host, many, n_pairs=20))
    assert (S["best"], S["n_scanned"], S["flags"]) == (0, 5, host.POSE_SELECT_EARLY_STOP)
    # a stop at h = 3 but not at h = 2
    S = host.host_pose_select(*_rows(host, [(1, 6.0, 18), (1, 1.5, 4), (1, 1.5, 4), (1, 1.5, 4), (1, 9.0, 20)], n_pairs=20))
    assert (S["best"], S["n_scanned"]) == (0, 4)
    # n_pairs = 5: 5 x (double)0.80f is a little above 4, its ceil is 5, and no count of inliers exceeds it: no stop
    assert 5 * float(np.float32(0.80)) > 4.0 and math.ceil(5 * float(np.float32(0.80))) == 5
    S = host.host_pose_select(*_rows(host, [(1, 5 / 3, 5)] * 4 + [(1, 1.9, 5), (1, 1.0, 1)], n_pairs=5))
    assert (S["best"], S["n_scanned"], S["flags"]) == (4, 6, 0)
    # ... where 10 pairs stop at 9 inliers (ceil(8.0000001) = 9 is not exceeded by 9, but by 10)
    S = host.host_pose_select(*_rows(host, [(1, 3.0, 9)] * 5, n_pairs=10))
    assert S["n_scanned"] == 5
    S = host.host_pose_select(*_rows(host, [(1, 10 / 3, 10)] * 5, n_pairs=10))
    assert S["n_scanned"] == 4 and S["flags"] == host.POSE_SELECT_EARLY_STOP


def test_refit_from_a_selection(host):
    planes, arrays, tracks, detected, x_true, rng = make_frame(11)
    match = np.arange(128, dtype=np.int32)
    sel = np.zeros(1, host.POSE_SELECTION_DTYPE)
    sel["best"], sel["x"], sel["inlier_words"] = 2, x_true + np.array([20.0, 10.0, -15.0, 0.01, 0.0, -0.01]), [0xFFFFFFFF] * 4
    rows, poses, _ = host.host_pose_solve(arrays, tracks, match, detected, selection=sel[0])
    direct, poses2, _ = host.host_pose_solve(arrays, tracks, match, detected, sel["x"], sel["inlier_words"])
    assert rows[0]["status"] in (1, 2, 3) and rows[0]["n_pairs_used"] == 128
    assert rows.tobytes() == direct.tobytes() and poses.tobytes() == poses2.tobytes()
    sel["best"] = -1
    rows, _, _ = host.host_pose_solve(arrays, tracks, match, detected, selection=sel[0])
    assert rows[0]["status"] == host.POSE_SOLVE_NO_SELECTION and rows[0]["n_pairs_used"] == 0 and rows[0]["nfev"] == 0


def test_rules_header_under_the_host_sanitizers(tmp_path):
    """tests/host/pose_solve_check.cpp: the rules header in a stand-alone program built with AddressSanitizer and UBSan"""
    import os
    import shutil
    import subprocess

    if shutil.which("g++") is None:
        pytest.skip("g++ is not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host_dir = os.path.join(root, "rgb-d-slam_amd", "host")
    exe = str(tmp_path / "pose_solve_check.exe")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + host_dir, "-I" + os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "host", "pose_solve_check.cpp"),
                            os.path.join(host_dir, "boundary_polygon.cpp")], capture_output=True, text=True)
    if build.returncode != 0 and "sanitizer" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("the sanitizer runtimes are not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "0 expectations missed" in run.stdout, run.stdout[-2000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def test_abi(hip_library, host):
    import ctypes as C
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    public = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "cape_hip.h")).read(), flags=re.S)
    for name in ("cape_map_pose_solve", "cape_copy_pose_solutions", "cape_pose_solve_device", "cape_map_pose_select", "cape_copy_pose_selection"):
        assert re.search(r"int %s\(cape_handle h" % name, public) and name in host.EXPORTED_SYMBOLS
    L = host.load_library()
    x = np.zeros(6)
    w = np.zeros(4, np.uint32)
    xp, wp = x.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)
    assert L.cape_map_pose_solve(None, 1, 1, xp, wp, None, 0, None) == -1 and b"null handle" in L.cape_last_error()
    assert L.cape_map_pose_solve(None, 1, 0, xp, wp, None, 0, None) == -1 and b"n_hypotheses" in L.cape_last_error()
    assert L.cape_map_pose_solve(None, 1, 1, xp, wp, None, 1 << 2, None) == -1 and b"unknown pose-solve flag" in L.cape_last_error()
    assert L.cape_map_pose_solve(None, 1, 2, None, None, None, host.POSE_SOLVE_FROM_SELECTION, None) == -1 and b"n_hypotheses must be 1" in L.cape_last_error()
    bad = host.pose_solve_params(maxfev=0)
    assert L.cape_map_pose_solve(None, 1, 1, xp, wp, bad.ctypes.data_as(C.c_void_p), 0, None) == -1 and b"parameter" in L.cape_last_error()
    assert L.cape_copy_pose_solutions(None, 1, None, None) == -1 and L.cape_map_pose_select(None, 1, None) == -1
    assert L.cape_copy_pose_selection(None, 1, None) == -1 and L.cape_pose_solve_device(None, None, None) == -1
    for name in ("map_pose_solve", "pose_solutions", "map_pose_select", "pose_selection"):
        assert callable(getattr(host.Extractor, name))
    assert callable(host.host_pose_solve) and callable(host.host_pose_select)

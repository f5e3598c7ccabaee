"""Device scalar math vs the CPU oracle / host libm, bit for bit (through cape_debug_eval of the C ABI)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_f64_sqrt_div_correctly_rounded():
    from cape_amd import debug_eval

    rng = np.random.default_rng(1)
    a = np.abs(rng.standard_normal(200000)) * 10.0 ** rng.integers(-8, 9, 200000)
    b = rng.standard_normal(200000) * 10.0 ** rng.integers(-8, 9, 200000)
    assert np.array_equal(_bits(debug_eval("sqrt", a)), _bits(np.sqrt(a)))
    assert np.array_equal(_bits(debug_eval("div", a, b)), _bits(a / b))
    f = (np.abs(rng.standard_normal(100000)) * 1e4).astype(np.float32)
    assert np.array_equal(debug_eval("sqrtf", f.astype(np.float64)).astype(np.float32).view(np.uint32),
                          np.sqrt(f).view(np.uint32))


def test_quantization_bitwise(oracle_mod):
    from cape_amd import debug_eval

    z = np.concatenate([np.linspace(0, 10000, 5001), [500.0, 1000.0, 2000.0, 4000.0]])
    ref = np.array([oracle_mod.depth_quantization(v) for v in z])
    assert np.array_equal(_bits(debug_eval("quant", z)), _bits(ref))


def test_acos_atan2_bins_match_host_libm():
    """ocml vs glibc may differ in the last ulp; what must agree is the histogram bin (histogram.hpp:48-54)."""
    from cape_amd import debug_eval

    rng = np.random.default_rng(2)
    n = rng.standard_normal((300000, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    th_d = debug_eval("acos", -n[:, 2])
    ph_d = debug_eval("atan2", n[:, 0], n[:, 1])
    th_h, ph_h = np.arccos(-n[:, 2]), np.arctan2(n[:, 0], n[:, 1])
    ulp = np.abs(_bits(th_d).astype(np.int64) - _bits(th_h).astype(np.int64))
    assert ulp.max() <= 2
    xq_d, xq_h = np.floor(19 * th_d / np.pi), np.floor(19 * th_h / np.pi)
    yq_d, yq_h = np.floor(19 * (ph_d + np.pi) / (2 * np.pi)), np.floor(19 * (ph_h + np.pi) / (2 * np.pi))
    assert np.array_equal(xq_d, xq_h) and np.array_equal(yq_d, yq_h)
    # exact special values
    sp = debug_eval("acos", np.array([1.0, -1.0, 0.0]))
    assert np.array_equal(_bits(sp), _bits(np.arccos(np.array([1.0, -1.0, 0.0]))))


def test_eigen3_bitwise_vs_oracle(oracle_mod):
    from cape_amd import debug_eval

    rng = np.random.default_rng(3)
    N = 4000
    mats = np.zeros((N, 6))
    refs = np.zeros((N, 12))
    for i in range(N):
        p = rng.standard_normal((400, 3)) * rng.uniform(0.01, 100, 3)
        if i % 7 == 0:
            p[:, 2] = 0.0  # degenerate direction
        c = p.T @ p
        mats[i] = [c[0, 0], c[1, 0], c[1, 1], c[2, 0], c[2, 1], c[2, 2]]
        ev, vec, _ = oracle_mod.eigen3(c)
        refs[i, :3] = ev
        refs[i, 3:] = vec.ravel()
    out = debug_eval("eigen3", mats)
    assert np.array_equal(_bits(out), _bits(refs))


# ---- the eigen-solver's second block and fit_plane at their edges ---------------------------------------------------------------
# The families of tests/cell_fit_cases.py; tests/test_cell_fit_cases.py asserts on the CPU, at the same seed, that each reaches the
# branch it is named for.  self_adjoint_eigen3 picks its QR step's code by a wave vote (__any(start != 0)): plain k = 0 code when no
# lane of the wave is in block [1,2], code on selected operands when one is.  debug_eval_kernel gives row i to thread i of 256-thread
# blocks, so rows 64 w ... 64 w + 63 share wave w: the company tests below choose a row's 63 neighbours by its position in the array.

def _bits_nan(a):
    """bit patterns with every NaN as one pattern: the payload of a generated NaN is the hardware's choice (x86 sets the sign bit of its
    default NaN, gfx950 does not); the NaN positions and everything that is not a NaN are compared bit for bit"""
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return b


def _oracle_eigen3(oracle_mod, mats):
    import cell_fit_cases as K

    refs = np.zeros((len(mats), 12))
    for i, m in enumerate(mats):
        ev, vec, _ = oracle_mod.eigen3(K.full(m))
        refs[i, :3] = ev
        refs[i, 3:] = vec.ravel()
    return refs


def _oracle_fit_plane(oracle_mod, rows):
    return np.array([oracle_mod.fit_plane(r[:9], int(r[9])) for r in rows])


def _mismatch(got, ref, rows):
    """the first rows that differ, for the failure message"""
    bad = np.flatnonzero((got != ref).any(axis=1))
    return "%d rows differ; first: %s" % (len(bad), [(int(i), rows[i].tolist(), np.flatnonzero(got[i] != ref[i]).tolist()) for i in bad[:3]])


def test_eigen3_edge_families_bitwise(oracle_mod):
    import cell_fit_cases as K
    from cape_amd import debug_eval

    failures = []
    for name, make in K.SOLVER_FAMILIES.items():
        mats = make(K.SEED)
        ref = _oracle_eigen3(oracle_mod, mats)
        out = debug_eval("eigen3", mats)  # returns: the loop is capped at 90 steps, NaN or not
        if name == "non_finite":
            assert np.isnan(ref).any(axis=1).all()
            if not np.array_equal(np.isnan(out), np.isnan(ref)):
                failures.append(name + ": NaN positions differ in rows %s" % np.flatnonzero((np.isnan(out) != np.isnan(ref)).any(axis=1))[:8].tolist())
            out, ref = _bits_nan(out), _bits_nan(ref)
        else:
            assert np.isfinite(ref).all()
            out, ref = _bits(out), _bits(ref)
        if not np.array_equal(out, ref):
            failures.append(name + ": " + _mismatch(out, ref, mats))
    assert not failures, "\n".join(failures)


def test_eigen3_wave_company_independent(oracle_mod):
    """A dense row (blocks [0,1] and [0,2] only) gives the same bits alone among its kind, beside one lane in block [1,2], beside 32 of
    them, and in a partial last wave; the [1,2] rows equal the oracle in every company, a wave full of them included."""
    import cell_fit_cases as K
    from cape_amd import debug_eval

    N = 4096
    dense, xdec = K.dense(K.SEED + 1, N), K.x_decoupled(K.SEED + 2, N)
    dense_ref, xdec_ref = _oracle_eigen3(oracle_mod, dense), _oracle_eigen3(oracle_mod, xdec)
    baseline = debug_eval("eigen3", dense)
    assert np.array_equal(_bits(baseline), _bits(dense_ref))
    row = np.arange(N)
    wave, lane = row // 64, row % 64
    one_lane = lane == wave % 64
    half = np.where(wave % 2 == 0, lane % 2 == 1, lane >= 32)
    for label, replaced in (("one lane", one_lane), ("half a wave", half), ("whole waves", np.ones(N, bool))):
        assert all(replaced.reshape(-1, 64).sum(axis=1) == {"one lane": 1, "half a wave": 32, "whole waves": 64}[label])
        mats = np.where(replaced[:, None], xdec, dense)
        out = debug_eval("eigen3", mats)
        assert np.array_equal(_bits(out[~replaced]), _bits(baseline[~replaced])), label + ": a dense row depends on its wave's company"
        assert np.array_equal(_bits(out[replaced]), _bits(xdec_ref[replaced])), label + ": " + _mismatch(_bits(out[replaced]), _bits(xdec_ref[replaced]), mats[replaced])
    # a partial last wave: the vote runs among the 17 lanes that the i >= n return leaves, one of them (row 325) in block [1,2]
    n = 64 * 5 + 17
    mats = np.where(one_lane[:n, None], xdec[:n], dense[:n])
    assert one_lane[320:n].sum() == 1
    out = debug_eval("eigen3", mats)
    assert out.shape == (n, 12)
    assert np.array_equal(_bits(out[~one_lane[:n]]), _bits(baseline[:n][~one_lane[:n]]))
    assert np.array_equal(_bits(out[one_lane[:n]]), _bits(xdec_ref[:n][one_lane[:n]]))


def test_fit_plane_edge_families_bitwise(oracle_mod):
    """All ten outputs.  Where the oracle says not planar, its cleared segment holds the defaults that cape_device.h documents for
    PlaneFit (zero normal, d = 0, mse = DBL_MAX, score = 0: test_cell_fit_cases.py asserts them of the oracle), so those rows too are
    compared in full, centroid included."""
    import cell_fit_cases as K
    from cape_amd import debug_eval

    failures = []
    for name, make in K.FIT_FAMILIES.items():
        rows = make(K.SEED)
        ref = _oracle_fit_plane(oracle_mod, rows)
        assert np.isfinite(ref).all()
        out = debug_eval("fit_plane", rows)
        if not np.array_equal(out[:, 9], ref[:, 9]):
            failures.append(name + ": planar differs in rows %s" % np.flatnonzero(out[:, 9] != ref[:, 9])[:8].tolist())
        off = out[:, 9] == 0.0
        if out[off, 0:4].any() or np.signbit(out[off, 0:4]).any() or np.any(out[off, 7] != np.finfo(np.float64).max) or out[off, 8].any():
            failures.append(name + ": a row that is not planar holds other than PlaneFit's defaults")
        if not np.array_equal(_bits(out), _bits(ref)):  # the sign of a zero d or normal component too
            failures.append(name + ": " + _mismatch(_bits(out), _bits(ref), rows))
    assert not failures, "\n".join(failures)


def test_fit_plane_wave_company_independent(oracle_mod):
    """Rows that return at the determinant test (their lanes sit out the solver's vote), mirrored_x rows (block [1,2]) and noisy_plane
    rows (blocks [0,1], [0,2]) in the same waves: each equals its result from a run among its own family only."""
    import cell_fit_cases as K
    from cape_amd import debug_eval

    edge = np.concatenate([K.det_edge(K.SEED + 3), K.huygens_clamp(K.SEED + 3)])
    families = [edge[_oracle_fit_plane(oracle_mod, edge)[:, 9] == 0.0][:320], K.mirrored_x(K.SEED + 4, 320), K.noisy_plane(K.SEED + 5, 320)]
    assert all(len(f) == 320 for f in families)
    alone = np.concatenate([debug_eval("fit_plane", f) for f in families])
    assert not alone[:320, 9].any() and alone[320:, 9].all()
    rows = np.concatenate(families)
    assert np.array_equal(_bits(alone), _bits(_oracle_fit_plane(oracle_mod, rows)))
    interleaved = np.arange(960).reshape(3, 320).T.ravel()  # lanes 0 1 2 3 ...: return, [1,2], dense, return ...
    shuffled = np.random.default_rng(K.SEED).permutation(960)
    lone = np.concatenate([np.arange(640, 960)[:63], [320], np.arange(0, 320)[:63], [321]])  # one [1,2] lane beside 63 of another kind
    for label, order in (("interleaved", interleaved), ("shuffled", shuffled), ("one lane", lone)):
        out = debug_eval("fit_plane", rows[order])
        assert np.array_equal(_bits(out), _bits(alone[order])), label + ": " + _mismatch(_bits(out), _bits(alone[order]), rows[order])

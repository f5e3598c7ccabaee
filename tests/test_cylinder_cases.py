"""The table of tests/cylinder_cases.py without a GPU: the oracle's trace of the cylinder branch on every case.  Each case reaches the
edges it claims, family A's candidates have exactly the N cells of their names, and the table as a whole covers the issue's list.  Run
with -s for the table (name, N, and every loop's m / wins / iterations / stop)."""
import numpy as np
import pytest

import cylinder_cases as CC


@pytest.fixture(scope="module")
def traced(oracle_mod):
    """name -> OracleResult of every case, computed once."""
    oracles, out = {}, {}
    for case in CC.CASES:
        key = (case.width, case.height)
        if key not in oracles:
            oracles[key] = oracle_mod.Oracle(case.width, case.height, cylinders=True, **CC.intrinsics(case))
        out[case.name] = oracles[key].run(case.build())
    return out


def test_table_shape():
    names = [c.name for c in CC.CASES]
    assert len(set(names)) == len(names)
    assert len(CC.CASES) <= 45
    for c in CC.CASES:
        assert (c.width, c.height) in CC.SIZES and c.width <= 1280 and c.height <= 960
        assert c.edges and c.edges <= CC.REQUIRED, c.name
        d = c.build()
        assert d.dtype == np.float32 and d.shape == (c.height, c.width) and np.isfinite(d).all() and (d >= 0).all(), c.name
        assert np.array_equal(d, c.build()), c.name + ": the builder is not a function of its literals"
    assert sorted(sum((CC.cases_of_size(*s) for s in CC.SIZES), []), key=lambda c: names.index(c.name)) == CC.CASES


def test_trace_is_consistent_with_the_results(traced):
    """The observer against what the oracle returned: labels, segments and seed outcomes."""
    for case in CC.CASES:
        r = traced[case.name]
        assert [c.n for c in r.cyl_candidates] == [int(a) for o, a in zip(r.seed_outcome, r.seed_activated) if o == 2], case.name
        labels = sum(c.segments - sum(c.plane_won) for c in r.cyl_candidates)
        assert labels == int(r.cyl_labels.max()), case.name
        assert len(r.segments) == int(np.sum(r.seed_outcome == 1)) + sum(sum(c.plane_won) for c in r.cyl_candidates), case.name
        for k, c in enumerate(r.cyl_candidates):
            loops = [lp for lp in r.cyl_loops if lp.candidate == k]
            assert c.score_passed == (c.end != CC.END_SCORE_GATE) and (c.score_passed or not loops), case.name
            assert len(c.inliers) == len(c.plane_won) == c.segments, case.name
            assert len(loops) == c.segments + (c.end == CC.END_BEST_UNDER_SIX), case.name
            left = c.n
            for lp, inl in zip(loops, c.inliers + [None]):
                assert lp.m == left and lp.wins == len(lp.win_iterations) <= lp.iterations <= CC.MAX_ITERATIONS, case.name
                assert lp.win_iterations == sorted(set(lp.win_iterations)) and (not lp.wins or lp.win_iterations[-1] <= lp.iterations), case.name
                assert not lp.early_stop or lp.win_iterations[-1] == lp.iterations, case.name
                assert lp.early_stop or lp.iterations == (CC.MAX_ITERATIONS if lp.m >= 3 else 0), case.name
                if inl is None:
                    assert lp.best < 6, case.name
                else:
                    assert lp.best == inl >= 6, case.name
                    left -= inl


def test_every_claimed_edge_is_reached(traced):
    for case in CC.CASES:
        r = traced[case.name]
        got = CC.reached(case, r)
        loops = ["%d/%d/%d%s" % (lp.m, lp.wins, lp.iterations, "s" if lp.early_stop else "") for lp in r.cyl_loops]
        print("%-28s %4dx%-4d N=%s  m/wins/iterations(s=stop): %s" % (case.name, case.width, case.height,
                                                                     ",".join(str(c.n) for c in r.cyl_candidates), " ".join(loops)))
        assert case.edges <= got, "%s does not reach %s" % (case.name, sorted(case.edges - got))


def test_family_a_has_one_candidate_of_exactly_n_cells(traced):
    sizes = []
    for case in CC.CASES:
        if not case.name.startswith("A "):
            continue
        r = traced[case.name]
        n = int(case.name.split("N=")[1])
        assert len(r.seeds) == 1 and len(r.cyl_candidates) == 1, case.name
        c = r.cyl_candidates[0]
        assert c.n == n and c.score_passed and c.segments == 1 and c.plane_won == [False], case.name
        assert int(np.count_nonzero(r.cyl_labels == 1)) == c.inliers[0] and len(r.segments) == 0, case.name
        sizes.append((case.width, n))
    assert sorted(sizes) == sorted([(640, n) for n in CC.A_SIZES_640] + [(1280, n) for n in CC.A_SIZES_1280])
    assert max(CC.A_SIZES_1280) > 2304  # three streamed trips beyond the 768-cell cache


def test_the_table_covers_the_list(traced):
    claimed = set().union(*(c.edges for c in CC.CASES))
    assert claimed | set(CC.UNREACHABLE) == CC.REQUIRED and not claimed & set(CC.UNREACHABLE)
    reached = set().union(*(CC.reached(c, traced[c.name]) for c in CC.CASES))
    assert CC.REQUIRED - set(CC.UNREACHABLE) <= reached

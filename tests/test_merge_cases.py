"""Every named case of tests/merge_cases.py reaches what it is named for, on the CPU oracle, with the cylinder branch off and on: the
conditions under which tests/test_gpu_merge_planes.py sends merging frames through each grow instance.  A generator that drifts fails
here, not silently on the GPU.  classify() is structural (label grid, merge labels, planar flags, output roots); the oracle alone
decides what merges."""
import numpy as np
import pytest

import merge_cases as M

CYL = [False, True]


def _classified(oracle_mod, name, cyl):
    r = M.oracle(name, cyl)
    return r, M.classify(r, M.grid(name)[0])


def test_classifier_on_hand_made_results():
    """classify() on label grids and merge labels written by hand: a 3 x 4 grid of cells (W = 80), sources without the last row and
    column, links to the right and below."""
    class R:
        pass

    r = R()
    # segments 1..4; 4 touches 3 only from the last column of the last row, where no cell is a source: not a link
    r.plane_labels = np.array([1, 1, 2, 0,
                               1, 3, 2, 0,
                               0, 3, 3, 4], np.int32)
    conn = M.connectivity(r.plane_labels, 80)
    assert conn.tolist() == [[False, True, True, False], [True, False, True, False], [True, True, False, False], [False] * 4]
    r.merge_labels = np.array([0, 0, 0, 3], np.uint32)
    r.segments = np.zeros((4, 20))
    r.segments[:, 19] = 1.0
    r.planes = np.zeros((1, 20))
    r.planes[0, 19] = 0.0
    c = M.classify(r, 80)
    assert (c["segments"], c["merged"], c["multi"], c["through_absorbed"], c["rejected"], c["dropped_roots"]) == (4, 2, 1, 0, 0, 1)
    assert c["absorbed_row_with_later_link"] == 1  # row 1 is absorbed and linked to column 2
    r.merge_labels = np.array([0, 0, 2, 3], np.uint32)
    c = M.classify(r, 80)
    assert (c["merged"], c["multi"], c["rejected"], c["dropped_roots"]) == (1, 0, 2, 2)
    # 70 segments in a row of cells, each linked to the next; 66 merged into 62 (straddle), 68 into 67 (a root beyond 63)
    n = 70
    r.plane_labels = np.concatenate([np.arange(1, n + 1), np.zeros(1), np.arange(1, n + 1), np.zeros(1)]).astype(np.int32)
    ml = np.arange(n)
    ml[66], ml[68] = 62, 67
    r.merge_labels = ml.astype(np.uint32)
    r.segments = np.ones((n, 20))
    r.planes = np.zeros((0, 20))
    c = M.classify(r, (n + 1) * M.CELL)
    assert (c["straddle64"], c["root_ge64"], c["row63_link"], c["through_absorbed"], c["merged"]) == (1, 1, 1, 1, 2)
    assert c["rejected"] == n - 1 - 1  # every link but 67-68


@pytest.mark.parametrize("cyl", CYL)
def test_small_cases(oracle_mod, cyl):
    r, c = _classified(oracle_mod, "pair", cyl)
    assert c["segments"] == 2 and c["merged"] == 1 and len(r.planes) == 1
    r, c = _classified(oracle_mod, "star", cyl)
    assert c["segments"] == 3 and c["multi"] >= 1 and c["through_absorbed"] == 0, "one root connected to both of the segments it absorbs"
    r, c = _classified(oracle_mod, "chain", cyl)
    assert c["segments"] == 3 and c["through_absorbed"] >= 1 and c["absorbed_row_with_later_link"] >= 1
    r, c = _classified(oracle_mod, "chain_reject", cyl)
    assert c["segments"] == 3 and c["merged"] >= 1 and c["rejected"] >= 1 and len(r.planes) == 2
    for name in ("pair", "star", "chain", "chain_reject"):
        assert len(M.oracle(name, cyl).cylinders) == 0 and M.classify(M.oracle(name, cyl), 640)["dropped_roots"] == 0


@pytest.mark.parametrize("cyl", CYL)
@pytest.mark.parametrize("name", sorted(M.LATTICE_COUNTS))
def test_lattice_counts(oracle_mod, name, cyl):
    r, c = _classified(oracle_mod, name, cyl)
    assert (c["segments"], c["merged"], len(r.planes)) == M.LATTICE_COUNTS[name]
    assert c["rejected"] >= 1, "a connected pair that is rejected next to the ones that merge"
    assert c["dropped_roots"] == 0 and c["nonplanar_roots"] == 0 and len(r.cylinders) == 0
    assert r.log_not_planar_after_merge == 0
    if c["segments"] > 64:
        assert c["straddle64"] >= 1, "a segment of the spill record absorbed by a root of the first record"
    if name.endswith("_lean"):
        assert c["segments"] > 64 and c["root_ge64"] >= 1, "a merge root in the spill record"
        assert c["row63_link"] >= 1, "row 63 linked to a column of the second adjacency word"


def test_frontal_lattices_keep_their_roots_in_the_first_record(oracle_mod):
    """Why the leaning lattices exist: a frontal strip is an exact plane in float32 and is seeded before every hinged strip, so with
    the table's parameters every merge root of a frame of more than 64 segments is one of the first 48 segments."""
    for name in ("lattice_12x8", "mid_12x8", "big_9x8"):
        assert _classified(oracle_mod, name, False)[1]["root_ge64"] == 0


@pytest.mark.parametrize("radius", [600, 900, 1400])
def test_lattice_with_a_cylinder(oracle_mod, radius):
    name = f"lattice_cyl_{radius}"
    off, c_off = _classified(oracle_mod, name, False)
    on, c_on = _classified(oracle_mod, name, True)
    for r, c in ((off, c_off), (on, c_on)):
        assert (c["segments"], c["merged"]) == (19, 7) and c["merged"] >= 5
    assert len(off.cylinders) == 0
    assert int((on.seed_outcome == 2).sum()) >= 1 and len(on.cylinders) >= 1, "merges and the cylinder branch share the frame"
    assert [k.score_passed for k in on.cyl_candidates] == [True] and 112 <= on.cyl_candidates[0].n <= 128


@pytest.mark.parametrize("cyl", CYL)
def test_masked_ring(oracle_mod, cyl):
    """Two merged pairs of the 6 x 4 lattice lose the centre pixels of their ring cells: the pair left with two boundary points is
    dropped, the pair left with three is output with exactly three; every cell stays planar, so the segments are the lattice's."""
    r, c = _classified(oracle_mod, "masked_ring", cyl)
    whole, c_whole = _classified(oracle_mod, "lattice_6x4", cyl)
    assert np.array_equal(r.planar, whole.planar), "a cell lost its plane to the hole on its centre pixel"
    assert (c["segments"], c["merged"]) == (c_whole["segments"], c_whole["merged"]) == (23, 11)
    assert c["dropped_roots"] == 1 and len(r.planes) == len(whole.planes) - 1
    labels = r.plane_labels.reshape(24, 32)
    roots = [int(r.merge_labels[labels[rect[0], rect[2]] - 1]) for rect, _ in M.MASKED_RING]
    out = r.planes[:, 19].astype(int).tolist()
    assert roots[0] not in out and roots[1] in out
    assert all((r.merge_labels == root).sum() == 2 for root in roots), "both are merged pairs"
    assert len(r.boundary[out.index(roots[1])]) == 3
    assert sum(1 for k in out if (r.merge_labels == k).sum() == 2) >= 2, "other merged groups still output"


@pytest.mark.parametrize("name", ["lattice_12x8", "lattice_12x8_lean"])
def test_output_planes_of_the_92_segment_frames_are_kept_planes(oracle_mod, name):
    """The polygon of every output plane is valid with at least three vertices (the oracle of the reference's polygon class on the
    oracle's boundary points), so the planes Primitive_Detection keeps are exactly the output roots; one of them, a root of the
    first record, has a member beyond segment 63."""
    import polygon_oracle_py as P

    P.build()
    r = M.oracle(name, False)
    for k in range(len(r.planes)):
        normal, d = r.planes[k][0:3], r.planes[k][3]
        pol = P.Polygon.from_points(r.boundary[k], normal, normal * (-d))  # (Plane_Segment::get_center(): normal * (-d))
        assert not pol.threw and pol.valid and pol.is_valid() and len(pol.ring) >= 3 and pol.area > 0.0, f"plane {k}"
    ml = r.merge_labels.astype(int)
    assert any(k < 64 and (ml[64:] == k).any() for k in r.planes[:, 19].astype(int))


def test_cases_are_cached_and_read_only(oracle_mod):
    a, b = M.case("pair"), M.case("pair")
    assert a[0] is b[0] and not a[0].flags.writeable and M.oracle("pair", False) is M.oracle("pair", False)
    assert a[1] == M.intrinsics(640)

"""cape_host_map_union_cut and cape_host_polygon_union_cut -- the host twins of cape_map_union_cut and cape_debug_polygon_union_cut:
the polygon step of cape_host_map_update where the detection covers a part of a hole of the map plane -- against
cape_host_map_update itself and against the twins of the holes mode, on the table of tests/map_union_cut_cases.py, on the tables of
the holes mode and on the star sets with a hole.  CPU only."""
import numpy as np
import pytest

from map_union_cut_cases import CUT_HOLES, IN_THE_UPDATES_FRAME, PIECES
from map_union_hole_cases import CAPACITY, TABLES, holed_star_pairs
from test_map_union_holes_host import _update_polygon
from test_map_union_host import L, _bits, _measurement_rows, _one_plane_map, _world, ca, rect  # noqa: F401
from test_map_update_host import CTR, D, N, POSE, X, Y, _det


def _same(mine, theirs):
    """two results (row, ring row, polygon) are the same bytes and the same vertices"""
    if mine[0].tobytes() != theirs[0].tobytes() or mine[1].tobytes() != theirs[1].tobytes() or (mine[2] is None) != (theirs[2] is None):
        return False
    return mine[2] is None or (len(mine[2]) == len(theirs[2]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(mine[2], theirs[2])))


def _pair_against_the_update(ca, L, rings_a, b, d=1010.0):  # noqa: F811
    """[outer, hole, ...] as the map plane, ring b as the detection at distance d, through the update, the cut twin and the holes twin.
    A served polygon -- every ring, the frame, the area -- must be the update's new polygon bit for bit; the cut twin is HOST_CAPACITY
    exactly where the update reports OVERFLOW or a stated device rule applies, and never HOST_HOLE_CUT; where the holes twin does not
    flag HOST_HOLE_CUT, the cut twin's rows are its rows.  Returns (row, ring row, polygon, overflow, the holes twin's flags)."""
    arrays, tracks = _one_plane_map(ca, L, rings_a[0], rings_a[1:])
    det = [_det(b, d=d)]
    (P, R, V), Tr, _, _ = ca.host_map_update(arrays, tracks, [0], det, np.eye(4), POSE)
    assert Tr[0]["result"] & ca.MAP_RESULT_UPDATED
    mrows = _measurement_rows(ca, L, det)
    _, frows, _ = ca.host_map_kalman(arrays, tracks, [0], mrows)
    rows, ring_rows, polys = ca.host_map_union_cut(arrays, [0], frows, mrows, [_world(b)])
    hrows, hring_rows, hpolys = ca.host_map_union_holes(arrays, [0], frows, mrows, [_world(b)])
    row, rr, poly = rows[0], ring_rows[0], polys[0]
    if hrows[0]["flags"] != ca.UNION_HOST_HOLE_CUT:
        assert _same((row, rr, poly), (hrows[0], hring_rows[0], hpolys[0])) and not row["flags"] & ca.UNION_HOLE_PIECES
    else:
        assert row["flags"] == ca.UNION_HOST_CAPACITY or row["flags"] & (ca.UNION_SERVED | ca.UNION_HOLE_PIECES) == ca.UNION_SERVED | ca.UNION_HOLE_PIECES
    want = _update_polygon(P, R, V)
    overflow = bool(Tr[0]["result"] & ca.MAP_RESULT_OVERFLOW)
    assert row["map_plane"] == 0 and row["n_nodes"] == 0 and rr["pad"] == 0
    assert not row["flags"] & (ca.UNION_HOST_MAP_HOLES | ca.UNION_HOST_NEW_HOLE | ca.UNION_HOST_AMBIGUOUS | ca.UNION_HOST_HOLE_CUT)
    if row["flags"] & ca.UNION_SERVED:
        assert not overflow
        assert rr["ring_count"] == len(want) == len(poly) and bool(row["flags"] & ca.UNION_HOLES) == (len(want) > 1)
        assert rr["vertex_count"][: len(want)].tolist() == [len(r) for r in want] and not rr["vertex_count"][len(want):].any()
        assert row["vertex_count"] == len(want[0]) and row["vertex_offset"] == 0
        for k, (mine, theirs) in enumerate(zip(poly, want)):
            assert np.array_equal(_bits(mine), _bits(theirs)), f"ring {k}"
        for k in ("x_axis", "y_axis", "center"):
            assert np.array_equal(_bits(row[k]), _bits(P[0][k])), k
        area = sum((1 if k == 0 else -1) * 0.5 * abs(np.dot(r[:, 0], np.roll(r[:, 1], -1)) - np.dot(r[:, 1], np.roll(r[:, 0], -1)))
                   for k, r in enumerate(want))
        assert abs(row["area"] - area) <= 1e-9 * row["area"]
    else:
        assert poly is None and row["vertex_count"] == 0 and row["area"] == 0 and not row["x_axis"].any() and not rr.tobytes().strip(b"\0")
        assert row["flags"] == ca.UNION_HOST_CAPACITY
        if overflow:  # the update kept the old polygon
            assert [len(r) for r in want] == [len(r) for r in rings_a]
    return row, rr, poly, overflow, int(hrows[0]["flags"])


@pytest.mark.parametrize("case", CUT_HOLES, ids=[c[0] for c in CUT_HOLES])
@pytest.mark.parametrize("d", [D, 1010.0], ids=["same plane", "fused plane"])
def test_table_pairs_equal_the_update(ca, L, case, d):  # noqa: F811
    """the outcomes in the update's frame: the canonical frame's, but for the two rows whose piece order or first vertex the frame moves"""
    name, rings_a, b, outcome = case
    row, rr, poly, overflow, holes_flags = _pair_against_the_update(ca, L, rings_a, b, d=d)
    if outcome == CAPACITY:
        assert row["flags"] == ca.UNION_HOST_CAPACITY
        # the update's own overflow, or the rule of the device that the twins know: interior rings beyond 512 vertices before simplify
        assert overflow != (name == "four holes cut in two: 520 interior vertices"), name
    else:
        assert row["flags"] & ca.UNION_SERVED and [len(r) for r in poly] == IN_THE_UPDATES_FRAME.get(name, outcome), name
    assert bool(row["flags"] & ca.UNION_HOLE_PIECES) == (name in PIECES), name
    assert (holes_flags == ca.UNION_HOST_HOLE_CUT) == (name in PIECES or outcome == CAPACITY), name


def test_table_outcomes_in_the_canonical_frame(ca):  # noqa: F811
    for name, rings_a, b, outcome in CUT_HOLES:
        row, rr, poly = ca.host_polygon_union_cut(rings_a, b)
        hrow, hrr, hpoly = ca.host_polygon_union(rings_a, b)
        assert (hrow["flags"] == ca.UNION_HOST_HOLE_CUT) == (name in PIECES or outcome == CAPACITY), name
        if hrow["flags"] != ca.UNION_HOST_HOLE_CUT:
            assert _same((row, rr, poly), (hrow, hrr, hpoly)), name
        if outcome == CAPACITY:
            assert row["flags"] == ca.UNION_HOST_CAPACITY and poly is None and not rr.tobytes().strip(b"\0"), name
        else:
            assert row["flags"] & ca.UNION_SERVED and [len(r) for r in poly] == outcome == rr["vertex_count"][: rr["ring_count"]].tolist(), name
        assert bool(row["flags"] & ca.UNION_HOLE_PIECES) == (name in PIECES), name


def test_the_hole_counts_and_the_order_of_the_rings(ca):  # noqa: F811
    """holes_covered counts the wholly covered holes only; a cut hole counts in none of the three; the new holes stand first, then per
    hole of the map plane, in its order, the kept hole or its pieces"""
    want = {"an L-shaped piece": (0, 0, 0), "a fork: a new hole, then three pieces": (1, 0, 0), "kept, cut and covered": (0, 1, 1),
            "new, kept and a piece": (1, 1, 0), "exactly eight interior rings": (0, 6, 0), "a sliver piece falls to drop_collinear": (0, 0, 0),
            "kept: the edge runs along the hole's side": (0, 1, 0), "covered: the corner on the hole's corner": (0, 0, 1)}
    polys = {}
    for name, rings_a, b, _ in CUT_HOLES:
        if name in want:
            row, rr, polys[name] = ca.host_polygon_union_cut(rings_a, b)
            assert (rr["holes_new"], rr["holes_kept"], rr["holes_covered"]) == want[name], name
    assert len(polys) == len(want)
    fork = polys["a fork: a new hole, then three pieces"]
    assert fork[1][:, 1].min() == 1000 and all(p[:, 1].max() == 500 for p in fork[2:])  # the face above the map, then the hole's pieces
    mixed = polys["kept, cut and covered"]
    assert mixed[1][:, 0].max() == 200 and len(mixed[2]) == 6  # the kept hole stands before the piece of the hole behind it
    three = polys["new, kept and a piece"]
    assert three[1][:, 0].min() == 1000 and three[2][:, 0].max() == 200 and three[3][:, 0].max() == 2500
    eight = polys["exactly eight interior rings"]
    assert [p[:, 1].max() for p in eight[1:]] == [150.0] * 6 + [500.0] * 2


def test_pairs_without_a_cut_hole_keep_the_rows_of_the_holes_twins(ca, L):  # noqa: F811
    """the tables of the holes mode: its one partly covered pair is served with its L-shaped piece, every other row is the same"""
    cut = 0
    for name, rings_a, b, outcome in TABLES:
        mine, theirs = ca.host_polygon_union_cut(rings_a, b), ca.host_polygon_union(rings_a, b)
        if theirs[0]["flags"] == ca.UNION_HOST_HOLE_CUT:
            assert mine[0]["flags"] == ca.UNION_SERVED | ca.UNION_HOLES | ca.UNION_HOLE_PIECES and [len(r) for r in mine[2]] == [8, 6], name
            cut += 1
        else:
            assert _same(mine, theirs), name
    assert cut == 1


@pytest.mark.parametrize("n", [8, 24])
def test_star_sets_with_a_hole_equal_the_update(ca, L, n):  # noqa: F811
    """200 pairs each; the partly covered ones (11 of the 8-vertex set, 17 of the 24-vertex one) are all served with HOLE_PIECES"""
    pieces = capacity = 0
    for rings_a, b in holed_star_pairs(n):
        row, rr, poly, _, holes_flags = _pair_against_the_update(ca, L, rings_a, b)
        assert (holes_flags == ca.UNION_HOST_HOLE_CUT) == (bool(row["flags"] & ca.UNION_HOLE_PIECES) or row["flags"] == ca.UNION_HOST_CAPACITY)
        pieces += bool(row["flags"] & ca.UNION_HOLE_PIECES)
        capacity += row["flags"] == ca.UNION_HOST_CAPACITY
    print(f"\n{n}-vertex stars with a hole: {pieces} served with pieces, {capacity} capacity, of 200")
    assert (pieces, capacity) == {8: (11, 0), 24: (17, 0)}[n]


def test_argument_checks(ca):  # noqa: F811
    import ctypes as C

    Lh = ca._host_library()
    row, rr = np.zeros(128, ca.PLANE_UNION_DTYPE), np.zeros(128, ca.PLANE_UNION_RINGS_DTYPE)
    ver = np.zeros((ca.MAP_UNION_FRAME_VERTICES, 2))
    sq = rect(0, 1, 0, 1)
    src, view = ca._map_arrays(ca.pack_map([(N, D, X, Y, CTR, sq, [])]))
    ok = (C.byref(view), None, None, None, None, 0, row.ctypes.data, rr.ctypes.data, ver.ctypes.data)
    assert Lh.cape_host_map_union_cut(*ok) == 0
    for k in (0, 6, 7, 8):
        assert Lh.cape_host_map_union_cut(*(ok[:k] + (None,) + ok[k + 1:])) == -1
    assert Lh.cape_host_map_union_cut(*(ok[:5] + (129,) + ok[6:])) == -1
    counts = np.array([4], np.int32)
    ok = (sq.ctypes.data, counts.ctypes.data, 1, sq.ctypes.data, 4, None, row.ctypes.data, rr.ctypes.data, ver.ctypes.data)
    assert Lh.cape_host_polygon_union_cut(*ok) == 0
    for k in (0, 1, 3, 6, 7, 8):
        assert Lh.cape_host_polygon_union_cut(*(ok[:k] + (None,) + ok[k + 1:])) == -1
    for n_rings in (0, 10):
        assert Lh.cape_host_polygon_union_cut(*(ok[:2] + (n_rings,) + ok[3:])) == -1
    for n_b in (2, 4097):
        assert Lh.cape_host_polygon_union_cut(*(ok[:4] + (n_b,) + ok[5:])) == -1
    for bad in (2, 4097):
        assert Lh.cape_host_polygon_union_cut(*(ok[:1] + (np.array([bad], np.int32).ctypes.data,) + ok[2:])) == -1

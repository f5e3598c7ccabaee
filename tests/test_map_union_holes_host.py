"""cape_host_map_union_holes and cape_host_polygon_union -- the host twins of cape_map_union_holes and cape_debug_polygon_union: the
polygon step of cape_host_map_update for a map plane that has interior rings and / or a union that creates some -- against
cape_host_map_update itself on the tables of tests/map_union_hole_cases.py and on the star sets with a hole.  CPU only."""
import numpy as np
import pytest

from map_union_hole_cases import CAPACITY, HOLE_CUT, HOLED_MAPS, IN_THE_UPDATES_FRAME, TABLES, holed_star_pairs
from test_map_union_host import (ALL_PAIRS, L, _bits, _measurement_rows, _one_plane_map, _world, ca, classify, rect,  # noqa: F401
                                 star_pairs)
from test_map_update_host import CTR, D, N, PCC, POSE, X, Y, _c, _det, _p


def _update_polygon(P, R, V, j=0):
    """[outer, hole, ...] of map plane j of a packed map"""
    out = []
    for k in range(int(P[j]["ring_count"])):
        r = R[P[j]["ring_first"] + k]
        out.append(V[r["vertex_offset"]: r["vertex_offset"] + r["vertex_count"]])
    return out


def _pair_against_the_update(ca, L, rings_a, b, d=1010.0):  # noqa: F811
    """[outer, hole, ...] as the map plane, ring b as the detection at distance d, through the update and through the twin.  A served
    polygon -- every ring, the frame, the area -- must be the update's new polygon bit for bit; the twin is HOST_CAPACITY exactly
    where the update reports OVERFLOW or a stated device rule applies.  Returns (row, ring row, polygon)."""
    arrays, tracks = _one_plane_map(ca, L, rings_a[0], rings_a[1:])
    det = [_det(b, d=d)]
    (P, R, V), Tr, _, _ = ca.host_map_update(arrays, tracks, [0], det, np.eye(4), POSE)
    assert Tr[0]["result"] & ca.MAP_RESULT_UPDATED
    mrows = _measurement_rows(ca, L, det)
    _, frows, _ = ca.host_map_kalman(arrays, tracks, [0], mrows)
    rows, ring_rows, polys = ca.host_map_union_holes(arrays, [0], frows, mrows, [_world(b)])
    row, rr, poly = rows[0], ring_rows[0], polys[0]
    want = _update_polygon(P, R, V)
    overflow = bool(Tr[0]["result"] & ca.MAP_RESULT_OVERFLOW)
    assert row["map_plane"] == 0 and row["n_nodes"] == 0
    assert not row["flags"] & (ca.UNION_HOST_MAP_HOLES | ca.UNION_HOST_NEW_HOLE | ca.UNION_HOST_AMBIGUOUS)
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
        if not row["flags"] & (ca.UNION_DISJOINT | ca.UNION_UNCHANGED):
            assert rr["holes_new"] + rr["holes_kept"] == len(want) - 1
    else:
        assert poly is None and row["vertex_count"] == 0 and row["area"] == 0 and not row["x_axis"].any() and not rr.tobytes().strip(b"\0")
        assert row["flags"] in (ca.UNION_HOST_CAPACITY, ca.UNION_HOST_HOLE_CUT)
        if overflow:  # the update kept the old polygon
            assert row["flags"] == ca.UNION_HOST_CAPACITY
            assert [len(r) for r in want] == [len(r) for r in rings_a]
    return row, rr, poly, overflow


@pytest.mark.parametrize("case", TABLES, ids=[c[0] for c in TABLES])
@pytest.mark.parametrize("d", [D, 1010.0], ids=["same plane", "fused plane"])
def test_table_pairs_equal_the_update(ca, L, case, d):  # noqa: F811
    name, rings_a, b, outcome = case
    row, rr, poly, overflow = _pair_against_the_update(ca, L, rings_a, b, d=d)
    if outcome == CAPACITY:
        assert row["flags"] == ca.UNION_HOST_CAPACITY
        # the update's own overflow, or a rule of the device: a ring of the map plane beyond 128 vertices, interior rings beyond 512
        device_rule = max(len(r) for r in rings_a) > ca.MAP_UNION_MAX_RING or sum(len(r) for r in rings_a[1:]) > ca.MAP_UNION_HOLE_VERTICES
        assert overflow != device_rule, name
    elif outcome == HOLE_CUT:
        assert row["flags"] == ca.UNION_HOST_HOLE_CUT
    else:
        assert row["flags"] & ca.UNION_SERVED and [len(r) for r in poly] == IN_THE_UPDATES_FRAME.get(name, outcome), name


def test_table_outcomes_in_the_canonical_frame(ca):  # noqa: F811
    for name, rings_a, b, outcome in TABLES:
        row, rr, poly = ca.host_polygon_union(rings_a, b)
        if outcome in (CAPACITY, HOLE_CUT):
            assert row["flags"] == (ca.UNION_HOST_CAPACITY if outcome == CAPACITY else ca.UNION_HOST_HOLE_CUT) and poly is None, name
        else:
            assert row["flags"] & ca.UNION_SERVED and [len(r) for r in poly] == outcome == rr["vertex_count"][: rr["ring_count"]].tolist(), name


def test_the_hole_counts_of_the_rings_row(ca):  # noqa: F811
    want = {"C shape and bar": (1, 0, 0), "comb of 9 and bar": (8, 0, 0), "a hole clear of the detection": (0, 1, 0), "a covered hole": (0, 0, 1),
            "eight holes": (0, 8, 0), "a new hole before a kept one": (1, 1, 0), "disjoint, the holed map bigger": (0, 1, 0),
            "disjoint, the holed map bigger, the rule fires": (0, 0, 0),
            "the outer face is the detection's": (0, 1, 0), "a hole covered by exactly tiny": (0, 1, 0)}
    seen = 0
    for name, rings_a, b, _ in TABLES:
        if name in want:
            row, rr, poly = ca.host_polygon_union(rings_a, b)
            assert (rr["holes_new"], rr["holes_kept"], rr["holes_covered"]) == want[name], name
            seen += 1
    assert seen == len(want)
    # the new holes stand before the kept one, in the host's order
    _, _, poly = ca.host_polygon_union(*[c for c in HOLED_MAPS if c[0] == "a new hole before a kept one"][0][1:3])
    assert poly[1][:, 0].min() == 1000 and poly[2][:, 0].min() == 100


@pytest.mark.parametrize("n", [8, 24])
def test_star_sets_with_a_hole_equal_the_update(ca, L, n):  # noqa: F811
    kept = covered = cut = 0
    for rings_a, b in holed_star_pairs(n):
        row, rr, _, _ = _pair_against_the_update(ca, L, rings_a, b)
        assert not row["flags"] & ca.UNION_HOST_CAPACITY
        cut += bool(row["flags"] & ca.UNION_HOST_HOLE_CUT)
        kept += bool(row["flags"] & ca.UNION_SERVED and rr["holes_kept"])
        covered += bool(row["flags"] & ca.UNION_SERVED and rr["holes_covered"])
    print(f"\n{n}-vertex stars with a hole: {kept} kept, {covered} covered, {cut} partly covered of 200")
    assert cut <= 20 and kept >= 20 and covered >= 20


@pytest.mark.parametrize("n", [8, 24])
def test_plain_star_sets_are_served_with_their_new_holes(ca, L, n):  # noqa: F811
    holes = 0
    for a, b in star_pairs(n):
        row, rr, poly, _ = _pair_against_the_update(ca, L, [a], b)
        assert row["flags"] & ca.UNION_SERVED
        holes += bool(row["flags"] & ca.UNION_HOLES)
        plain, _ = ca.host_ring_union(a, b)
        assert bool(plain["flags"] & ca.UNION_HOST_NEW_HOLE) == bool(rr["holes_new"])
    print(f"\n{n}-vertex stars: {holes} of 200 pairs are served with a hole")
    assert holes == {8: 1, 24: 9}[n]


def test_the_frames_slab_fills_up_in_kept_plane_order_with_holed_polygons(ca, L):  # noqa: F811
    """16 pairs whose polygons keep 4 + 96 + 48 vertices each (cog holes, most of whose teeth simplify's tolerance of 10 leaves
    standing) do not fit 2 048: the first thirteen are served back to back, rings and all, the rest are HOST_CAPACITY -- a polygon
    goes in whole or not at all."""
    from test_map_union_host import cog

    n_pairs = 16
    outer = rect(0, 400, 0, 400)
    holes = [cog(128, 50.0, 30.0) + [100.0, 200.0], cog(64, 50.0, 30.0) + [250.0, 200.0]]
    shift = lambda j: np.array([1000.0 * j, 0.0])  # noqa: E731
    planes = [(N, D, X, Y, CTR, outer + shift(j), [h + shift(j) for h in holes]) for j in range(n_pairs)]
    arrays = ca.pack_map(planes)
    cov = np.zeros(16)
    assert L.cape_host_plane_covariance(_p(N), D, _p(_c(PCC)), _p(cov)) == 1
    tracks = np.zeros(n_pairs, ca.MAP_TRACK_DTYPE)
    tracks["covariance"] = cov.reshape(4, 4)
    det = [_det(rect(350, 390, 10, 390) + shift(j)) for j in range(n_pairs)]
    mrows = _measurement_rows(ca, L, det)
    match = list(range(n_pairs))
    _, frows, _ = ca.host_map_kalman(arrays, tracks, match, mrows)
    rows, ring_rows, polys = ca.host_map_union_holes(arrays, match, frows, mrows, [_world(d[5]) for d in det])
    served = [bool(r["flags"] & ca.UNION_SERVED) for r in rows]
    assert served[0] and not served[-1] and served == sorted(served, reverse=True)
    used = 0
    for r, q, poly in zip(rows, ring_rows, polys):
        if r["flags"] & ca.UNION_SERVED:
            assert r["vertex_offset"] == used and [len(x) for x in poly] == q["vertex_count"][: q["ring_count"]].tolist()
            used += int(q["vertex_count"].sum())
        else:
            assert r["flags"] == ca.UNION_HOST_CAPACITY and poly is None and not q["ring_count"]
    assert used <= ca.MAP_UNION_FRAME_VERTICES
    first_refused = served.index(False)
    (P, R, V), _, _, _ = ca.host_map_update(arrays, tracks, match, det, np.eye(4), POSE)
    assert sum(len(r) for r in _update_polygon(P, R, V, first_refused)) > ca.MAP_UNION_FRAME_VERTICES - used
    # the outer ring alone would still have fitted
    assert len(_update_polygon(P, R, V, first_refused)[0]) <= ca.MAP_UNION_FRAME_VERTICES - used


def test_the_plain_twins_keep_their_rows(ca, L):  # noqa: F811
    """cape_host_ring_union's and cape_host_map_union's rows on ALL_PAIRS are the table's, as before the holes mode.  The second runs on
    a one-plane map per pair through the checks of tests/test_map_union_host.py (a served ring and its frame are the update's bit for
    bit, a union with a hole is HOST_NEW_HOLE and nothing else); where a plain twin serves a pair, the holes twin gives the same row,
    byte for byte, and the same ring."""
    from test_map_union_host import _pair_against_the_update as plain_pair

    for name, a, b, cls, count in ALL_PAIRS:
        row, ring = ca.host_ring_union(a, b)
        assert classify(ca, int(row["flags"])) == cls, name
        if count is not None:
            assert len(ring) == count == row["vertex_count"], name
        hrow, hrr, poly = ca.host_polygon_union([a], b)
        if row["flags"] & ca.UNION_SERVED:
            assert hrow.tobytes() == row.tobytes() and hrr["ring_count"] == 1 and np.array_equal(_bits(poly[0]), _bits(ring)), name
        mrow, mring, _, _ = plain_pair(ca, L, a, b)
        assert classify(ca, int(mrow["flags"])) == cls, name
        hmrow, hmrr, hmpoly, _ = _pair_against_the_update(ca, L, [a], b)
        if mrow["flags"] & ca.UNION_SERVED:
            assert hmrow.tobytes() == mrow.tobytes() and hmrr["ring_count"] == 1 and np.array_equal(_bits(hmpoly[0]), _bits(mring)), name
        elif cls == "new_hole":
            assert mrow["flags"] == ca.UNION_HOST_NEW_HOLE and mring is None, name
        else:
            assert mrow["flags"] == ca.UNION_HOST_CAPACITY and mring is None, name


def test_argument_checks(ca):  # noqa: F811
    import ctypes as C

    Lh = ca._host_library()
    row, rr = np.zeros(128, ca.PLANE_UNION_DTYPE), np.zeros(128, ca.PLANE_UNION_RINGS_DTYPE)
    ver = np.zeros((ca.MAP_UNION_FRAME_VERTICES, 2))
    sq = rect(0, 1, 0, 1)
    src, view = ca._map_arrays(ca.pack_map([(N, D, X, Y, CTR, sq, [])]))
    ok = (C.byref(view), None, None, None, None, 0, row.ctypes.data, rr.ctypes.data, ver.ctypes.data)
    assert Lh.cape_host_map_union_holes(*ok) == 0
    for k in (0, 6, 7, 8):
        assert Lh.cape_host_map_union_holes(*(ok[:k] + (None,) + ok[k + 1:])) == -1
    assert Lh.cape_host_map_union_holes(*(ok[:5] + (129,) + ok[6:])) == -1
    counts = np.array([4], np.int32)
    ok = (sq.ctypes.data, counts.ctypes.data, 1, sq.ctypes.data, 4, None, row.ctypes.data, rr.ctypes.data, ver.ctypes.data)
    assert Lh.cape_host_polygon_union(*ok) == 0
    for k in (0, 1, 3, 6, 7, 8):
        assert Lh.cape_host_polygon_union(*(ok[:k] + (None,) + ok[k + 1:])) == -1
    for n_rings in (0, 10):
        assert Lh.cape_host_polygon_union(*(ok[:2] + (n_rings,) + ok[3:])) == -1
    for n_b in (2, 4097):
        assert Lh.cape_host_polygon_union(*(ok[:4] + (n_b,) + ok[5:])) == -1
    for bad in (2, 4097):
        assert Lh.cape_host_polygon_union(*(ok[:1] + (np.array([bad], np.int32).ctypes.data,) + ok[2:])) == -1

"""The ring-pair table of tests/ring_pair_cases.py without a GPU: its exact reference against closed forms, the cells the table must
fill, the host class (cape_host_match_map) against the exact reference on every case, and the hand-made shard of tests/packing.py
through cape_host_shard_frame.  Run with -s for the table of cells and the host class's worst error."""
from fractions import Fraction

import numpy as np
import pytest

import ring_pair_cases as R
from packing import clockwise, make_shard, ring_area

AREA_RTOL = 1e-9  # tests/test_gpu_polygon_oracle.py


def _pair(det, outer, holes=()):
    return dict(name="closed form", det=det, outer=outer, holes=list(holes))


def test_exact_reference_against_closed_forms():
    # rectangle n rectangle
    assert R._ring_pair(R.rect(0, 0, 10, 7), R.rect(4, -3, 25, 5))["area"] == 6 * 5
    assert R._ring_pair(R.rect(0, 0, 10, 7), R.rect(10, 0, 25, 5))["area"] == 0
    # a slanted pair with a crossing off the integer grid: the triangles (0,0) (3,0) (0,3) and (0,0) (3,0) (3,2) meet in (0,0) (3,0) (9/5, 6/5)
    assert R._ring_pair([(0, 0), (0, 3), (3, 0)], [(0, 0), (3, 2), (3, 0)])["area"] == Fraction(3 * 6, 2 * 5)
    # comb n rectangle: the sum of the teeth's overlaps.  Tooth k is the triangle P_k Q_k P_k+1; its width at x is linear in x
    T, L, H = 5, 4000, 200
    comb, x0, x1 = R.comb_right(T, L, H, skew=3), 1000, 3000
    teeth = Fraction(0)
    for k in range(T):
        p, q, r = (-1 if k == 0 else 0, k * H), (L + 3 * k, k * H + H // 2), (-1 if k == T - 1 else 0, (k + 1) * H)
        width = lambda x: (r[1] + Fraction((q[1] - r[1]) * (x - r[0]), q[0] - r[0])) - (p[1] + Fraction((q[1] - p[1]) * (x - p[0]), q[0] - p[0]))
        teeth += (width(x0) + width(x1)) / 2 * (x1 - x0)
    got = R._ring_pair(comb, R.rect(x0, -50, x1, T * H + 50))
    assert got["area"] == teeth and got["stack"] == 2 * T and got["terms"] == T
    assert R._ring_pair(R.rect(x0, -50, x1, T * H + 50), comb)["area"] == teeth
    # a ring with itself, and with itself the other way round
    for ring in (R.regular(17, 1000, 5, -7), R.comb_up(4, 100, 300), R.mountain(9, 10, 0, 0, 50, 10, 5)):
        own = Fraction(abs(R.signed_area2(ring)), 2)
        assert R._ring_pair(ring, ring)["area"] == own and R._ring_pair(ring, ring[::-1])["area"] == own
    # a holed square: detection over all of it, over half the hole, beside the hole; the crossing count of two combs at right angles
    square, hole = R.rect(0, 0, 100, 100), R.rect(40, 40, 60, 60)
    assert R.exact_inter_area(_pair(R.rect(-5, -5, 105, 105), square, [hole])) == 100 * 100 - 20 * 20
    assert R.exact_inter_area(_pair(R.rect(50, 0, 100, 100), square, [hole])) == 50 * 100 - 10 * 20
    assert R.exact_inter_area(_pair(R.rect(0, 0, 30, 100), square, [hole])) == 30 * 100
    assert R.exact_inter_area(_pair(R.rect(45, 45, 55, 55), square, [hole])) == 0
    d = R.demand(_pair(R.comb_right(3, 9000, 600, -500, 300), R.comb_up(4, 2000, 3000)))
    assert (d["ring"], d["boundaries"], d["stack"]) == (9, 7 + 9 + 6 * 8, 6)


def test_expected_walk_restates_the_capacity_table():
    walk = lambda ring, boundaries, stack: R.expected_walk(dict(ring=ring, pairs=[(boundaries, stack)]))
    assert walk(32, 256, 6) == ([0], 0, None) and walk(33, 10, 2) == ([0, 1], 1, None) and walk(10, 257, 2) == ([0, 1], 1, None)
    assert walk(10, 20, 8) == ([0, 1], 1, None) and walk(10, 20, 18) == ([0, 1, 2], 2, None) and walk(129, 20, 2) == ([0, 1, 2, 3], 3, None)
    assert walk(10, 1025, 2) == ([0, 1, 2, 3], 3, None) and walk(10, 2049, 2) == ([0, 1, 2, 3], None, "slabs")
    assert walk(513, 20, 2) == ([0, 1, 2, 3], None, "ring") and walk(10, 20, 34) == ([0, 1, 2], None, "stack")
    assert walk(200, 20, 34) == ([0, 1, 2, 3], None, "stack")  # (its rings take it to tier 3, which is as small in that resource)
    # a hole is taken after the outer ring: the first ring beyond a capacity names the resource
    assert R.expected_walk(dict(ring=10, pairs=[(20, 2), (20, 34)])) == ([0, 1, 2], None, "stack")
    assert R.expected_walk(dict(ring=10, pairs=[(20, 34), (2049, 2)])) == ([0, 1, 2], None, "stack")


def test_every_required_cell_is_filled():
    """what keeps the GPU test from passing on an empty cell: demand and expected_walk place a case in every required cell"""
    for cell in R.REQUIRED_CELLS:
        names = R.CELLS.get(cell, [])
        assert names, cell
        for name in names:
            case = R.BY_NAME[name]
            R.check_cell(cell, case)
            d = R.demand(case)
            visited, served, why = R.expected_walk(d)
            print(f"{cell:32s} {name:32s} ring {d['ring']:4d}  boundaries {d['boundaries']:5d}  stack {d['stack']:3d}  tiers {visited} -> "
                  f"{'tier %d' % served if served is not None else 'none (' + why + ')'}")
    assert len({c["name"] for c in R.CASES}) == len(R.CASES) <= 120
    # the cases no tier holds are of the three kinds, and at most four cases reach 2048 boundaries
    assert {R.expected_walk(R.demand(c))[2] for c in R.CASES} == {None, "ring", "slabs", "stack"}
    assert sum(1 for c in R.CASES if R.demand(c)["boundaries"] >= 2048) <= 4


def test_host_class_against_the_exact_reference(host_binaries):
    import cape_amd

    worst, worst_name = 0.0, None
    for k, case in enumerate(R.CASES):
        det, plane = R.planes_of(case, R.depth_of(k))
        match, map_of, inter = cape_amd.host_match_map(cape_amd.pack_map([plane]), [(*det, None)], None, None, cape_amd.MATCH_ALLOW_INDEX0, areas=True)
        got, exact = float(inter[0, 0]), R.exact_inter_area(case)
        xs, ys = zip(*(p for ring in [case["det"], case["outer"], *case["holes"]] for p in ring))
        box = (max(xs) - min(xs)) * (max(ys) - min(ys))
        if case["zero"]:
            assert got == 0.0, case["name"]
        elif exact < Fraction(box, 10**6):
            assert abs(Fraction(got) - exact) <= Fraction(box, 10**9), case["name"]
        else:
            err = float(abs(Fraction(got) - exact) / exact)
            if err > worst:
                worst, worst_name = err, case["name"]
            assert err <= R.HOST_RTOL, (case["name"], err)
        # the decision of a lone pair: matched when the overlap reaches 40 % of the detection
        overlap = exact / Fraction(abs(R.signed_area2(case["det"])), 2)
        if abs(overlap - Fraction(2, 5)) > Fraction(1, 1000):
            assert (match[0] == 0) == (overlap >= Fraction(2, 5)) and map_of[0] == (0 if match[0] == 0 else -1), case["name"]
    print(f"host class against the exact reference over {len(R.CASES)} cases: worst relative error {worst:.3e} ({worst_name}); bound {R.HOST_RTOL:.3e}")
    assert R.HOST_RTOL <= AREA_RTOL, "a bound above the project's own AREA_RTOL is a finding to report, not a bound to adopt"


def test_hand_made_shard_returns_the_planes_put_in(host_binaries):
    import cape_amd
    from cape_amd.dist import Shard, packed_layout

    names = ["stack6_det", "hole_cut_flipped", "det33", "itself_flipped", "equal_heights", "seam65_t0", "det513"]
    frames = [[], [0, 1, 2], [3], [], [4, 5, 6]]  # ragged, with empty frames
    planes = [R.planes_of(R.BY_NAME[n], R.depth_of(k))[0] for k, n in enumerate(names)]
    layout = packed_layout(6, cells=0, planes_per_frame=2, cylinders_per_frame=0, polygons=True, vertices_per_frame=200)
    buf = make_shard([[planes[i] for i in f] for f in frames], layout, first_frame=11)
    shard = Shard(buf, layout)
    assert shard.first_frame == 11 and len(shard.frames) == len(frames) and int(shard.header["overflow"]) == 0
    assert int(shard.polygon_header["n_polygons_valid"]) == len(names) and int(shard.polygon_header["n_vertices_total"]) == sum(len(p[5]) for p in planes)
    for k, f in enumerate(frames):
        det, segs = cape_amd.host_shard_frame(buf, layout, k)
        assert len(det) == len(f) and list(segs) == list(range(len(f)))
        assert len(shard.kept_planes(k)) == len(f)
        for got, i in zip(det, f):
            normal, d, x_axis, y_axis, center, ring = planes[i]
            assert np.array_equal(got[0], normal) and got[1] == d and np.array_equal(got[2], x_axis) and np.array_equal(got[3], y_axis)
            assert np.array_equal(got[4], center) and np.array_equal(got[5], clockwise(ring)) and got[6] == ring_area(ring)[0]
            assert got[6] * 2 == abs(R.signed_area2(R.BY_NAME[names[i]]["det"])) and np.array_equal(got[7], np.eye(3))
    with pytest.raises(cape_amd.CapeError):
        cape_amd.host_shard_frame(buf, layout, len(frames))


def test_map_match_lists_is_exported_and_checks_its_arguments(hip_library):
    """cape_debug_map_match_lists, the accessor tests/test_gpu_ring_tiers.py reads the tier counts through (argument checks come before
    any device call: no GPU needed)"""
    import ctypes as C
    import cape_amd

    lib = cape_amd.load_library()
    assert "cape_debug_map_match_lists" in cape_amd.EXPORTED_SYMBOLS
    words = (C.c_uint32 * 8)(*[7] * 8)
    assert lib.cape_debug_map_match_lists(None, words) == -1 and list(words) == [7] * 8

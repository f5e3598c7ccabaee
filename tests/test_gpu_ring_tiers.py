"""The ring intersection at every capacity tier's edges: the table of tests/ring_pair_cases.py through cape_match_map_shards on a handle
that never extracted, one case per slot of a hand-made shard (tests/packing.make_shard), the map through cape_map_upload.  Areas and
decisions bit for bit against the host twin (which tests/test_ring_pair_cases.py holds to an exact reference), the pairs handed to
tiers 1..3 against expected_walk (cape_debug_map_match_lists), the overflow flag on exactly the pairs no tier holds, four tiers in one
frame, and ten cases under a pose that is not the identity.  A handful of launches over some ninety small pairs."""
import numpy as np
import pytest

import ring_pair_cases as R
from packing import make_shard
from test_gpu_map_match import _bits, _lift, _w2c
from test_gpu_match_map_shards import _assert_equals_host_route, _assert_same, _frames_view

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FF8000000000000  # nan_code(k) = NAN_BITS | k (cape_ring_area.h)


def _mixed_frame():
    """two detected planes facing four map planes at one depth, whose pairs end in tiers 0, 1, 2 and 3: (detections, map rings, the
    eight pairs as cases, indexed [j][i])"""
    dets = [R.rect(200, 100, 2200, 1900), R.rect(500, 50, 3500, 3150)]
    maps = [R.rect(0, 0, 2000, 2000), R.comb_right(8, 4000, 200, skew=3), R.comb_right(16, 4000, 200, skew=3), R.regular(200, 1500, 1500, 1500)]
    pairs = [[dict(name=f"mixed_{j}_{i}", det=d, outer=m, holes=[], zero=False) for i, d in enumerate(dets)] for j, m in enumerate(maps)]
    return dets, maps, pairs


class _Table:
    pass


@pytest.fixture(scope="module")
def table(hip_library):
    """Slot k holds case k's detection, map plane k its polygon, both at depth_of(k); the last slot is the mixed frame, its four map
    planes the last four.  One call over the whole table, kept with its counters."""
    import torch
    import cape_amd
    from cape_amd import Extractor, synth
    from cape_amd.dist import packed_layout

    T = _Table()
    T.cases = R.CASES
    n = len(T.cases)
    dets, maps, T.mixed = _mixed_frame()
    both = [R.planes_of(c, R.depth_of(k)) for k, c in enumerate(T.cases)]
    mixed_depth = R.depth_of(n + 1)
    T.frames = [[d] for d, _ in both] + [[R.planes_of(dict(det=d, outer=d, holes=[]), mixed_depth)[0] for d in dets]]
    T.planes = [m for _, m in both] + [R.planes_of(dict(det=m, outer=m, holes=[]), mixed_depth)[1] for m in maps]
    T.n_slots, T.mixed_slot, T.mixed_first = n + 1, n, n
    vertices = sum(len(p[5]) for f in T.frames for p in f)
    T.layout = packed_layout(T.n_slots, cells=0, planes_per_frame=2, cylinders_per_frame=0, polygons=True, vertices_per_frame=vertices // T.n_slots + 1)
    T.buf = make_shard(T.frames, T.layout)
    T.arrays = cape_amd.pack_map(T.planes)
    T.flags = cape_amd.MATCH_ALLOW_INDEX0  # (a slot's only detection has index 0)
    T.walks = [R.expected_walk(R.demand(c)) for c in T.cases]
    T.overflowing = [k for k, w in enumerate(T.walks) if w[1] is None]
    T.stream = torch.cuda.current_stream().cuda_stream
    T.owner = Extractor(640, 480, cylinders=False, max_batch=1, **synth.DEFAULT_INTRINSICS)  # never extracts
    T.owner.upload_map(T.arrays)
    assert T.owner.map_match_lists() == dict(reserved=0, tiers=[0, 0, 0], tickets=[0, 0, 0])  # no map-matcher call yet
    T.device = torch.from_numpy(T.buf).cuda()
    T.owner.match_map_shards(T.device.data_ptr(), 1, T.layout, None, None, T.flags | cape_amd.MATCH_MAP_AREAS, T.stream)
    T.result = T.owner.shard_map_matches(T.n_slots, areas=True)
    T.lists = T.owner.map_match_lists()
    yield T
    T.owner.close()


def _assert_overflowed(res, s, j, why):
    """the form of _assert_flagged: a slot with a pair no tier holds reports nothing -- and the pair's area names the resource"""
    import cape_amd

    frames, match, inter = res
    assert frames[s]["flags"] == cape_amd.MATCH_EXACT_OVERFLOW, (s, frames[s]["flags"])
    assert np.all(match[s] == -1) and np.all(frames[s]["map_of"] == -1) and frames[s]["n_matched"] == 0
    code = int(_bits(inter[s][j, :1])[0])
    assert code == NAN_BITS | R.NAN_CODE[why], (s, hex(code))
    rest = inter[s].copy()
    rest[j, 0] = -1.0
    assert np.all(rest == -1.0)


def test_areas_and_decisions_equal_the_host_twin(table):
    T = table
    frames, match, inter = T.result
    matched = 0
    for k, case in enumerate(T.cases):
        if k in T.overflowing:
            continue
        _assert_equals_host_route(T.result, k, T.buf, T.layout, k, T.arrays, None, None, T.flags)
        # the distance gate pairs case k with case k only: every other pair reads -1
        others = inter[k].copy()
        others[k, 0] = -1.0
        assert np.all(others == -1.0) and frames[k]["n_cur"] == 1 and frames[k]["flags"] == 0, case["name"]
        got, exact = float(inter[k][k, 0]), R.exact_inter_area(case)
        assert (got == 0.0) if exact == 0 else abs(got - float(exact)) <= R.HOST_RTOL * float(exact), case["name"]
        matched += int(match[k][k] == 0)
    assert 10 < matched < len(T.cases) - 10  # both decisions occur


def test_pairs_handed_to_each_tier(table):
    T = table
    pairs = list(T.cases) + [p for row in T.mixed for p in row]
    expected = R.tier_counts(pairs)
    print("reserved", T.lists["reserved"], "tiers 1..3", T.lists["tiers"], "expected", expected, "tickets", T.lists["tickets"])
    assert T.lists["reserved"] == len(pairs)
    assert T.lists["tiers"] == expected
    assert all(t >= c for t, c in zip(T.lists["tickets"], expected))  # (a wave draws one ticket past the list before it leaves)
    # in particular: the 34-edge pairs stop at tier 2
    for name in ("stack34_det", "stack34_map"):
        assert R.expected_walk(R.demand(R.BY_NAME[name]))[0] == [0, 1, 2]


def test_pairs_no_tier_holds_flag_their_slot_and_no_other(table):
    import torch
    import cape_amd

    T = table
    assert sorted({T.walks[k][2] for k in T.overflowing}) == ["ring", "slabs", "stack"] and len(T.overflowing) <= 6
    for k, walk in enumerate(T.walks):
        if walk[1] is None:
            _assert_overflowed(T.result, k, k, walk[2])
        else:
            assert T.result[0][k]["flags"] == 0, T.cases[k]["name"]
    assert T.result[0][T.mixed_slot]["flags"] == 0
    # the same call without those slots: every other slot is byte-equal
    without = T.buf.copy()
    _frames_view(without, T.layout)["n_planes"][T.overflowing] = 0
    dev = torch.from_numpy(without).cuda()
    T.owner.match_map_shards(dev.data_ptr(), 1, T.layout, None, None, T.flags | cape_amd.MATCH_MAP_AREAS, T.stream)
    got = T.owner.shard_map_matches(T.n_slots, areas=True)
    lists = T.owner.map_match_lists()
    others = np.array([s for s in range(T.n_slots) if s not in T.overflowing])
    _assert_same(got, T.result, others)
    assert np.array_equal(got[0][others].view(np.uint8), T.result[0][others].view(np.uint8))
    for k in T.overflowing:
        assert got[0][k]["flags"] == 0 and got[0][k]["n_cur"] == 0 and np.all(got[2][k] == -1.0)
    served = [c for k, c in enumerate(T.cases) if k not in T.overflowing] + [p for row in T.mixed for p in row]
    assert lists["reserved"] == len(served) and lists["tiers"] == R.tier_counts(served)


def test_four_tiers_in_one_frame(table):
    T = table
    assert [[R.expected_walk(R.demand(p))[1] for p in row] for row in T.mixed] == [[0, 0], [1, 1], [2, 2], [3, 3]]
    segs = _assert_equals_host_route(T.result, T.mixed_slot, T.buf, T.layout, T.mixed_slot, T.arrays, None, None, T.flags)
    assert segs == [0, 1]
    frames, match, inter = T.result
    # every area in its own (j, i) cell: the eight are all different, and each is the exact one of ITS pair
    block = inter[T.mixed_slot][T.mixed_first:, :2]
    assert len(set(block.reshape(-1).tolist())) == 8 and np.all(inter[T.mixed_slot][: T.mixed_first] == -1.0)
    for j, row in enumerate(T.mixed):
        for i, pair in enumerate(row):
            exact = float(R.exact_inter_area(pair))
            assert abs(block[j, i] - exact) <= R.HOST_RTOL * exact, pair["name"]
    assert frames[T.mixed_slot]["n_matched"] >= 2 and sorted(v for v in match[T.mixed_slot] if v >= 0) == [0, 1]


def test_ten_cases_under_a_pose(table):
    """the map lifted into a world frame by a rotation and a translation (as _lift does), the slots' pose bringing it back: areas and
    decisions against the host twin bit for bit (the exact reference does not apply: the coordinates are no integers any more)"""
    import torch
    import cape_amd
    from cape_amd.dist import packed_layout

    T = table
    names = ["det33", "map129", "stack6_det", "stack18_map", "t0_xs256", "xs1024", "seam65_t0", "seam129_t1", "hole_cut", "comb_in_comb_t1"]
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rm = np.eye(3) + np.sin(0.3) * K + (1 - np.cos(0.3)) * (K @ K)
    o = np.array([120.5, -340.25, 77.125])
    both = [R.planes_of(R.BY_NAME[name], R.depth_of(k)) for k, name in enumerate(names)]
    planes = [_lift(m, Rm, o, holes=m[6]) for _, m in both]
    frames = [[d] for d, _ in both]
    layout = packed_layout(len(names), cells=0, planes_per_frame=1, cylinders_per_frame=0, polygons=True, vertices_per_frame=200)
    buf = make_shard(frames, layout)
    arrays = cape_amd.pack_map(planes)
    pose = np.stack([_w2c(Rm, o)] * len(names))
    T.owner.upload_map(arrays)
    try:
        dev = torch.from_numpy(buf).cuda()
        T.owner.match_map_shards(dev.data_ptr(), 1, layout, pose, None, T.flags | cape_amd.MATCH_MAP_AREAS, T.stream)
        res = T.owner.shard_map_matches(len(names), areas=True)
        lists = T.owner.map_match_lists()
    finally:
        T.owner.upload_map(T.arrays)
    for k, name in enumerate(names):
        assert res[0][k]["flags"] == 0, name
        _assert_equals_host_route(res, k, buf, layout, k, arrays, pose[k], None, T.flags)
        exact = float(R.exact_inter_area(R.BY_NAME[name]))
        assert abs(res[2][k][k, 0] - exact) <= 1e-9 * exact, name  # (the suite's AREA_RTOL: a rigid motion keeps the area)
    assert lists["reserved"] == len(names)

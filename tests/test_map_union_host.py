"""cape_host_map_union and cape_host_ring_union -- the host twins of cape_map_union and cape_debug_ring_union: the polygon step of
cape_host_map_update (Polygon::project, merge_union, simplify on the host class) per matched pair -- against cape_host_map_update itself
on hand-built pairs placed on the plane z = 1000 and on two sets of random star outlines, fed the rows of cape_host_map_kalman.  CPU
only.  The pair generators are shared with tests/test_gpu_map_union.py."""
import ctypes as C

import numpy as np
import pytest

from test_map_kalman_host import _rows
from test_map_update_host import CTR, D, N, POSE, X, Y, _det, _p, _c, PCC


@pytest.fixture(scope="module")
def ca(host_binaries):
    import cape_amd

    cape_amd._host_library()
    return cape_amd


@pytest.fixture(scope="module")
def L(ca):
    L = ca._host_library()
    vp = C.c_void_p
    L.cape_host_covariance_valid.argtypes = [vp, C.c_int]
    L.cape_host_plane_covariance.argtypes = [vp, C.c_double, vp, vp]
    L.cape_host_world_plane_covariance.argtypes = [vp, C.c_double, vp, vp, vp, vp]
    L.cape_host_kalman_update.argtypes = [vp, vp, vp, vp, vp, vp]
    return L


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the pairs --------------------------------------------------------------------------------------------------------------------
def rect(x0, x1, y0, y1):
    return np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0]], np.float64)


def ngon(n, r, cx, cy, phase):
    t = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)


def comb(teeth=30, pitch=100.0, width=50.0, spine=100.0, length=3000.0):
    """a comb of `teeth` vertical teeth on a spine along x: 4 * teeth + 2 vertices"""
    pts = [(0.0, 0.0), ((teeth - 1) * pitch + width, 0.0)]
    for k in range(teeth - 1, -1, -1):
        x = k * pitch
        pts += [(x + width, spine), (x + width, length), (x, length), (x, spine)]
    return np.array(pts, np.float64)


C_SHAPE = np.array([[0, 0], [3000, 0], [3000, 1000], [1000, 1000], [1000, 2000], [3000, 2000], [3000, 3000], [0, 3000]], np.float64)
DIAMOND = np.array([[1000, 0], [0, 1000], [-1000, 0], [0, -1000]], np.float64)
COMB = comb()
assert len(COMB) == 122
# (name, ring a, ring b, expected class, expected vertex count or None)
SERVED, DISJOINT, NEW_HOLE, CAPACITY = "served", "disjoint", "new_hole", "capacity"
HAND_BUILT = [
    ("overlapping squares", rect(0, 400, 0, 400), rect(200, 600, 200, 600), SERVED, 8),
    ("big holds small", rect(-100, 700, -100, 700), rect(0, 400, 0, 400), SERVED, 4),
    ("small in big", rect(0, 400, 0, 400), rect(-100, 700, -100, 700), SERVED, 4),
    ("disjoint, map bigger", rect(0, 400, 0, 400), rect(5000, 5100, 0, 100), DISJOINT, 4),
    ("disjoint, detection bigger", rect(5000, 5100, 0, 100), rect(0, 400, 0, 400), DISJOINT, 4),
    ("square and diamond", rect(-1000, 1000, -1000, 1000), DIAMOND, SERVED, 4),
    ("a ring with itself", rect(0, 400, 0, 400), rect(0, 400, 0, 400), SERVED, 4),
    ("shared edge", rect(0, 400, 0, 400), rect(400, 800, 0, 400), SERVED, 4),
    ("two 128-gons", ngon(128, 1000, 0, 0, 0.01), ngon(128, 1000, 700, 100, 0.01), SERVED, 18),
    ("two 129-gons", ngon(129, 1000, 0, 0, 0.01), ngon(129, 1000, 700, 100, 0.01), CAPACITY, None),
    ("C shape and bar", C_SHAPE, rect(2500, 4000, 0, 3000), NEW_HOLE, None),
    ("crossed combs", COMB, COMB[:, ::-1] + [1450.0, 1525.0], NEW_HOLE, None),  # (841 holes; the device: DEVICE_CAPACITY below)
]


def cog(n=128, even=1000.0, odd=700.0):
    """a cog of n vertices whose radii alternate: simplify keeps every vertex"""
    t = 2 * np.pi * np.arange(n) / n
    r = np.where(np.arange(n) % 2 == 0, even, odd)
    return np.stack([r * np.cos(t), r * np.sin(t)], 1)


def subdivided(ring, parts=32):
    """every edge a -> b of the ring cut into `parts` equal parts: a + (b - a) * k / parts"""
    k = np.arange(parts)[:, None]
    return np.concatenate([a + (b - a) * k / parts for a, b in zip(ring, np.roll(ring, -1, axis=0))])


def saw(teeth=60):
    """a saw on a base along x: the valleys at y = 1000, the tips at y = 2000, 2 * teeth + 3 vertices"""
    pts = [(0.0, 0.0), (100.0 * teeth, 0.0)]
    for k in range(teeth, 0, -1):
        pts += [(100.0 * k, 1000.0), (100.0 * (k - 0.5), 2000.0)]
    return np.array(pts + [(0.0, 1000.0)], np.float64)


def about(ring, centre, M):
    """the ring's vertices about `centre` times the matrix M (row vectors)"""
    return (np.asarray(ring, np.float64) - centre) @ np.asarray(M, np.float64) + centre


def snag(teeth=32):
    """A U whose arms stand 30 apart.  The left arm's inner wall has a dent 9 deep, below simplify's tolerance of 10; the right arm's
    inner wall has a spike 38 long whose tip lies inside the dent.  Douglas-Peucker drops the dent and keeps the spike, so its
    candidate crosses itself and simplify keeps the ring as it is.  Saw teeth on the upper left wall (and those of snag_plate below it)
    bring the straightened wall to edge 127 of the candidate, the spike to edges 130 and 131: the only pairs of edges that meet."""
    pts = [(-100.0, -100.0), (130.0, -100.0), (130.0, 1000.0), (30.0, 1000.0), (30.0, 505.0), (-8.0, 500.0), (30.0, 495.0), (30.0, 0.0),
           (0.0, 0.0), (0.0, 480.0), (-9.0, 490.0), (-9.0, 510.0), (0.0, 520.0), (0.0, 1000.0), (-50.0, 1050.0)]
    pitch = 600.0 / teeth
    for k in range(teeth):
        pts += [(-200.0, 1000.0 - pitch * (k + 0.5))] + ([(-100.0, 1000.0 - pitch * (k + 1))] if k + 1 < teeth else [])
    return np.array(pts, np.float64)


def snag_plate(teeth=32):
    """a plate on the lower left wall of snag() with saw teeth of its own, further out"""
    pts = [(-50.0, -80.0), (-50.0, 380.0), (-150.0, 380.0)]
    pitch = 460.0 / teeth
    for k in range(teeth):
        pts += [(-300.0, 380.0 - pitch * (k + 0.5)), (-150.0, 380.0 - pitch * (k + 1))]
    return np.array(pts, np.float64)


COG = cog()
PINCH_8 = np.array([[0, 0], [400, 400], [800, 0], [800, 800], [400, 400], [0, 800]], np.float64)
PINCH_10 = np.array([[0, 0], [400, 400], [800, 0], [900, 400], [400, 400], [800, 800], [400, 900], [400, 400], [0, 800]], np.float64)
PINCH_TURNED = about(PINCH_8, [400.0, 400.0], [[.6, .8], [-.8, .6]])
# One node more than the device holds.  Two rings of at most 128 vertices whose union has no hole weave around each other like the
# half-step 128-gons, which use every vertex and reach CAPE_MAP_UNION_MAX_NODES exactly; more nodes need edges that cross many
# edges, which encloses cells: three horizontal teeth across the 30 vertical ones cross 360 times, 122 + 14 + 360 = 496 nodes, and 17
# more vertices on the spine of ring b make 513.
RAKE = comb(3, length=3200.0)[:, ::-1] + [-150.0, 1000.0]
RAKE = np.concatenate([RAKE[:1], [[-150.0, 1000.0 + 10.0 * k] for k in range(1, 18)], RAKE[1:]])
assert len(COG) == 128 and len(subdivided(rect(0, 400, 0, 400))) == 128 and len(saw()) == 123 and len(RAKE) == 31
# The long pairs: operands of more than 64 vertices, whose cut lists, arrangements, walked faces, erased tails, Douglas-Peucker spans
# and candidates all span more than one 64-wide chunk of the device's lane loops.  (name, ring a, ring b, expected class, expected
# vertex count or None) like HAND_BUILT; LONG_NODES holds the arrangement's node count per pair from the one-lane port
# (tests/host/map_union_algebra.cpp prints them), the reference for the device's n_nodes.
LONG_PAIRS = [
    ("half-step 128-gons", ngon(128, 1000, 0, 0, 0), ngon(128, 1000, 0, 0, np.pi / 128), SERVED, 16),
    ("mirrored cogs", COG, COG * [1.0, -1.0] + [150.0, 40.0], SERVED, 188),
    ("half-step cogs", COG, cog(even=700.0, odd=1000.0), SERVED, 256),
    ("subdivided squares", subdivided(rect(0, 400, 0, 400)), subdivided(rect(200, 600, 200, 600)), SERVED, 8),
    ("comb and foot", COMB, rect(-50, 100, -50, 50), SERVED, 124),
    ("saw and bar", saw(), rect(100, 5900, 500, 1500), SERVED, 122),
    ("comb of 9 and bar", comb(9), rect(-100, 1000, 1500, 1600), NEW_HOLE, None),
    ("comb of 10 and bar", comb(10), rect(-100, 1100, 1500, 1600), NEW_HOLE, None),
    ("comb of 30 and bar", COMB, rect(-100, 3100, 1500, 1600), NEW_HOLE, None),
    ("pinched rings, degree 8", PINCH_8, PINCH_TURNED, SERVED, 16),
    ("pinched rings, degree 10", PINCH_10, PINCH_TURNED, SERVED, 17),
    ("comb and rake, 513 nodes", COMB, RAKE, NEW_HOLE, None),
    ("snag at candidate edge 127", snag(), snag_plate(), SERVED, 159),
]
# what the device alone hands to the host (CAPE_UNION_HOST_CAPACITY) where the twin has an answer, the class of the table: more cuts
# than its list holds (3 600), a node of 10 neighbours, and an arrangement of more than CAPE_MAP_UNION_MAX_NODES nodes
DEVICE_CAPACITY = ("crossed combs", "pinched rings, degree 10", "comb and rake, 513 nodes")
LONG_NODES = {
    "two 128-gons": 258, "half-step 128-gons": 512, "mirrored cogs": 386, "half-step cogs": 384, "subdivided squares": 254,
    "comb and foot": 128, "saw and bar": 243, "comb of 9 and bar": 78, "comb of 10 and bar": 86, "comb of 30 and bar": 246,
    "pinched rings, degree 8": 15, "pinched rings, degree 10": 15, "comb and rake, 513 nodes": 513, "snag at candidate edge 127": 177,
}
ALL_PAIRS = HAND_BUILT + LONG_PAIRS


def star(rng, n, cx, cy):
    t = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = 1000 * rng.uniform(0.5, 1, n)
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)


def star_pairs(n, count=200, seed=1):
    rng = np.random.default_rng(seed)
    return [(star(rng, n, 0, 0), star(rng, n, rng.uniform(-600, 600), rng.uniform(-600, 600))) for _ in range(count)]


def classify(ca, flags):
    if flags & ca.UNION_HOST_NEW_HOLE:
        return NEW_HOLE
    if flags & (ca.UNION_HOST_CAPACITY | ca.UNION_HOST_AMBIGUOUS | ca.UNION_HOST_MAP_HOLES):
        return CAPACITY
    assert flags & ca.UNION_SERVED
    return DISJOINT if flags & ca.UNION_DISJOINT else SERVED


# ---- one pair through the update and through the twin -----------------------------------------------------------------------------
def _one_plane_map(ca, L, ring, holes=()):
    cov = np.zeros(16)
    assert L.cape_host_plane_covariance(_p(N), D, _p(_c(PCC)), _p(cov)) == 1
    tracks = np.zeros(1, ca.MAP_TRACK_DTYPE)
    tracks[0]["covariance"] = cov.reshape(4, 4)
    return ca.pack_map([(N, D, X, Y, CTR, ring, list(holes))]), tracks


def _world(ring):
    """the detection's world ring for the identity pose: the ring as the host class holds it (clockwise)"""
    x, y = ring[:, 0], ring[:, 1]
    return ring[::-1].copy() if 0.5 * (np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))) > 0 else ring.copy()


def _measurement_rows(ca, L, det):
    rows = _rows(ca, L, det, np.eye(4), POSE)
    for r, d in zip(rows, det):
        r["x_axis"], r["y_axis"], r["center"], r["vertex_count"] = d[2], d[3], d[4], len(d[5])
    return rows


def _pair_against_the_update(ca, L, a, b, d=1010.0, holes=()):
    """ring a as the map plane, ring b as the detection at distance d: (the twin's row, its ring, the update's new plane, its outer
    ring).  A served ring and its frame must be the update's new polygon bit for bit."""
    arrays, tracks = _one_plane_map(ca, L, a, holes)
    det = [_det(b, d=d)]
    (P, R, V), Tr, _, _ = ca.host_map_update(arrays, tracks, [0], det, np.eye(4), POSE)
    assert Tr[0]["result"] & ca.MAP_RESULT_UPDATED
    mrows = _measurement_rows(ca, L, det)
    _, frows, _ = ca.host_map_kalman(arrays, tracks, [0], mrows)
    rows, rings = ca.host_map_union(arrays, [0], frows, mrows, [_world(b)])
    r0 = R[P[0]["ring_first"]]
    outer = V[r0["vertex_offset"]: r0["vertex_offset"] + r0["vertex_count"]]
    row = rows[0]
    assert row["map_plane"] == 0
    if row["flags"] & ca.UNION_SERVED:
        assert P[0]["ring_count"] == 1 and not Tr[0]["result"] & ca.MAP_RESULT_OVERFLOW
        assert row["vertex_count"] == len(outer) and np.array_equal(_bits(rings[0]), _bits(outer))
        for k in ("x_axis", "y_axis", "center"):
            assert np.array_equal(_bits(row[k]), _bits(P[0][k])), k
        x, y = outer[:, 0], outer[:, 1]
        assert abs(row["area"] - 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))) <= 1e-9 * row["area"]
    else:
        assert rings[0] is None and row["vertex_count"] == 0 and row["area"] == 0 and not row["x_axis"].any()
        if row["flags"] & ca.UNION_HOST_NEW_HOLE:  # the update adds the holes, or -- more than CAPE_MAP_MAX_HOLES -- keeps the old polygon
            assert row["flags"] == ca.UNION_HOST_NEW_HOLE
            assert P[0]["ring_count"] > 1 or (Tr[0]["result"] & ca.MAP_RESULT_OVERFLOW and P[0]["ring_count"] == 1 and len(outer) == len(a))
    return row, rings[0], P[0], outer


@pytest.mark.parametrize("case", ALL_PAIRS, ids=[c[0] for c in ALL_PAIRS])
@pytest.mark.parametrize("d", [D, 1010.0], ids=["same plane", "fused plane"])
def test_hand_built_pairs_equal_the_update(ca, L, case, d):
    _, a, b, cls, count = case
    row, ring, _, _ = _pair_against_the_update(ca, L, a, b, d=d)
    assert classify(ca, int(row["flags"])) == cls
    # (the vertex counts of the table hold in the canonical frame: test_ring_union_twin_classes.  Here the Kalman step moves the frame,
    #  and the count is the update's own, checked above.)
    if cls == DISJOINT:
        assert row["flags"] == ca.UNION_SERVED | ca.UNION_DISJOINT
    if cls == CAPACITY:
        assert row["flags"] == ca.UNION_HOST_CAPACITY


@pytest.mark.parametrize("n", [8, 24])
def test_star_sets_equal_the_update(ca, L, n):
    holes = 0
    for a, b in star_pairs(n):
        row, _, _, _ = _pair_against_the_update(ca, L, a, b)
        cls = classify(ca, int(row["flags"]))
        assert cls in (SERVED, DISJOINT, NEW_HOLE)  # (a star need not hold its own centre: a few pairs are disjoint)
        holes += cls == NEW_HOLE
    print(f"{n}-vertex stars: {holes} of 200 pairs make a hole")
    assert holes <= 10  # at most 5 % of a set


def test_ring_union_twin_classes(ca):
    for name, a, b, cls, count in ALL_PAIRS:
        row, ring = ca.host_ring_union(a, b)
        assert classify(ca, int(row["flags"])) == cls, name
        assert row["map_plane"] == 0 and row["n_nodes"] == 0
        if count is not None:
            assert len(ring) == count == row["vertex_count"], name
    # merge_union returns false where the outer face is no simple ring (a map ring that crosses itself, beside a small detection): the
    # projected map ring as it is, not simplified
    bowtie = np.array([[0, 0], [400, 400], [400, 0], [0, 300.0]])
    row, ring = ca.host_ring_union(bowtie, rect(1000, 1010, 0, 10))
    assert row["flags"] == ca.UNION_SERVED | ca.UNION_UNCHANGED | ca.UNION_DISJOINT and np.array_equal(ring, bowtie) and row["area"] == 20000.0
    # the map ring's own frame is kept where it already is the target: the canonical frames
    row, ring = ca.host_ring_union(rect(0, 400, 0, 400), rect(200, 600, 200, 600))
    assert row["x_axis"].tolist() == [1, 0, 0] and row["y_axis"].tolist() == [0, 1, 0] and row["center"].tolist() == [0, 0, 0]
    assert row["area"] == 400 * 400 * 2 - 200 * 200


def test_a_map_plane_with_a_hole_is_the_hosts(ca, L):
    hole = rect(100, 200, 100, 200)
    row, ring, _, _ = _pair_against_the_update(ca, L, rect(0, 400, 0, 400), rect(200, 600, 200, 600), holes=[hole])
    assert row["flags"] == ca.UNION_HOST_MAP_HOLES and ring is None


def test_an_unmatched_or_failed_pair_has_no_row(ca, L):
    arrays, tracks = _one_plane_map(ca, L, rect(0, 400, 0, 400))
    det = [_det(rect(5000, 5400, 0, 400)), _det(rect(200, 600, 200, 600), d=1010.0)]
    mrows = _measurement_rows(ca, L, det)
    worlds = [_world(d[5]) for d in det]
    _, frows, _ = ca.host_map_kalman(arrays, tracks, [1], mrows)
    rows, rings = ca.host_map_union(arrays, [1], frows, mrows, worlds)
    assert rows[0]["map_plane"] == -1 and rows[0].tobytes()[:80] == bytes(80) and rows[0]["flags"] == 0 and rings[0] is None
    assert rows[1]["map_plane"] == 0 and rows[1]["flags"] == ca.UNION_SERVED and rows[1]["vertex_offset"] == 0
    # the match says otherwise: no pair
    rows, _ = ca.host_map_union(arrays, [-1], frows, mrows, worlds)
    assert rows[1]["map_plane"] == -1 and rows[1]["flags"] == 0
    # the detection's polygon failed in cape_map_measure: cape_map_kalman reports FAIL_POLYGON, and there is no pair
    mrows[1]["flags"] = ca.MEASURE_KEPT | ca.MEASURE_FAIL_POLYGON
    _, frows, res = ca.host_map_kalman(arrays, tracks, [1], mrows)
    assert res[0]["result"] & ca.MAP_RESULT_FAIL_POLYGON and frows[1]["flags"] & ca.FUSION_FRAME
    rows, rings = ca.host_map_union(arrays, [1], frows, mrows, worlds)
    assert rows[1]["map_plane"] == -1 and rows[1]["flags"] == 0 and rings[1] is None
    # the Kalman step failed: no frame, no pair
    mrows = _measurement_rows(ca, L, det)
    mrows[1]["flags"] = ca.MEASURE_KEPT | ca.MEASURE_FAIL_WORLD_COV
    _, frows, _ = ca.host_map_kalman(arrays, tracks, [1], mrows)
    rows, _ = ca.host_map_union(arrays, [1], frows, mrows, worlds)
    assert rows[1]["map_plane"] == -1


def test_the_frames_slab_fills_up_in_kept_plane_order(ca, L):
    """12 pairs of 128-vertex cogs whose unions keep some 250 vertices each do not fit 2 048: the first ones are served back to back,
    the rest are HOST_CAPACITY."""
    n_pairs = 12
    t = 2 * np.pi * np.arange(128) / 128
    r = np.where(np.arange(128) % 2 == 0, 1000.0, 700.0)  # a cog: simplify keeps every vertex
    cog = np.stack([r * np.cos(t), r * np.sin(t)], 1)
    planes = [(N, D, X, Y, CTR, cog + [5000.0 * j, 0], []) for j in range(n_pairs)]
    arrays = ca.pack_map(planes)
    cov = np.zeros(16)
    assert L.cape_host_plane_covariance(_p(N), D, _p(_c(PCC)), _p(cov)) == 1
    tracks = np.zeros(n_pairs, ca.MAP_TRACK_DTYPE)
    tracks["covariance"] = cov.reshape(4, 4)
    det = [_det(cog * [1.0, -1.0] + [5000.0 * j + 150.0, 40.0]) for j in range(n_pairs)]
    mrows = _measurement_rows(ca, L, det)
    match = list(range(n_pairs))
    _, frows, _ = ca.host_map_kalman(arrays, tracks, match, mrows)
    rows, rings = ca.host_map_union(arrays, match, frows, mrows, [_world(d[5]) for d in det])
    served = [bool(r["flags"] & ca.UNION_SERVED) for r in rows]
    assert served[0] and not served[-1] and served == sorted(served, reverse=True)
    used = 0
    for r, ring in zip(rows, rings):
        if r["flags"] & ca.UNION_SERVED:
            assert r["vertex_offset"] == used and len(ring) == r["vertex_count"]
            used += int(r["vertex_count"])
        else:
            assert r["flags"] == ca.UNION_HOST_CAPACITY and ring is None
    assert used <= ca.MAP_UNION_FRAME_VERTICES
    first_refused = served.index(False)
    # ... and the refused one would not have fitted: the update's polygon for it is longer than what was left
    (P, R, V), _, _, _ = ca.host_map_update(arrays, tracks, match, det, np.eye(4), POSE)
    assert R[P[first_refused]["ring_first"]]["vertex_count"] > ca.MAP_UNION_FRAME_VERTICES - used


def test_argument_checks(ca):
    Lh = ca._host_library()
    row = np.zeros(128, ca.PLANE_UNION_DTYPE)
    ver = np.zeros((ca.MAP_UNION_FRAME_VERTICES, 2))
    sq = rect(0, 1, 0, 1)
    assert Lh.cape_host_map_union(None, None, None, None, None, 0, row.ctypes.data, ver.ctypes.data) == -1
    src, view = ca._map_arrays(ca.pack_map([(N, D, X, Y, CTR, sq, [])]))
    assert Lh.cape_host_map_union(C.byref(view), None, None, None, None, 0, row.ctypes.data, ver.ctypes.data) == 0
    assert Lh.cape_host_map_union(C.byref(view), None, None, None, None, 1, row.ctypes.data, ver.ctypes.data) == -1
    assert Lh.cape_host_map_union(C.byref(view), None, None, None, None, -1, row.ctypes.data, ver.ctypes.data) == -1
    assert Lh.cape_host_map_union(C.byref(view), None, None, None, None, 129, row.ctypes.data, ver.ctypes.data) == -1
    assert Lh.cape_host_map_union(C.byref(view), None, None, None, None, 0, None, ver.ctypes.data) == -1
    assert Lh.cape_host_map_union(C.byref(view), None, None, None, None, 0, row.ctypes.data, None) == -1
    assert Lh.cape_host_ring_union(None, 4, sq.ctypes.data, 4, None, row.ctypes.data, ver.ctypes.data) == -1
    assert Lh.cape_host_ring_union(sq.ctypes.data, 2, sq.ctypes.data, 4, None, row.ctypes.data, ver.ctypes.data) == -1
    assert Lh.cape_host_ring_union(sq.ctypes.data, 4, sq.ctypes.data, 4097, None, row.ctypes.data, ver.ctypes.data) == -1
    assert Lh.cape_host_ring_union(sq.ctypes.data, 4, sq.ctypes.data, 4, None, None, ver.ctypes.data) == -1
    assert Lh.cape_host_ring_union(sq.ctypes.data, 4, sq.ctypes.data, 4, None, row.ctypes.data, ver.ctypes.data) == 0
    with pytest.raises(ca.CapeError, match="one measurement row"):
        ca.host_map_union(ca.pack_map([(N, D, X, Y, CTR, sq, [])]), [0], np.zeros(1, ca.PLANE_FUSION_DTYPE),
                          np.zeros(2, ca.PLANE_MEASUREMENT_DTYPE), [sq])

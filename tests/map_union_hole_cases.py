"""The pairs of the holes mode of the polygon union (cape_map_union_holes, cape_debug_polygon_union and their host twins), shared by
tests/test_map_union_holes_host.py and tests/test_gpu_map_union_holes.py.  Built from the generators of tests/test_map_union_host.py.
A row is (name, [outer ring, hole, ...] of the map plane, the detection's ring, outcome); the outcome is the list of ring lengths of
the served polygon in the canonical frame, or CAPACITY / HOLE_CUT.  The outcomes were measured on the CPU with the host class."""
import numpy as np

from test_map_union_host import C_SHAPE, cog, comb, ngon, rect, star_pairs

CAPACITY, HOLE_CUT = "capacity", "hole_cut"


def _bar(teeth):
    return rect(-100, 100 * teeth + 100, 1500, 1600)


# a union that encloses faces: they become interior rings in face-walk order
NEW_HOLES = [
    ("C shape and bar", [C_SHAPE], rect(2500, 4000, 0, 3000), [4, 4]),
    ("comb of 2 and bar", [comb(2)], rect(-100, 300, 1500, 1600), [16, 4]),
    ("comb of 3 and bar", [comb(3)], _bar(3), [20, 4, 4]),
    ("comb of 9 and bar", [comb(9)], _bar(9), [44] + [4] * 8),  # exactly CAPE_MAP_MAX_HOLES
    ("comb of 10 and bar", [comb(10)], _bar(10), CAPACITY),  # 9 holes: the update reports OVERFLOW and keeps the 42-vertex ring
    ("comb of 30 and bar", [comb(30)], _bar(30), CAPACITY),  # 29 holes
]

MAP = rect(0, 1000, 0, 1000)
MID = rect(400, 500, 400, 500)
EIGHT = [rect(100 + 90 * k, 150 + 90 * k, 100, 150) for k in range(8)]
DENTED = np.array([[100, 100], [100, 200], [150, 200.5], [200, 200], [200, 100]], np.float64)
TRIANGLE = np.array([[100, 100], [200, 100], [150, 200]], np.float64)
# cogs whose teeth are shallow enough for the intersection's 16 edges of a ring over one slab, inside an outer ring large enough
# that simplify's tolerance (area / 1e5) does not matter to the capacity rule, which counts the vertices before simplify
BIG = rect(0, 10000, 0, 10000)
COGS = [cog(128, 500.0, 480.0) + [1500.0 + 2000.0 * k, 5000.0] for k in range(4)]
BIG_DETECTION = rect(9000, 11000, 0, 10000)
DENTED_MAP = np.array([[0, 0], [0, 1000], [300, 1000.5], [1000, 1000], [1000, 0]], np.float64)
NEW_AND_KEPT, TINY, SMALL_TRIANGLE = [4, 4, 4], [8, 4], [8, 3]
HOLED_MAPS = [
    ("a hole clear of the detection", [MAP, rect(100, 200, 100, 200)], rect(600, 1400, 600, 1400), [8, 4]),
    ("a hole touching the detection in a corner", [MAP, rect(500, 600, 500, 600)], rect(600, 1400, 600, 1400), [8, 4]),
    ("a covered hole", [MAP, MID], rect(300, 1200, 300, 1200), [8]),
    ("a partly covered hole", [MAP, MID], rect(450, 1200, 450, 1200), HOLE_CUT),  # the update gives [8, 6]
    # two pieces, the holed map the bigger one: on the right of it the small detection is no part of the outer face and the hole is
    # carried like any other; on the left the outer face is the detection's, the disjoint rule fires and simplify() takes the
    # projected map polygon with its hole
    ("disjoint, the holed map bigger", [MAP, MID], rect(5000, 5100, 0, 100), [4, 4]),
    ("disjoint, the holed map bigger, the rule fires", [MAP, MID], rect(-5100, -5000, 0, 100), [4, 4]),
    # a bigger detection far away: on the right the outer face walked from the leftmost node is the map's, the disjoint rule fires and
    # the map's hole goes with the map; on the left the outer face is the detection's ring alone, the rule does not fire, and the
    # map's hole is kept -- outside its new outer ring
    ("disjoint, the detection bigger, on the right", [rect(0, 400, 0, 400), rect(100, 200, 100, 200)], rect(5000, 6000, 0, 1000), [4]),
    ("the outer face is the detection's", [rect(0, 400, 0, 400), rect(100, 200, 100, 200)], rect(-6000, -5000, 0, 1000), [4, 4]),
    ("eight holes", [MAP] + EIGHT, rect(900, 1400, 0, 1000), [4] + [4] * 8),
    ("eight holes and a new one", [C_SHAPE] + EIGHT, rect(2500, 4000, 0, 3000), CAPACITY),  # 9 holes
    ("Douglas-Peucker drops a hole's vertex", [MAP, DENTED], rect(600, 1400, 600, 1400), [8, 4]),
    ("a triangular hole", [MAP, TRIANGLE], rect(600, 1400, 600, 1400), [8, 3]),
    ("a hole of 128 vertices", [MAP, ngon(128, 200, 300, 300, 0.01)], rect(600, 1400, 600, 1400), [8, 16]),
    ("a hole of 129 vertices", [MAP, ngon(129, 200, 300, 300, 0.01)], rect(600, 1400, 600, 1400), CAPACITY),
    # a new hole and a kept one: the new ones come first
    ("a new hole before a kept one", [C_SHAPE, rect(100, 200, 100, 200)], rect(2500, 4000, 0, 3000), NEW_AND_KEPT),
    # the detection covers exactly tiny = 1e-12 * 2^20 of the hole (a 2^-10 x 1e-12 * 2^30 corner): covered <= tiny keeps the hole
    ("a hole covered by exactly tiny", [rect(-512, 512, -512, 512), rect(-100, 0, -100, 0)], rect(-2.0 ** -10, 600, -1e-12 * 2.0 ** 30, 600), TINY),
    # a triangle no Douglas-Peucker pass would leave standing (every vertex within the tolerance of vertex 0) is skipped by simplify,
    # which goes on to drop the outer ring's shallow vertex
    ("a small triangle under a dented outer ring", [DENTED_MAP, np.array([[100, 100], [105, 100], [102, 105]], np.float64)],
     rect(600, 1400, 600, 1400), SMALL_TRIANGLE),
    # a 5 x 5 hole's candidate is a single vertex: simplify replaces no ring, the dented hole keeps its fifth vertex
    ("an invalid candidate keeps every ring", [MAP, DENTED, rect(700, 705, 100, 105)], rect(600, 1400, 600, 1400), [8, 5, 4]),
    # simplify's tolerance comes from the area without the holes: 88.5 with the big hole, which keeps its vertex 100 off the edge
    # (180 from the outer ring alone would drop it)
    ("the tolerance counts the holes out", [rect(0, 4000, 0, 4000), np.array([[500, 500], [500, 3500], [2000, 3600], [3500, 3500], [3500, 500]], np.float64)],
     rect(3800, 4500, 0, 4000), [4, 5]),
    ("four cog holes, 512 vertices", [BIG] + COGS, BIG_DETECTION, [4, 128, 128, 128, 128]),
    ("four cog holes and a triangle, 515 vertices", [BIG] + COGS + [TRIANGLE], BIG_DETECTION, CAPACITY),
]
TABLES = NEW_HOLES + HOLED_MAPS
# cape_host_map_update works in the frame of tests/test_map_update_host.py (X, Y), not the canonical one, and which piece holds the
# leftmost node depends on the frame: there these disjoint pairs come out as follows (measured, like the rest)
IN_THE_UPDATES_FRAME = {"disjoint, the detection bigger, on the right": [4, 4], "the outer face is the detection's": [4, 4]}


def square_hole(ring, side=40.0):
    """a side x side square centred at the ring's vertex mean"""
    cx, cy = np.asarray(ring, np.float64).mean(axis=0)
    return rect(cx - side / 2, cx + side / 2, cy - side / 2, cy + side / 2)


def holed_star_pairs(n, count=200):
    """star_pairs(n) with a 40 x 40 square hole centred at ring a's vertex mean: ([a, hole], b)"""
    return [([a, square_hole(a)], b) for a, b in star_pairs(n, count)]


def tilted_frames():
    """27 doubles: ring a's frame, ring b's frame and the target, three different frames of the same plane (rotations about its
    normal and shifts inside it), so that Polygon::project moves every vertex of every ring"""
    def frame(angle, shift):
        n = np.array([1.0, 2.0, 2.0]) / 3.0
        u = np.cross(n, [0.0, 0.0, 1.0])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        x, y = np.cos(angle) * u + np.sin(angle) * v, -np.sin(angle) * u + np.cos(angle) * v
        return np.concatenate([x, y, 1000.0 * n + shift[0] * u + shift[1] * v])
    return np.concatenate([frame(0.0, (0.0, 0.0)), frame(0.3, (25.0, -40.0)), frame(-0.2, (-10.0, 15.0))])

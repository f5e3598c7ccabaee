"""The pairs of the cut mode of the polygon union (cape_map_union_cut, cape_debug_polygon_union_cut and their host twins): a hole of the
map plane that the detection covers in part is cut into the pieces of (hole minus detection).  Shared by
tests/test_map_union_cut_host.py and tests/test_gpu_map_union_cut.py; tests/host/map_union_cut_algebra.cpp runs the same rings through
the one-lane port.  A row is (name, [outer ring, hole, ...] of the map plane, the detection's ring, outcome) in the format of
tests/map_union_hole_cases.py; the outcome is the list of ring lengths of the served polygon after simplify -- the outer ring, the
new holes, then per hole of the map plane the kept hole or its pieces in face-walk order -- or CAPACITY.  The outcomes were measured
on the CPU with the host class (merge_union, canonical frame).  The lengths are only a row's label: where the order of the pieces or
of their vertices is the point of a row, what checks it is the comparison of every vertex, bit for bit, with the twin."""
import numpy as np

from map_union_hole_cases import CAPACITY, EIGHT, MAP, MID
from test_map_union_host import C_SHAPE, cog, comb, ngon, rect

FORK = np.array([[300, 300], [300, 1200], [700, 1200], [700, 300], [600, 300], [600, 1100], [400, 1100], [400, 300]], np.float64)
WIDE = rect(200, 800, 400, 500)
BAR = rect(440, 460, 300, 1200)
# Two combs across each other inside a map plane so large (tiny = 1e-12 * 4e10 = 0.04) that what the detection's thick teeth leave of
# the hole's thin ones (0.001 x 5 each) is no piece, while what they cover of them (0.001 x 95 each) is far more than tiny: the
# hole is cut, and the host class serves the pair with ONE piece, the spine with the stubs of its teeth.  The hole's 11 teeth stand
# upright, the detection's 11 lie across them, each pair of teeth crosses four times: 46 + 46 + 484 = 576 distinct points, of which the
# arrangement of (hole, detection) numbers 554 nodes (measured with the one-lane port) from 968 cuts -- beyond
# CAPE_MAP_UNION_MAX_NODES, within the 1 024 cuts.  The device and the port answer CAPACITY; the twins, which are the host class, serve.
HUGE = rect(-1e5, 1e5, -1e5, 1e5)
WIDE_MAP = rect(-1e4, 1e4, -1e4, 1e4)
UPRIGHT = comb(11, 100.0, 0.001, 100.0, 1590.0)
LYING = comb(11, 100.0, 95.0, 100.0, 2000.0)[:, ::-1] + [-500.0, 500.0]
CROSSED_COMBS = "crossed combs: the second arrangement beyond 512 nodes"
COG_ACROSS = "a cog across a 128-gon"
COG_64 = "a cog of 64 vertices across a 128-gon"
# four holes of 126 vertices, 504 in all, each cut in two by a bar that passes between their vertices: four crossings each make 520
# interior vertices before simplify, in eight rings
FOUR = [ngon(126, 100.0, 150.0 + 230.0 * k, 200.0, np.pi / 126) for k in range(4)]

CUT_HOLES = [
    ("an L-shaped piece", [MAP, MID], rect(450, 1200, 450, 1200), [8, 6]),
    ("a bar cuts the hole in two", [MAP, MID], BAR, [8, 4, 4]),  # the order of the two is the face walk's
    # holes_new = 1 (the face between the fork's prongs above the map), then the three pieces of the wide hole: new holes come first
    ("a fork: a new hole, then three pieces", [MAP, rect(100, 900, 400, 500)], FORK, [8, 4, 4, 4, 4]),
    # collinear cuts with the hole in ring A's role
    ("the detection's edge on the hole's edge line", [MAP, MID], rect(450, 1200, 400, 1200), [8, 4]),
    # these two bracket the `cut` decision: kept, not cut; covered, not cut
    ("kept: the edge runs along the hole's side", [MAP, MID], rect(500, 1200, 300, 1200), [8, 4]),
    ("covered: the corner on the hole's corner", [MAP, MID], rect(400, 1200, 400, 1200), [8]),
    ("a triangular piece", [MAP, MID], np.array([[390, 510], [390, 1200], [1200, 1200], [1200, 300], [510, 300], [510, 390]], np.float64),
     [8, 3]),  # simplify skips it
    # angles of the second walk that are not axis-parallel
    ("a tilted bar", [MAP, MID], np.array([[430, 300], [450, 300], [470, 1200], [450, 1200]], np.float64), [8, 4, 4]),
    ("kept, cut and covered", [MAP, rect(100, 200, 100, 200), MID, rect(700, 800, 700, 800)], rect(450, 1200, 450, 1200), [8, 4, 6]),
    ("new, kept and a piece", [C_SHAPE, rect(100, 200, 100, 200), rect(2400, 2600, 100, 200)], rect(2500, 4000, 0, 3000), [4, 4, 4, 4]),
    ("exactly eight interior rings", [MAP] + EIGHT[:6] + [WIDE], BAR, [8] + [4] * 8),  # CAPE_MAP_MAX_HOLES
    ("nine interior rings", [MAP] + EIGHT[:7] + [WIDE], BAR, CAPACITY),  # the update reports OVERFLOW
    # HOLE_PIECES with no piece: the 1e-7 wide sliver is cut, and falls to drop_collinear
    ("a sliver piece falls to drop_collinear", [MAP, MID], rect(400.0000001, 1200, 300, 1200), [8]),
    ("a sliver just above tiny", [rect(-512, 512, -512, 512), rect(-100, 0, -100, 0)], rect(-100 + 2.0 ** -20, 600, -600, 600), [8, 4]),
    ("99 interior vertices before simplify", [MAP, ngon(128, 200, 300, 300, 0.01)], rect(300, 1400, 300, 1400), [8, 8]),
    # three pieces and the largest second arrangement of the table that the host class serves (262 nodes).  rings_inter_area(hole,
    # detection) cuts the x range of BOTH rings into slabs, and at the cog's own left and right ends up to 26 of its edges lie over one
    # slab, beyond the 16 of the device's tier: the device answers CAPACITY before it cuts anything (COG_ACROSS below), wherever the
    # cog stands.  A cog of half as many teeth (14 edges over a slab) is the row the device serves
    (COG_ACROSS, [rect(0, 4000, 0, 4000), ngon(128, 500, 1000, 1000, 0.01)], cog(128, 900.0, 700.0) + [1700.0, 1000.0], [4, 8, 85, 7]),
    (COG_64, [rect(0, 4000, 0, 4000), ngon(128, 500, 1000, 1000, 0.01)], cog(64, 900.0, 700.0) + [1700.0, 1000.0], [4, 11, 73, 10]),
    # A map plane of 2e4 x 2e4: tiny = 4e-4, the first arrangement's eps = 1e-5; the hole and the detection stay within 600 of the
    # origin, so the second arrangement's own eps is 6e-7.  Two pieces, of which the 2^-12 x 1 sliver on the left (2.44e-4) is below tiny
    # and nothing but the `> tiny` filter removes it (drop_collinear's threshold is 1e-9 here, and the sliver is simple) ...
    ("a second piece below tiny", [WIDE_MAP, rect(-100, 0, -1, 0)], rect(-100 + 2.0 ** -12, -50, -600, 600), [4, 4]),
    # ... and a sliver 2^-18 wide (3.8e-6) and 200 high, above tiny: its two sides are one node each under the first arrangement's
    # eps and four nodes under the second's own
    ("a sliver narrower than the first eps", [WIDE_MAP, rect(-100, 0, -200, 0)], rect(-100 + 2.0 ** -18, 600, -600, 600), [4, 4]),
    (CROSSED_COMBS, [HUGE, UPRIGHT], LYING, [4, 44]),
    ("four holes cut in two: 520 interior vertices", [rect(0, 1000, 0, 400)] + FOUR, rect(20, 1200, 199, 201), CAPACITY),
]
# the rows where merge_union's `cut` branch runs: the twins set HOLE_PIECES there (with SERVED), and nowhere else
PIECES = {name for name, _, _, _ in CUT_HOLES} - {"kept: the edge runs along the hole's side", "covered: the corner on the hole's corner",
                                                   "nine interior rings", "four holes cut in two: 520 interior vertices"}
# The rows the device hands to the host although the host class, and with it the twins, serves them: a capacity the twins do not
# have.  The crossed combs exceed the second arrangement's nodes, which the one-lane port restates: it answers CAPACITY too.  The cog
# across the 128-gon exceeds the intersection's edges over one slab, which the port takes from the host class: it serves the row.
DEVICE_CAPACITY = (CROSSED_COMBS, COG_ACROSS)
# cape_host_map_update works in the frame of tests/test_map_update_host.py (X, Y), not the canonical one.  Which node an arrangement
# starts from, and with it the order in which the faces are walked and the vertex a piece begins with, depends on the frame: there the
# three pieces of the two cog rows come out in another order, and Douglas-Peucker, which starts from a piece's first vertex, leaves the
# long piece of the 128-gon one vertex more (measured, like the rest).  No row changes between served and CAPACITY.
IN_THE_UPDATES_FRAME = {"99 interior vertices before simplify": [8, 9], COG_ACROSS: [4, 7, 85, 8],
                        COG_64: [4, 10, 73, 11]}

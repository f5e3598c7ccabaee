"""Hand-made ring pairs for the ring intersection of csrc/cape_ring_area.h (rings_inter_area / rings_inter_area_coop and the
four-tier walk around them), with an exact reference.  Plain Python, no GPU.

A case is one detection ring against one map polygon (outer ring + holes), both in the canonical plane frame -- x axis (1,0,0), y axis
(0,1,0), normal (0,0,1), identity pose -- with integer vertices below 2^20 in magnitude, so that every projection on the way to the
kernel is exact and the kernel sees the numbers written here.

  exact_inter_area(case)  the area of detection n (outer minus holes) in rational arithmetic, by slabs
  demand(case)            what the kernel needs for the pair: ring length, boundaries before std::unique, edges of a ring over a slab
  expected_walk(demand)   the capacity table and the leave rule restated: tiers visited, the tier that serves (None: no tier does)

Host class against exact_inter_area over this table (tests/test_ring_pair_cases.py prints it):
  worst relative error observed: 1.62e-14 (case `two_overflows_t2`: up to 17 trapezoids in each of 1 053 slabs; 1.13e-14 on `xs2048`,
  below 1e-15 on every case of at most 1 025 boundaries)
  bound = 10 x observed, the margin for the association order that differs between slabs of a case: HOST_RTOL = 1.7e-13
  (far below the suite's AREA_RTOL = 1e-9 of tests/test_gpu_polygon_oracle.py: nothing to report)

Boundaries of the first tier: 256 exactly IS reachable with rings of <= 32 vertices and <= 6 edges over a slab (`t0_xs256`: a
three-tooth comb whose lowest edge weaves around six edges of a fifteen-tooth comb), and 257 is the smallest count that leaves."""
import bisect
import math
from fractions import Fraction

import numpy as np

HOST_RTOL = 1.7e-13

# (ring vertices, slab boundaries, edges of one ring over one slab) of tiers 0..3 (cape_ring_area.h: Tier<>)
TIERS = ((32, 256, 6), (128, 1024, 16), (128, 1024, 32), (512, 2048, 32))
RESOURCES = ("ring", "slabs", "stack")  # the NaN codes 1, 2, 3
NAN_CODE = dict(ring=1, slabs=2, stack=3)
MIN_GAP = Fraction(1, 10**6)


# ---- the exact reference -------------------------------------------------------------------------------------------------------

def _edges(ring):
    """the non-vertical edges (r[i-1], r[i]) in ring order, left end first (edges_of)"""
    out = []
    for i in range(len(ring)):
        p, q = ring[i - 1], ring[i]
        if p[0] == q[0]:
            continue
        out.append((p, q) if p[0] < q[0] else (q, p))
    return out


def _crossing_abscissae(ea, eb):
    """the abscissa of every proper crossing of an edge of ea with an edge of eb (t and u strictly inside (0, 1), the edges not
    parallel), found with integer cross products"""
    if not ea or not eb:
        return []
    A = np.array(ea, np.int64).reshape(-1, 4)
    B = np.array(eb, np.int64).reshape(-1, 4)
    ax, ay, bx, by = (A[:, k][:, None] for k in range(4))
    cx, cy, dx, dy = (B[:, k][None, :] for k in range(4))
    d1x, d1y, d2x, d2y = bx - ax, by - ay, dx - cx, dy - cy
    den = d1x * d2y - d1y * d2x  # (coordinates below 2^20: every product below 2^43)
    tn = (cx - ax) * d2y - (cy - ay) * d2x
    un = (cx - ax) * d1y - (cy - ay) * d1x
    s = np.sign(den)
    hit = (den != 0) & (tn * s > 0) & (tn * s < den * s) & (un * s > 0) & (un * s < den * s)
    out = []
    for i, j in zip(*np.nonzero(hit)):
        out.append(int(A[i, 0]) + Fraction(int(tn[i, j]) * int(d1x[i, 0]), int(den[i, j])))
    return out


def _ring_pair(a, b):
    """rings a and b (integer vertices): the exact area of their intersection and what rings_inter_area needs for it"""
    ea, eb = _edges(a), _edges(b)
    xs = [Fraction(p[0]) for p in a] + [Fraction(p[0]) for p in b] + _crossing_abscissae(ea, eb)
    bounds = sorted(set(xs))
    gap = min((y - x for x, y in zip(bounds, bounds[1:])), default=None)
    slabs = [([], []) for _ in range(max(len(bounds) - 1, 0))]
    for side, es in enumerate((ea, eb)):
        for k, (p, q) in enumerate(es):
            for s in range(bisect.bisect_left(bounds, p[0]), bisect.bisect_left(bounds, q[0])):
                slabs[s][side].append(k)
    area, stack, terms = Fraction(0), 0, 0
    for s, both in enumerate(slabs):
        x0, x1 = bounds[s], bounds[s + 1]
        xm = (x0 + x1) / 2
        stack = max(stack, len(both[0]), len(both[1]))
        ys = []
        for side, es in enumerate((ea, eb)):
            ys.append(sorted((p[1] + (q[1] - p[1]) * (xm - p[0]) / (q[0] - p[0]), k) for k in both[side] for p, q in (es[k],)))
        n = 0
        for i in range(0, len(ys[0]) - 1, 2):
            for j in range(0, len(ys[1]) - 1, 2):
                lo, hi = max(ys[0][i][0], ys[1][j][0]), min(ys[0][i + 1][0], ys[1][j + 1][0])
                if hi > lo:  # (no two edges cross inside a slab: the height at its middle times its width is the trapezoid)
                    area += (hi - lo) * (x1 - x0)
                    n += 1
        terms = max(terms, n)
    return dict(area=area, boundaries=len(xs), distinct=len(bounds), stack=stack, terms=terms, gap=gap)


_analysed = {}


def _analyse(case):
    got = _analysed.get(case["name"])
    if got is None or got[0] is not case:
        got = (case, [_ring_pair(case["det"], ring) for ring in [case["outer"], *case["holes"]]])
        _analysed[case["name"]] = got
    return got[1]


def exact_inter_area(case):
    """area(detection n outer) - area(detection n hole_k) in order, never below 0 (polygons_inter_area), as a Fraction"""
    pairs = _analyse(case)
    acc = pairs[0]["area"]
    for p in pairs[1:]:
        acc -= p["area"]
    return max(acc, Fraction(0))


def demand(case):
    """ring: the longest ring; boundaries: na + nb + proper crossings (the count BEFORE std::unique, the one the kernel compares with
    its capacity), the largest over the map polygon's rings; stack: the most non-vertical edges of one ring over one slab; pairs:
    (boundaries, stack) per ring of the map polygon in the order the kernel takes them; distinct: the boundaries std::unique leaves
    for the outer ring; terms: the most trapezoids one slab adds"""
    pairs = _analyse(case)
    return dict(ring=max(len(case["det"]), len(case["outer"]), *(len(h) for h in case["holes"])), boundaries=max(p["boundaries"] for p in pairs),
                stack=max(p["stack"] for p in pairs), pairs=[(p["boundaries"], p["stack"]) for p in pairs], distinct=pairs[0]["distinct"],
                terms=max(p["terms"] for p in pairs))


def expected_walk(d):
    """(tiers visited, the tier that serves or None, the resource named by the NaN the pair keeps or None).  A tier checks the ring
    lengths first, then ring by ring the boundaries and then the edges over a slab; a pair leaves for the NEXT tier while some later
    tier is larger in the resource that ran out."""
    visited = []
    for t, caps in enumerate(TIERS):
        visited.append(t)
        why = None
        if d["ring"] > caps[0]:
            why = 0
        else:
            for boundaries, stack in d["pairs"]:
                if boundaries > caps[1]:
                    why = 1
                elif stack > caps[2]:
                    why = 2
                if why is not None:
                    break
        if why is None:
            return visited, t, None
        if not any(later[why] > caps[why] for later in TIERS[t + 1:]):
            return visited, None, RESOURCES[why]
    raise AssertionError("the last tier has no later one")


def tier_counts(cases):
    """pairs handed to tiers 1, 2 and 3 over the cases"""
    counts = [0, 0, 0]
    for c in cases:
        for t in expected_walk(demand(c))[0]:
            if t > 0:
                counts[t - 1] += 1
    return counts


def signed_area2(ring):
    """twice the signed area (exact: integers)"""
    return sum(ring[i - 1][0] * ring[i][1] - ring[i][0] * ring[i - 1][1] for i in range(len(ring)))


# ---- a case as the planes the matchers take ---------------------------------------------------------------------------------------

def depth_of(k):
    """planes of case k: 300 apart, three times the distance gate (100), so that the gate pairs case k with case k only"""
    return 1000.0 + 300.0 * k


def planes_of(case, depth):
    """(detected plane as tests/packing.make_shard and -- with its area appended -- cape_amd.host_match_map take it, map plane as
    cape_amd.pack_map takes it): the canonical frame at `depth` along the normal"""
    frame = ((0.0, 0.0, 1.0), -float(depth), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, float(depth)))
    as_array = lambda ring: np.array(ring, np.float64).reshape(-1, 2)
    return (*frame, as_array(case["det"])), (*frame, as_array(case["outer"]), [as_array(h) for h in case["holes"]])


# ---- the families ----------------------------------------------------------------------------------------------------------------

def rect(x0, y0, x1, y1):
    return [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]  # clockwise


def comb_right(T, L, H, ox=0, oy=0, skew=0, rise=0):
    """T slanted teeth pointing +x from the line x = ox: 2T edges over every slab of (ox, ox + L), 2T + 1 vertices.  The two end
    vertices sit at ox - 1, so that the (vertical, dropped) closing edge misses the inner ones; the tips at ox + L + skew k."""
    ring = []
    for k in range(T):
        ring.append((ox - (1 if k == 0 else 0), oy + k * H))
        ring.append((ox + L + skew * k, oy + k * H + H // 2 + rise))
    ring.append((ox - 1, oy + T * H))
    return ring[::-1]  # clockwise


def comb_up(T, P, H, ox=0, oy=0, extra=0):
    """T slanted teeth pointing +y from the line y = oy: two edges over a slab (a tooth's flank and the closing edge at oy - 1),
    2T + 1 vertices + `extra` collinear ones on the closing edge, each at an abscissa of its own"""
    ring = []
    for k in range(T):
        ring.append((ox + k * P, oy - (1 if k == 0 else 0)))
        ring.append((ox + k * P + P // 2, oy + H))
    ring.append((ox + T * P, oy - 1))
    ring += [(ox + T * P - 7 - 13 * k, oy - 1) for k in range(1, extra + 1)]
    return ring  # clockwise


def regular(n, R, cx, cy, phase=0.1):
    return [(cx + round(R * math.cos(phase - 2 * math.pi * k / n)), cy + round(R * math.sin(phase - 2 * math.pi * k / n))) for k in range(n)]  # clockwise


def mountain(m, step, ox, base, height, bump, mod):
    """m vertices, each at an abscissa of its own: a chain of m - 2 peaks left to right over a base edge; two edges over a slab"""
    chain = [(ox + step * i, height + bump * ((7 * i) % mod)) for i in range(m - 2)]
    return chain + [(chain[-1][0] + 5, base), (ox - 5, base)]  # clockwise


def weaving_comb(weaves, extras):
    """A three-tooth comb_right over comb_up(15, 2000, 6000) whose lowest edge (y = 600) weaves around the rising flank of teeth
    1..weaves -- two vertices and two more crossings each -- and carries `extras` further vertices: 7 + 2 weaves + extras vertices, six
    edges over a slab, 180 + 2 weaves crossings"""
    low = [(-501, 600)]
    for k in range(1, weaves + 1):
        low += [(2000 * k + 80, 400), (2000 * k + 120, 800)]  # the flank passes (2000 k + 100, 600) with slope 6
    low += [(2000 * (weaves + 1) + 1500 + 37 * i, 600) for i in range(extras)]
    ring = low + [(30500, 600), (-500, 1500), (30500, 2400), (-500, 3300), (30500, 4200), (-501, 5100)]
    return ring[::-1]  # clockwise


CASES = []
CELLS = {}  # required cell -> names of the cases that fill it


def _case(name, det, outer, holes=(), cells=(), zero=False):
    """zero: the rings share at most vertical or identical edges -- the host class must return exactly 0.0"""
    c = dict(name=name, det=[tuple(map(int, p)) for p in det], outer=[tuple(map(int, p)) for p in outer],
             holes=[[tuple(map(int, p)) for p in h] for h in holes], zero=zero)
    assert all(abs(v) < 2**20 for ring in [c["det"], c["outer"], *c["holes"]] for p in ring for v in p), name
    assert name not in {k["name"] for k in CASES}, name
    CASES.append(c)
    for cell in cells:
        CELLS.setdefault(cell, []).append(name)
    return c


def _flipped(case, cells=()):
    """the same pair with every ring in the other orientation"""
    return _case(case["name"] + "_flipped", case["det"][::-1], case["outer"][::-1], [h[::-1] for h in case["holes"]], cells, case["zero"])


def _seam(name, target, m_a, cells):
    """two mountains whose distinct boundaries number `target`: the second one inside the first (no crossing) or out of its right
    flank (two crossings), found by trying"""
    a = mountain(m_a, 20, 0, 0, 2000, 100, 5)
    for m_b in range(4, m_a + 1):
        for ox in (3, a[-3][0] - 10 * (m_b - 3) + 3):
            c = dict(name=name, det=a, outer=mountain(m_b, 10, ox, 50, 1000, 100, 4), holes=[])
            if _ring_pair(c["det"], c["outer"])["distinct"] == target:
                return _case(name, c["det"], c["outer"], cells=cells)
    raise AssertionError(f"no pair of mountains with {target} distinct boundaries")


def _build():
    small = regular(5, 60000, 260000, 230000, 0.3)
    # ring vertices
    for n in (32, 33, 128, 129, 512):
        _case(f"det{n}", regular(n, 100000, 200000, 200000), small, cells=[f"ring det {n}"])
        _case(f"map{n}", small, regular(n, 100000, 200000, 200000), cells=[f"ring map {n}"])
    _case("both512", regular(512, 100000, 200000, 200000), regular(512, 90000, 230000, 210000, 0.3), cells=["ring both 512"])
    _case("det513", regular(513, 100000, 200000, 200000), small, cells=["ring det 513", "no tier: ring"])
    # edges over one slab: a comb of T teeth against a rectangle across its teeth, the limit once in either ring
    for T in (3, 4, 8, 9, 16, 17):
        comb, across = comb_right(T, 4000, 200, skew=3), rect(1000, -50, 3000, T * 200 + 50)
        extra = ["bites"] if T in (3, 8) else []
        _case(f"stack{2 * T}_det", comb, across, cells=[f"stack det {2 * T}"] + extra + (["no tier: stack"] if T == 17 else []) +
              (["walk 1 -> 2 stack"] if T == 9 else []))
        _case(f"stack{2 * T}_map", across, comb, cells=[f"stack map {2 * T}"] + extra)
    # boundaries: two combs at right angles, 2 T_a x 2 T_b crossings, collinear vertices on the closing edge one boundary at a time
    _case("t0_xs256", weaving_comb(6, 13), comb_up(15, 2000, 6000, extra=1), cells=["slabs 256"])
    _case("t0_xs257", weaving_comb(7, 10), comb_up(15, 2000, 6000, extra=1), cells=["slabs 257"])
    wide8, wide16 = comb_right(8, 61000, 2000, -500, 1000, rise=500), comb_right(16, 61000, 2000, -500, 1000, rise=500)
    _case("xs1024", wide8, comb_up(29, 2000, 40000, extra=20), cells=["slabs 1024"])
    _case("xs1025", wide8, comb_up(29, 2000, 40000, extra=21), cells=["slabs 1025", "walk 2 -> 3 slabs"])
    _case("xs2048", comb_up(30, 2000, 40000, extra=34), wide16, cells=["slabs 2048"])
    _case("xs2049", comb_up(30, 2000, 40000, extra=35), wide16, cells=["slabs 2049", "no tier: slabs"])
    # two overflows at once.  Tier 0: slabs and stack, either way the pair leaves for tier 1.  Tier 2: boundaries beyond 1024 AND 34
    # edges over a slab -- the slab check comes first, so the pair goes on to tier 3 (a stack check first would keep it in tier 2)
    _case("two_overflows_t0", comb_right(4, 31000, 1200, -500, 600, rise=300), comb_up(15, 2000, 6000), cells=["two overflows tier 0"])
    _case("two_overflows_t2", comb_right(17, 31000, 1900, -500, 1000, rise=500), comb_up(15, 2000, 40000), cells=["two overflows tier 2"])
    # window seams: one slab short of, exactly at and one slab past a 64-slab window, on a lone wave and on four
    for target in (64, 65, 66):
        _seam(f"seam{target}_t0", target, 32, [f"seam {target} tier 0"])
    for target in (64, 65, 66, 128, 129, 130):
        _seam(f"seam{target}_t1", target, 40 if target < 100 else 100, [f"seam {target} tier 1"])
    # degenerate contact
    sq = rect(0, 0, 100, 100)
    contact = [
        _case("shared_vertical_edge", sq, rect(100, 0, 200, 100), cells=["shared vertical edge"], zero=True),
        _case("shared_slanted_edge", [(0, 0), (0, 100), (100, 150), (100, 50)], [(0, 0), (100, 50), (100, -80), (0, -80)],
              cells=["shared slanted edge"], zero=True),
        _case("one_vertex", sq, rect(100, 100, 180, 190), cells=["contact in one vertex"], zero=True),
        _case("vertex_on_edge_outside", sq, [(50, 100), (20, 180), (90, 170)], cells=["vertex on edge"], zero=True),
        _case("vertex_on_edge_inside", sq, [(50, 100), (90, 20), (20, 30)], cells=["vertex on edge"]),
        _case("inside", rect(-50, -60, 300, 200), [(10, 10), (30, 90), (95, 70), (60, 5)], cells=["one inside the other"]),
        _case("disjoint", sq, rect(150, 20, 260, 90), cells=["disjoint"], zero=True),
        _case("itself", regular(12, 500, 0, 0), regular(12, 500, 0, 0), cells=["a ring against itself"]),
        _case("one_abscissa", comb_right(3, 400, 60), [(-30, -10), (-30, 200), (300, 220), (310, -20)], cells=["many vertices on one abscissa"]),
        # the spike (100, 50) -> (200, 50) -> (100, 50): two edges of one ring at the same height over a slab
        _case("equal_heights", [(0, 0), (0, 100), (100, 100), (100, 50), (200, 50), (100, 50), (100, 0)], rect(50, 20, 180, 90),
              cells=["equal heights in a slab"]),
    ]
    hole = rect(400, 400, 600, 600)
    contact += [
        _case("hole_longer_than_outer", rect(300, 300, 700, 700), rect(0, 0, 1000, 1000), [regular(40, 150, 500, 500)], cells=["hole longer than outer"]),
        _case("hole_covered", rect(300, 300, 700, 700), rect(0, 0, 1000, 1000), [hole], cells=["hole covered fully"]),
        _case("hole_cut", rect(500, 300, 900, 700), rect(0, 0, 1000, 1000), [hole], cells=["hole covered partly"]),
        _case("hole_missed", rect(50, 50, 300, 300), rect(0, 0, 1000, 1000), [hole], cells=["hole not covered"]),
        _case("two_holes", [(100, 100), (150, 900), (950, 800), (700, 50)], rect(0, 0, 1000, 1000), [hole, [(700, 200), (850, 350), (900, 150)]]),
    ]
    for c in contact:
        _flipped(c, cells=["both orientations"])
    # a case that bites: more than two terms in one slab (the third and later ones travel through LDS in the ordered sum)
    _case("comb_in_comb_t0", comb_right(3, 4000, 200, skew=3), comb_right(3, 3500, 200, 7, 60, skew=5), cells=["bites"])
    _case("comb_in_comb_t1", comb_right(8, 4000, 200, skew=3), comb_right(7, 3500, 200, 7, 60, skew=5), cells=["bites"])


_build()
BY_NAME = {c["name"]: c for c in CASES}

REQUIRED_CELLS = (
    [f"ring det {n}" for n in (32, 33, 128, 129, 512, 513)] + [f"ring map {n}" for n in (32, 33, 128, 129, 512)] + ["ring both 512"] +
    [f"stack {side} {n}" for side in ("det", "map") for n in (6, 8, 16, 18, 32, 34)] + [f"slabs {n}" for n in (256, 257, 1024, 1025, 2048, 2049)] +
    ["two overflows tier 0", "two overflows tier 2", "walk 1 -> 2 stack", "walk 2 -> 3 slabs", "no tier: stack", "no tier: slabs", "no tier: ring"] +
    [f"seam {n} tier 0" for n in (64, 65, 66)] + [f"seam {n} tier 1" for n in (64, 65, 66, 128, 129, 130)] +
    ["shared vertical edge", "shared slanted edge", "contact in one vertex", "vertex on edge", "one inside the other", "disjoint", "a ring against itself",
     "many vertices on one abscissa", "equal heights in a slab", "hole longer than outer", "hole covered fully", "hole covered partly", "hole not covered",
     "both orientations", "bites"])


def check_cell(cell, case):
    """the assertion behind a required cell: the case's exact demands and expected walk put it there"""
    d = demand(case)
    visited, served, why = expected_walk(d)
    words = cell.split()
    if words[0] == "ring":
        n = int(words[2])
        sides = dict(det=[case["det"]], map=[case["outer"]], both=[case["det"], case["outer"]])[words[1]]
        assert all(len(r) == n for r in sides) and d["ring"] == n and d["stack"] <= 6 and d["boundaries"] <= 2048
        assert served == (None if n > 512 else 0 if n <= 32 else 1 if n <= 128 else 3) and visited == list(range((served if n <= 512 else 3) + 1))
    elif words[0] == "stack":
        n = int(words[2])
        own, other = (case["det"], case["outer"]) if words[1] == "det" else (case["outer"], case["det"])
        assert d["stack"] == n and _ring_pair(own, rect(-10**5, -10**5, 10**5, 10**5))["stack"] == n and len(other) == 4
        assert d["ring"] <= 128 and d["boundaries"] <= 256
        assert served == {6: 0, 8: 1, 16: 1, 18: 2, 32: 2, 34: None}[n]
        if n == 34:
            assert visited == [0, 1, 2] and why == "stack"  # tier 3 is not larger in that resource
    elif words[0] == "slabs":
        n = int(words[1])
        assert d["boundaries"] == n
        tier = 0 if n <= 257 else 1 if n <= 1025 else 3
        assert d["ring"] <= TIERS[tier][0] and d["stack"] <= TIERS[tier][2], "rings and stacks fit the tier"
        assert served == {256: 0, 257: 1, 1024: 1, 1025: 3, 2048: 3, 2049: None}[n]
    elif cell == "two overflows tier 0":
        assert d["ring"] <= 32 and d["boundaries"] > 256 and d["stack"] > 6 and served == 1
    elif cell == "two overflows tier 2":
        assert d["ring"] <= 128 and 1024 < d["boundaries"] <= 2048 and d["stack"] == 34 and (visited, served, why) == ([0, 1, 2, 3], None, "stack")
    elif cell == "walk 1 -> 2 stack":
        assert d["ring"] <= 128 and d["boundaries"] <= 1024 and 16 < d["stack"] <= 32 and (visited, served) == ([0, 1, 2], 2)
    elif cell == "walk 2 -> 3 slabs":
        assert d["ring"] <= 128 and d["stack"] <= 16 and 1024 < d["boundaries"] <= 2048 and (visited, served) == ([0, 1, 2, 3], 3)
    elif words[0] == "no":
        assert served is None and why == words[-1]
        assert visited == ([0, 1, 2] if why == "stack" else [0, 1, 2, 3])
    elif words[0] == "seam":
        assert d["distinct"] == int(words[1]) and served == int(words[3]) and d["stack"] == 2
    elif cell == "hole longer than outer":
        assert max(len(h) for h in case["holes"]) > 32 >= max(len(case["det"]), len(case["outer"])) and served == 1
    elif cell.startswith("hole "):
        whole, covered = abs(Fraction(signed_area2(case["holes"][0]), 2)), _analyse(case)[1]["area"]
        assert {"fully": covered == whole, "partly": 0 < covered < whole, "covered": covered == 0}[words[-1]]
    elif cell == "bites":
        assert d["terms"] > 2
    elif cell == "many vertices on one abscissa":
        assert d["boundaries"] - d["distinct"] >= 4
    elif cell == "equal heights in a slab":
        assert len(set(case["det"])) < len(case["det"])
    elif cell == "both orientations":
        twin = BY_NAME[case["name"][: -len("_flipped")]]
        assert signed_area2(twin["det"]) == -signed_area2(case["det"]) and signed_area2(twin["outer"]) == -signed_area2(case["outer"])
    elif cell in ("shared vertical edge", "shared slanted edge", "contact in one vertex", "disjoint"):
        assert case["zero"] and exact_inter_area(case) == 0
    elif cell == "a ring against itself":
        assert case["det"] == case["outer"] and exact_inter_area(case) * 2 == abs(signed_area2(case["det"]))
    elif cell == "one inside the other":
        assert exact_inter_area(case) * 2 == abs(signed_area2(case["outer"])) and d["boundaries"] == len(case["det"]) + len(case["outer"])
    else:
        assert cell == "vertex on edge", cell
        a, b = case["det"], case["outer"]
        assert any(p not in a and (q[0] - o[0]) * (p[1] - o[1]) == (q[1] - o[1]) * (p[0] - o[0]) and min(o, q) < p < max(o, q)
                   for p in b for o, q in zip(a, a[1:] + a[:1]))


# Rounding cannot merge two slabs, or part one, and so change a demand: distinct exact boundaries lie further apart than 1e-6 (a
# crossing's abscissa is off by a few ulps of 2^20: 1e-10).  A case with zero=True has an exact area of 0.
for _c in CASES:
    for _p in _analyse(_c):
        assert _p["gap"] is None or _p["gap"] > MIN_GAP, (_c["name"], float(_p["gap"]))
    assert not _c["zero"] or exact_inter_area(_c) == 0, _c["name"]
for _cell in REQUIRED_CELLS:
    assert CELLS.get(_cell), f"no case fills the cell `{_cell}`"
    for _name in CELLS[_cell]:
        check_cell(_cell, BY_NAME[_name])

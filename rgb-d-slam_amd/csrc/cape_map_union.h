// The polygon half of the map update for one matched pair (cape_map_union.hip, cape_debug_ring_union): the statements of
// Polygon::project, merge_union, rings_union_outer, drop_collinear, ring_is_simple, simplify, douglas_peucker and segment_distance2 of
// host/boundary_polygon.cpp in the host's order and with its early exits, on ONE wavefront.  Two pair functions:
//   union_pair               for a map polygon without holes whose union creates none (cape_map_union, cape_debug_ring_union);
//   union_pair_rings<Cuts>   for the modes with rings, one text: with add_hole, carry_hole's kept and covered cases, Polygon::area and
//       simplify over interior rings as well.  Cuts = false is the holes mode (cape_map_union_holes, cape_debug_polygon_union), where
//       a hole the detection covers in part stays the host's; Cuts = true the cut mode (cape_map_union_cut,
//       cape_debug_polygon_union_cut), which cuts such a hole into its pieces by a second arrangement inside the pair -- rule 1 of
//       union_arrange on (hole, detection).  `if constexpr (Cuts)` stands at the three places the two differ: that branch of the
//       carried-holes loop, the HOST_HOLE_CUT return, the HOLE_PIECES flag.
// Every per-lane and per-wave function stands once, and so do the steps that cost nothing to share: the placement of the operands
// (union_place_operands), the Douglas-Peucker loop (union_dp_candidate), union_orient with its sense, union_area on
// union_area_holed, union_hosted.  Everything of the modes with rings from the placement of the operands through step 6 stands once,
// in union_pair_rings.
// What still stands more than once, and why.  The arrangement (step 3 up to the last link), the start of the outer walk, the test of
// a walked face and union_left_out's loop stand in union_pair and in union_pair_rings, for a measured reason: shared as plain
// __forceinline__ functions they compute the same rows, but the optimiser simplifies a callee before it inlines it, the register
// allocation moves, and on an MI355X a call's median then left the spread of the restated build by 0.05 to 0.3 %
// (profiles/map_union_shared_steps.txt).  union_pair folded into the template as a third mode was tried and measured too
// (profiles/map_union_one_pair.txt): the plain frame kernel grows from 6 952 to 7 138 instructions, and cape_map_union's median
// leaves the parent's spread by 0.9 to 1.4 % in three of its four timed settings, so union_pair stays.  The arrangement with the face
// test also stands in union_arrange, which union_pair_rings<true> calls for the second arrangement only (rule 1; its rule 0 is the
// first arrangement and is kept for the one-lane port, which runs both): the first arrangement of union_pair_rings is the inline
// one in both modes, which is what keeps the holes kernels the parent's instructions.  So the arrangement stands in three places
// on the device (union_pair, union_pair_rings, union_arrange) and once in the ports (seq::Arrangement); the evidence for the one pair function of the modes with rings -- the holes kernels are the
// parent's instructions, the cut call's median lies inside the parent's spread -- is in profiles/map_union_one_pair.txt.
//
// Two parts.  The first holds the plain per-lane functions (projection, cut parameters, crossing points, the angle of the face walk
// with its guard band, the collinear test, the Douglas-Peucker distance, the bounding-box test in front of a hole's intersection): they
// need nothing of the wave and compile for the host too (tests/host/map_union_algebra.cpp and map_union_holes_algebra.cpp compare them
// and one-lane ports of the modes, map_union_cut_algebra.cpp the cut mode's, with the host class under the sanitizers).  The second,
// under __HIPCC__, is the
// wave's part: the LDS carve, node_of's search (ballot, lowest set lane), the walks, the point tests, ring_is_simple and the
// Douglas-Peucker loop.  What the host orders is uniform control flow: node numbering, the walks, drop_collinear's erase loop.
//
// segments_intersect, ring_is_simple and the Douglas-Peucker loop are restated here rather than shared with cape_polygon.hip: that
// file walks rings of indices into a point array, this one rings of coordinates, and cape_polygon.o stays byte for byte what it was.
//
// Vertex coordinates are + - x / only (-ffp-contract=off), so a served ring is the host's bit for bit.  sqrt (param_on), hypot
// (drop_collinear, the probe) and atan2 (next_of) feed comparisons only; the angles carry a guard band of 1e-10 rad that hands the
// pair to the host (CAPE_UNION_HOST_AMBIGUOUS; union_angle says which comparisons are exact on both sides and exempt); a hypot
// threshold tie has no guard.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cape_hip.h"

namespace cape {

namespace {

constexpr int kUnionRing = CAPE_MAP_UNION_MAX_RING;   // vertices of an operand
constexpr int kUnionNodes = CAPE_MAP_UNION_MAX_NODES; // nodes of the arrangement
constexpr int kUnionDegree = 8;                       // neighbours of a node
constexpr int kUnionCuts = 1024;                      // cuts of all segments (each crossing cuts two segments)
constexpr int kUnionOut = CAPE_MAP_MAX_RING;          // vertices of a walked face; the closed ring of simplify takes one more
constexpr double kUnionAngleBand = 1e-10;             // rad: the guard band of the face walk's angle comparisons
constexpr double kUnionTwoPi = 2 * 3.14159265358979323846;

struct UnionFrame
{
    double x[3], y[3], c[3];
};

__device__ __forceinline__ double umin(double a, double b) { return (b < a) ? b : a; } // std::min
__device__ __forceinline__ double umax(double a, double b) { return (a < b) ? b : a; } // std::max
__device__ __forceinline__ double ucross2(const double2& o, const double2& a, const double2& b)
{
    return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x);
}
__device__ __forceinline__ bool usame(const double2& a, const double2& b, double eps) { return fabs(a.x - b.x) <= eps && fabs(a.y - b.y) <= eps; }

// Eigen's isApprox on 3-vectors (host/polygon_capi.cpp: is_approx3)
__device__ __forceinline__ bool union_is_approx3(const double* a, const double* b)
{
    const double e0 = a[0] - b[0], e1 = a[1] - b[1], e2 = a[2] - b[2];
    const double diff = (e0 * e0 + e1 * e1) + e2 * e2;
    const double na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], nb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const double prec = 1e-12;
    return diff <= prec * prec * umin(na, nb);
}

// get_projected_plan_coordinates(get_point_from_plane_coordinates(p, from), to): one vertex of Polygon::project
__device__ __forceinline__ double2 union_project(const double2& p, const UnionFrame& from, const UnionFrame& to)
{
    const double q0 = from.c[0] + p.x * from.x[0] + p.y * from.y[0];
    const double q1 = from.c[1] + p.x * from.x[1] + p.y * from.y[1];
    const double q2 = from.c[2] + p.x * from.x[2] + p.y * from.y[2];
    const double d0 = q0 - to.c[0], d1 = q1 - to.c[1], d2 = q2 - to.c[2];
    return make_double2((to.x[0] * d0 + to.x[1] * d1) + to.x[2] * d2, (to.y[0] * d0 + to.y[1] * d1) + to.y[2] * d2);
}

// param_on of rings_union_outer: is p on the segment (a, b) within eps, strictly between its ends?  t = its position
__device__ __forceinline__ bool union_param_on(const double2& a, const double2& b, const double2& p, double eps, double& t)
{
    const double dx = b.x - a.x, dy = b.y - a.y;
    const double len2 = dx * dx + dy * dy;
    const double c = ucross2(a, b, p);
    if (fabs(c) > eps * sqrt(len2))
        return false;
    t = ((p.x - a.x) * dx + (p.y - a.y) * dy) / len2;
    return t > 0 && t < 1 && !usame(p, a, eps) && !usame(p, b, eps);
}

// the proper crossing of (sa, sb) and (ua, ub): the two cut parameters, and whether each is kept (the crossing point is not within
// eps of an end of its segment).  False without a proper crossing.
__device__ __forceinline__ bool union_crossing(const double2& sa, const double2& sb, const double2& ua, const double2& ub, double eps, double& ts,
                                               bool& keepS, double& tu, bool& keepU)
{
    const double d1 = ucross2(ua, ub, sa), d2 = ucross2(ua, ub, sb);
    const double d3 = ucross2(sa, sb, ua), d4 = ucross2(sa, sb, ub);
    if (!(((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0))))
        return false;
    ts = d1 / (d1 - d2);
    tu = d3 / (d3 - d4);
    const double2 x = make_double2(sa.x + ts * (sb.x - sa.x), sa.y + ts * (sb.y - sa.y));
    keepS = !usame(x, sa, eps) && !usame(x, sb, eps);
    keepU = !usame(x, ua, eps) && !usame(x, ub, eps);
    return true;
}

// the point of a cut: a + t (b - a)
__device__ __forceinline__ double2 union_cut_point(const double2& a, const double2& b, double t)
{
    return make_double2(a.x + t * (b.x - a.x), a.y + t * (b.y - a.y));
}

// One candidate of next_of: the counter-clockwise angle from the direction `ba` (an atan2) to the neighbour at (dx, dy), wrapped into
// (1e-12, 2 pi + 1e-12] like the host's while loop.  `ambiguous` is set when the unwrapped angle lies within the guard band of the
// wrap line, unless the candidate is `exact`: the node the walk came from (its direction IS `back`, the same atan2 of the same bits
// twice), or a candidate whose direction and `back` are both axis-parallel (union_axis_parallel: every atan2 involved is one of
// +-0, +-pi/2, +-pi by the C and OpenCL standards alike -- the vertical edge above the start node is the everyday case).
__device__ __forceinline__ bool union_axis_parallel(double dx, double dy, double bx, double by) { return (dx == 0 || dy == 0) && (bx == 0 || by == 0); }
__device__ __forceinline__ double union_angle(double dy, double dx, double ba, bool cameFrom, bool& ambiguous)
{
    double ang = atan2(dy, dx) - ba;
    for (int turn = 0; turn < 3 && ang <= 1e-12; ++turn) // (the angle starts above -2 pi - 1e-12: two turns at most)
    {
        if (!cameFrom && fabs(ang - 1e-12) < kUnionAngleBand)
            ambiguous = true;
        ang += kUnionTwoPi;
    }
    if (!cameFrom && fabs(ang - 1e-12) < kUnionAngleBand)
        ambiguous = true;
    return ang;
}

// drop_collinear's test: b lies on the segment joining its neighbours a and c
__device__ __forceinline__ bool union_collinear(const double2& a, const double2& b, const double2& c)
{
    const double cr = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
    const double len = hypot(c.x - a.x, c.y - a.y);
    return fabs(cr) <= 1e-9 * umax(1.0, len * len);
}

// segments_intersect: proper or touching intersection of the open segments; shared endpoints do not count
__device__ __forceinline__ bool union_segments_intersect(const double2& a1, const double2& a2, const double2& b1, const double2& b2)
{
    if (umax(a1.x, a2.x) < umin(b1.x, b2.x) || umax(b1.x, b2.x) < umin(a1.x, a2.x) || umax(a1.y, a2.y) < umin(b1.y, b2.y) ||
        umax(b1.y, b2.y) < umin(a1.y, a2.y))
        return false;
    if ((a1.x == b1.x && a1.y == b1.y) || (a1.x == b2.x && a1.y == b2.y) || (a2.x == b1.x && a2.y == b1.y) || (a2.x == b2.x && a2.y == b2.y))
        return false;
    const double d1 = ucross2(b1, b2, a1), d2 = ucross2(b1, b2, a2), d3 = ucross2(a1, a2, b1), d4 = ucross2(a1, a2, b2);
    if (((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0)))
        return true;
    if (d1 == 0 && umin(b1.x, b2.x) <= a1.x && a1.x <= umax(b1.x, b2.x) && umin(b1.y, b2.y) <= a1.y && a1.y <= umax(b1.y, b2.y))
        return true;
    if (d2 == 0 && umin(b1.x, b2.x) <= a2.x && a2.x <= umax(b1.x, b2.x) && umin(b1.y, b2.y) <= a2.y && a2.y <= umax(b1.y, b2.y))
        return true;
    if (d3 == 0 && umin(a1.x, a2.x) <= b1.x && b1.x <= umax(a1.x, a2.x) && umin(a1.y, a2.y) <= b1.y && b1.y <= umax(a1.y, a2.y))
        return true;
    if (d4 == 0 && umin(a1.x, a2.x) <= b2.x && b2.x <= umax(a1.x, a2.x) && umin(a1.y, a2.y) <= b2.y && b2.y <= umax(a1.y, a2.y))
        return true;
    return false;
}

// segment_distance2: Boost's projected_point strategy in its comparable form, the measure of its Douglas-Peucker
__device__ __forceinline__ double union_segment_distance2(const double2& p, const double2& a, const double2& b)
{
    const double vx = b.x - a.x, vy = b.y - a.y, wx = p.x - a.x, wy = p.y - a.y;
    const double c1 = wx * vx + wy * vy;
    if (c1 <= 0)
        return wx * wx + wy * wy;
    const double c2 = vx * vx + vy * vy;
    if (c2 <= c1)
    {
        const double ux = p.x - b.x, uy = p.y - b.y;
        return ux * ux + uy * uy;
    }
    const double t = c1 / c2;
    const double qx = a.x + t * vx, qy = a.y + t * vy;
    return (p.x - qx) * (p.x - qx) + (p.y - qy) * (p.y - qy);
}

// one edge (a = ring[i], b = ring[i - 1]) of point_in_ring: 2 = p lies on the edge, 1 = the ray towards +x crosses it, 0 = neither
__device__ __forceinline__ int union_point_edge(const double2& p, const double2& a, const double2& b)
{
    if (ucross2(a, b, p) == 0 && umin(a.x, b.x) <= p.x && p.x <= umax(a.x, b.x) && umin(a.y, b.y) <= p.y && p.y <= umax(a.y, b.y))
        return 2;
    if (((a.y > p.y) != (b.y > p.y)) && (p.x < (b.x - a.x) * (p.y - a.y) / (b.y - a.y) + a.x))
        return 1;
    return 0;
}

// is p inside or on ring[0, n)?  One lane walks the whole ring: simplify's check of an interior ring's candidate against the
// candidate outer ring (point_in_ring, closed)
__device__ __forceinline__ bool union_point_in_or_on(const double2& p, const double2* ring, int n)
{
    bool on = false, inside = false;
    for (int i = 0; i < n && !on; ++i)
    {
        const int e = union_point_edge(p, ring[i], ring[i == 0 ? n - 1 : i - 1]);
        on = e == 2;
        inside = inside != (e == 1);
    }
    return on || inside;
}

// are the bounding boxes of a[0, na) and b[0, nb) apart?  Then no slab of rings_inter_area holds an overlap and its sum is an empty
// one: + 0.0 on the host too.
__device__ __forceinline__ bool union_boxes_apart(const double2* a, int na, const double2* b, int nb)
{
    double ax0 = a[0].x, ax1 = a[0].x, ay0 = a[0].y, ay1 = a[0].y, bx0 = b[0].x, bx1 = b[0].x, by0 = b[0].y, by1 = b[0].y;
    for (int v = 1; v < na; ++v)
        ax0 = umin(ax0, a[v].x), ax1 = umax(ax1, a[v].x), ay0 = umin(ay0, a[v].y), ay1 = umax(ay1, a[v].y);
    for (int v = 1; v < nb; ++v)
        bx0 = umin(bx0, b[v].x), bx1 = umax(bx1, b[v].x), by0 = umin(by0, b[v].y), by1 = umax(by1, b[v].y);
    return ax1 < bx0 || bx1 < ax0 || ay1 < by0 || by1 < ay0;
}

} // namespace

} // namespace cape

#ifdef __HIPCC__
#include "cape_layout.h"
#include "cape_ring_area.h" // CAPE_MP_SYNC, ring_area_signed (the ordered sum)
#include "cape_wave.h"

namespace cape {

namespace {

// ---- the wave's carve: both operands, the segment and cut lists, the arrangement, two walked rings and simplify's arrays
struct UnionLdsLayout
{
    size_t ringA, ringB, segs, cutT, cutSeg, sortT, sortSeg, nodes, adj, deg, seen, outer, face, keep, stack, bytes;
};
constexpr int kUnionStack = kUnionOut + 8;
__host__ __device__ constexpr UnionLdsLayout union_layout()
{
    Layout l;
    UnionLdsLayout o{};
    o.ringA = l.take<double2>(kUnionRing + 1, 16); // (+ 1: simplify closes a ring onto its vertex 0)
    o.ringB = l.take<double2>(kUnionRing, 16);
    o.segs = l.take<unsigned short>(2 * kUnionRing); // bit 8: ring B; low bits: the first vertex of the segment
    o.cutT = l.take<double>(kUnionCuts);
    o.cutSeg = l.take<unsigned short>(kUnionCuts);
    o.nodes = l.take<double2>(kUnionNodes, 16);
    o.adj = l.take<unsigned short>((size_t)kUnionNodes * kUnionDegree);
    o.deg = l.take<unsigned char>(kUnionNodes);
    o.seen = l.take<unsigned char>(kUnionNodes); // bit k: the directed edge to neighbour k has been walked
    o.outer = l.take<double2>(kUnionOut + 1, 16);
    const size_t outerEnd = l.off;
    o.face = l.take<double2>(kUnionOut + 1, 16);
    const size_t faceEnd = l.off;
    // the sorted cuts live where the walked rings will: they are consumed by the node numbering, before the first walk
    o.sortT = l.alias<double>(o.outer, kUnionCuts, outerEnd);
    o.sortSeg = l.alias<unsigned short>(o.face, kUnionCuts, faceEnd);
    o.keep = l.take<unsigned char>(kUnionOut + 1);
    o.stack = l.take<unsigned>(kUnionStack);
    o.bytes = l.end(16);
    return o;
}
static_assert(kUnionCuts * sizeof(double) <= (kUnionOut + 1) * sizeof(double2), "the sorted cuts fit the outer ring's place");
static_assert(union_layout().bytes <= 64 * 1024, "one wave's carve fits the default LDS limit of a workgroup");
static_assert(kUnionRing <= 256 && kUnionNodes <= 65535 && kUnionDegree <= 8 && kUnionOut < 65536, "the packed indices");

struct UnionLds
{
    double2 *ringA, *ringB, *nodes, *outer, *face;
    unsigned short *segs, *cutSeg, *sortSeg, *adj;
    double *cutT, *sortT;
    unsigned char *deg, *seen, *keep;
    unsigned* stack;
};
__device__ __forceinline__ UnionLds union_carve(unsigned char* smem)
{
    constexpr UnionLdsLayout o = union_layout();
    UnionLds L;
    L.ringA = carve_at<double2>(smem, o.ringA);
    L.ringB = carve_at<double2>(smem, o.ringB);
    L.segs = carve_at<unsigned short>(smem, o.segs);
    L.cutT = carve_at<double>(smem, o.cutT);
    L.cutSeg = carve_at<unsigned short>(smem, o.cutSeg);
    L.sortT = carve_at<double>(smem, o.sortT);
    L.sortSeg = carve_at<unsigned short>(smem, o.sortSeg);
    L.nodes = carve_at<double2>(smem, o.nodes);
    L.adj = carve_at<unsigned short>(smem, o.adj);
    L.deg = carve_at<unsigned char>(smem, o.deg);
    L.seen = carve_at<unsigned char>(smem, o.seen);
    L.outer = carve_at<double2>(smem, o.outer);
    L.face = carve_at<double2>(smem, o.face);
    L.keep = carve_at<unsigned char>(smem, o.keep);
    L.stack = carve_at<unsigned>(smem, o.stack);
    return L;
}

// ---- the carve of the holes mode (cape_map_union_holes, cape_debug_polygon_union): the carve above, the interior rings of the merged
// polygon behind it, and the arrays of rings_inter_area (MpLds of cape_ring_area.h) for a hole against the detection.  The
// intersection runs after the face walks, so most of its arrays borrow what is dead by then: the cut lists, the nodes and the
// adjacency (`low`: cutT up to the outer ring) and the walked face (`face`).  Its tier: rings of kUnionRing vertices, 1024 slab
// boundaries, 16 edges of a ring over one slab (Tier<1>'s figures) -- what the borrowed regions and an LDS share of half a CU hold.
// simplify's candidates of the interior rings borrow the intersection's heights (`by`), dead once the last hole has been judged, and
// the ring it closes the nodes and the adjacency.
constexpr int kUnionHoleVertices = CAPE_MAP_UNION_HOLE_VERTICES; // interior rings of the merged polygon before simplify, in sum
constexpr int kUnionHoles = CAPE_MAP_MAX_HOLES;
constexpr int kUnionMpXs = 1024, kUnionMpStack = 16;
struct UnionHolesLdsLayout
{
    size_t holes, holeLen, candLen, srcOff, srcLen, ea, eb, xs, terms, elo, ehi, bk, inc, by, pre, cnt, sidx, sh, cand, closed, bytes;
};
__host__ __device__ constexpr UnionHolesLdsLayout union_holes_layout()
{
    constexpr UnionLdsLayout u = union_layout();
    UnionHolesLdsLayout o{};
    Layout low; // [cutT, outer)
    low.off = u.cutT;
    o.ea = low.take<Edge>(kUnionRing, 16);
    o.eb = low.take<Edge>(kUnionRing, 16);
    o.xs = low.take<double>(kUnionMpXs);
    o.terms = low.take<double>(64 * kUnionMpStack);
    o.elo = low.take<int>(2 * kUnionRing);
    o.ehi = low.take<int>(2 * kUnionRing);
    CAPE_LAYOUT_CHECK(low.off <= u.outer);
    // simplify closes an interior ring onto its vertex 0 in the place of the nodes and the adjacency (a face of kUnionOut vertices)
    o.closed = low.alias<double2>(u.nodes, kUnionOut + 1, u.deg);
    Layout face; // [face, keep)
    face.off = u.face;
    o.bk = face.take<unsigned short>(128 * kUnionMpStack);
    o.inc = face.take<unsigned short>(128 * kUnionMpStack);
    CAPE_LAYOUT_CHECK(face.off <= u.keep);
    Layout l;
    l.off = u.bytes;
    o.holes = l.take<double2>(kUnionHoleVertices, 16);
    o.by = l.take<double>(128 * kUnionMpStack, 16);
    const size_t byEnd = l.off;
    o.cand = l.alias<double2>(o.by, kUnionHoleVertices, byEnd);
    o.pre = l.take<int>(2 * kUnionRing + 2);
    o.cnt = l.take<int>(128);
    o.sh = l.take<int>(8, 16);
    o.srcOff = l.take<unsigned>(kUnionHoles);
    o.sidx = l.take<unsigned char>(128 * kUnionMpStack);
    o.holeLen = l.take<unsigned short>(kUnionHoles);
    o.candLen = l.take<unsigned short>(kUnionHoles);
    o.srcLen = l.take<unsigned short>(kUnionHoles);
    o.bytes = l.end(16);
    return o;
}
static_assert(union_layout().cutT % 16 == 0, "the borrowed edges are 16-byte aligned");
static_assert(2 * union_holes_layout().bytes <= 160 * 1024, "two waves' carves fit the LDS of a CU");
static_assert(kUnionHoleVertices * sizeof(double2) <= 128 * kUnionMpStack * sizeof(double), "the candidates fit the heights' place");

struct UnionHolesLds
{
    double2 *holes, *cand;                // the interior rings back to back; simplify's candidates of them, at the same offsets
    double2* closed;                      // kUnionOut + 1: the interior ring simplify is closing
    unsigned short *holeLen, *candLen;    // kUnionHoles lengths each
    unsigned* srcOff;                     // the map plane's interior rings: offsets into `src`, lengths (3 .. kUnionRing, checked)
    unsigned short* srcLen;
    const double2* src;
    int nSrc;
    MpLds mp;
};
__device__ __forceinline__ UnionHolesLds union_holes_carve(unsigned char* smem, const UnionLds& L)
{
    constexpr UnionHolesLdsLayout o = union_holes_layout();
    UnionHolesLds H;
    H.holes = carve_at<double2>(smem, o.holes);
    H.cand = carve_at<double2>(smem, o.cand);
    H.closed = carve_at<double2>(smem, o.closed);
    H.holeLen = carve_at<unsigned short>(smem, o.holeLen);
    H.candLen = carve_at<unsigned short>(smem, o.candLen);
    H.srcOff = carve_at<unsigned>(smem, o.srcOff);
    H.srcLen = carve_at<unsigned short>(smem, o.srcLen);
    H.src = nullptr;
    H.nSrc = 0;
    H.mp.ringCap = kUnionRing;
    H.mp.ringA = L.ringA; // a hole of the map plane
    H.mp.ringB = L.ringB; // the detection's ring
    H.mp.ea = carve_at<Edge>(smem, o.ea);
    H.mp.eb = carve_at<Edge>(smem, o.eb);
    H.mp.xs = carve_at<double>(smem, o.xs);
    H.mp.terms = carve_at<double>(smem, o.terms);
    H.mp.by = carve_at<double>(smem, o.by);
    H.mp.elo = carve_at<int>(smem, o.elo);
    H.mp.ehi = carve_at<int>(smem, o.ehi);
    H.mp.pre = carve_at<int>(smem, o.pre);
    H.mp.cnt = carve_at<int>(smem, o.cnt);
    H.mp.bk = carve_at<unsigned short>(smem, o.bk);
    H.mp.inc = carve_at<unsigned short>(smem, o.inc);
    H.mp.sidx = carve_at<unsigned char>(smem, o.sidx);
    H.mp.sh = carve_at<int>(smem, o.sh);
    return H;
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the orientation the host class gives an outer ring: reversed when its signed area is positive (every lane reads the whole ring
// before any lane rewrites it)
__device__ __forceinline__ void union_orient(double2* ring, int n, int lane, bool hole = false)
{
    const double s = ring_area_signed(ring, n);
    CAPE_MP_SYNC();
    if (hole ? s < 0 : s > 0)
    {
        for (int v = lane; v < n / 2; v += 64)
        {
            const double2 a = ring[v], b = ring[n - 1 - v];
            ring[v] = b;
            ring[n - 1 - v] = a;
        }
        CAPE_MP_SYNC();
    }
}

// Polygon::area: the outer ring minus the interior rings in order, clamped at 0
__device__ __forceinline__ double union_area_holed(const double2* ring, int n, const double2* holes, const unsigned short* len, int nHoles)
{
    if (n < 3)
        return 0.0;
    double a = fabs(ring_area_signed(ring, n));
    for (int k = 0, at = 0; k < nHoles; ++k)
    {
        const int nk = uni(len[k]);
        a -= fabs(ring_area_signed(holes + at, nk));
        at += nk;
    }
    return a < 0 ? 0.0 : a;
}

__device__ __forceinline__ double union_area(const double2* ring, int n) { return union_area_holed(ring, n, nullptr, nullptr, 0); }

// point_in_ring: crossing number, points on the boundary count as inside when `closed`.  Lanes over the edges.
__device__ __forceinline__ bool union_point_in_ring(const double2& p, const double2* ring, int n, bool closed, int lane)
{
    bool on = false, inside = false;
    for (int i = lane; i < n; i += 64)
    {
        const int e = union_point_edge(p, ring[i], ring[i == 0 ? n - 1 : i - 1]);
        on = on || e == 2;
        inside = inside != (e == 1);
    }
    if (__any(on))
        return closed;
    return (__popcll(__ballot(inside)) & 1) != 0;
}

// is every vertex of q[0, nq) outside ring[0, n) (not inside, not on it)?  Lanes over the vertices, each walks the whole ring.
__device__ __forceinline__ bool union_left_out(const double2* q, int nq, const double2* ring, int n, int lane)
{
    bool in = false;
    for (int v = lane; v < nq; v += 64)
    {
        const double2 p = q[v];
        bool on = false, inside = false;
        for (int i = 0; i < n && !on; ++i)
        {
            const int e = union_point_edge(p, ring[i], ring[i == 0 ? n - 1 : i - 1]);
            on = e == 2;
            inside = inside != (e == 1);
        }
        in = in || on || inside;
    }
    return !__any(in);
}

// ring_is_simple: no two non-adjacent edges touch, and the area is not zero.  Lanes over the first edge of a pair.
__device__ __forceinline__ bool union_ring_is_simple(const double2* r, int n, int lane)
{
    if (n < 3)
        return false;
    bool bad = false;
    for (int base = 0, round = 0; base < n; base += 64, ++round)
    {
        const int i = base + ((round & 1) ? 63 - lane : lane);
        if (i >= n)
            continue;
        const double2 a1 = r[i], a2 = r[i + 1 == n ? 0 : i + 1];
        for (int j = i + 1; j < n && !bad; ++j)
        {
            if (j == i + 1 || (i == 0 && j == n - 1))
                continue; // adjacent edges share a vertex
            bad = union_segments_intersect(a1, a2, r[j], r[j + 1 == n ? 0 : j + 1]);
        }
    }
    if (__any(bad))
        return false;
    return fabs(ring_area_signed(r, n)) > 0;
}

// drop_collinear: vertices on the segment joining their neighbours go, one at a time in ring order, until a pass changes nothing.
// Uniform: every lane runs the test, the erase shifts the tail down 64 vertices at a time.  Returns the new length.
__device__ __forceinline__ int union_drop_collinear(double2* r, int n, int lane)
{
    bool changed = true;
    while (changed && n > 3)
    {
        changed = false;
        for (int i = 0; i < n && n > 3; ++i)
        {
            const double2 a = r[i == 0 ? n - 1 : i - 1], b = r[i], c = r[i + 1 == n ? 0 : i + 1];
            if (union_collinear(a, b, c))
            {
                for (int base = i; base + 1 < n; base += 64)
                {
                    const int k = base + lane;
                    double2 v = make_double2(0.0, 0.0);
                    if (k + 1 < n)
                        v = r[k + 1];
                    CAPE_MP_SYNC();
                    if (k + 1 < n)
                        r[k] = v;
                    CAPE_MP_SYNC();
                }
                --n;
                changed = true;
                --i;
            }
        }
    }
    return n;
}

__device__ __forceinline__ int union_dp_candidate(const UnionLds& L, double2* ring, int n, double2* cand, double eps, int lane)
{
    if (lane == 0)
        ring[n] = ring[0]; // closed onto vertex 0
    for (int i = lane; i <= n; i += 64)
        L.keep[i] = (i == 0 || i == n) ? 1 : 0;
    if (lane == 0)
        L.stack[0] = (unsigned)n; // (a << 16) | b with a = 0
    int sp = 1;
    CAPE_MP_SYNC();
    while (sp > 0)
    {
        const unsigned ab = L.stack[--sp];
        const int a = uni((int)(ab >> 16)), b = uni((int)(ab & 0xFFFFu));
        if (b <= a + 1 || b > n)
            continue;
        const double2 pa = ring[a], pb = ring[b];
        unsigned long long best = 0ull; // squared distance bits (>= +0); the first index wins a tie, like the host's strict >
        int bestI = 0x7FFFFFFF;
        for (int i = a + 1 + lane; i < b; i += 64)
        {
            const double d = union_segment_distance2(ring[i], pa, pb);
            const unsigned long long db = (unsigned long long)__double_as_longlong(d);
            if (bestI == 0x7FFFFFFF || db > best)
            {
                best = db;
                bestI = i;
            }
        }
        const unsigned long long mx = ~wave_min_u64(~best);
        const unsigned mineKey = (bestI != 0x7FFFFFFF && best == mx) ? (unsigned)(0x7FFFFFFF - bestI) : 0u;
        const int idx = 0x7FFFFFFF - (int)wave_max_u32(mineKey);
        const double dmax = __longlong_as_double((long long)mx);
        if (dmax > eps * eps && idx > a && idx < b && sp + 2 <= kUnionStack)
        {
            if (lane == 0)
            {
                L.keep[idx] = 1;
                L.stack[sp] = ((unsigned)a << 16) | (unsigned)idx;
                L.stack[sp + 1] = ((unsigned)idx << 16) | (unsigned)b;
            }
            sp += 2;
            CAPE_MP_SYNC();
        }
    }
    int cn = 0;
    for (int base = 0; base < n; base += 64)
    {
        const int i = base + lane;
        const bool k = i < n && L.keep[i];
        const unsigned long long kb = __ballot(k);
        if (k)
            cand[cn + __popcll(kb & ((1ull << lane) - 1ull))] = ring[i];
        cn += __popcll(kb);
    }
    CAPE_MP_SYNC();
    return cn;
}

// Polygon::simplify of a polygon without holes: ring[0, n) (room for n + 1) becomes the Douglas-Peucker candidate if that is a
// simple ring of more than 75 % of the area; `cand` takes the candidate (room for n).  Returns the new length; area in / out.
__device__ __forceinline__ int union_simplify(const UnionLds& L, double2* ring, int n, double2* cand, double& area, int lane)
{
    area = union_area(ring, n);
    if (n < 4 || n > kUnionOut)
        return n;
    const double eps = umax(area / 1e5, 10.0);
    const int cn = union_dp_candidate(L, ring, n, cand, eps, lane);
    if (cn >= 3 && union_ring_is_simple(cand, cn, lane))
    {
        const double newArea = union_area(cand, cn);
        if (newArea > area * 0.75)
        {
            CAPE_MP_SYNC();
            for (int i = lane; i < cn; i += 64)
                ring[i] = cand[i];
            CAPE_MP_SYNC();
            area = newArea;
            return cn;
        }
    }
    return n;
}

// ---- interior rings (the holes mode)
// The Douglas-Peucker candidate (the loop of union_simplify above, for any ring) of the closed ring ring[0, n) (room for n + 1: the ring is closed onto its vertex 0) for the
// tolerance eps, into cand (room for n).  4 <= n <= kUnionOut.  Returns its length.
// does every vertex of q[0, nq) lie inside or on ring[0, n)?  Lanes over the vertices, each walks the whole ring.
__device__ __forceinline__ bool union_all_inside(const double2* q, int nq, const double2* ring, int n, int lane)
{
    bool out = false;
    for (int v = lane; v < nq; v += 64)
        out = out || !union_point_in_or_on(q[v], ring, n);
    return !__any(out);
}

// Polygon::simplify of a polygon with nHoles interior rings in H.holes: the Douglas-Peucker candidates of the outer ring (into
// `cand`, room for n) and of every interior ring of at least 4 vertices (into H.cand; H.closed takes the ring being closed); all
// rings are replaced or none.  Returns the outer ring's new length; H.holeLen follows; area in / out.
__device__ __forceinline__ int union_simplify_holed(const UnionLds& L, const UnionHolesLds& H, double2* ring, int n, int nHoles, double2* cand,
                                                    double& area, int lane)
{
    double2* closed = H.closed;
    area = union_area_holed(ring, n, H.holes, H.holeLen, nHoles); // the total area: eps and the 75 % rule are taken from it
    if (n < 4 || n > kUnionOut)
        return n;
    const double eps = umax(area / 1e5, 10.0);
    const int cn = union_dp_candidate(L, ring, n, cand, eps, lane);
    bool valid = cn >= 3 && union_ring_is_simple(cand, cn, lane);
    for (int k = 0, at = 0; valid && k < nHoles; ++k)
    {
        const int nk = uni(H.holeLen[k]);
        int ck = nk;
        if (nk < 4) // a triangle has nothing to drop: the candidate keeps it, and nothing is checked
        {
            for (int v = lane; v < nk; v += 64)
                H.cand[at + v] = H.holes[at + v];
            CAPE_MP_SYNC();
        }
        else
        {
            for (int v = lane; v < nk; v += 64)
                closed[v] = H.holes[at + v];
            CAPE_MP_SYNC();
            ck = union_dp_candidate(L, closed, nk, H.cand + at, eps, lane);
            valid = ck >= 3 && union_ring_is_simple(H.cand + at, ck, lane) && union_all_inside(H.cand + at, ck, cand, cn, lane);
        }
        if (lane == 0)
            H.candLen[k] = (unsigned short)ck;
        CAPE_MP_SYNC();
        at += nk;
    }
    if (!valid)
        return n;
    // the candidates lie at their rings' old offsets: the area walks them one by one
    double newArea = cn < 3 ? 0.0 : fabs(ring_area_signed(cand, cn));
    for (int k = 0, at = 0; k < nHoles; ++k)
    {
        newArea -= fabs(ring_area_signed(H.cand + at, uni(H.candLen[k])));
        at += uni(H.holeLen[k]);
    }
    newArea = newArea < 0 ? 0.0 : newArea;
    if (!(newArea > area * 0.75))
        return n;
    CAPE_MP_SYNC();
    for (int i = lane; i < cn; i += 64)
        ring[i] = cand[i];
    for (int k = 0, from = 0, to = 0; k < nHoles; ++k) // packed down: a ring never moves up, and ring k moves before ring k + 1 is read
    {
        const int nk = uni(H.holeLen[k]), ck = uni(H.candLen[k]);
        for (int base = 0; base < ck; base += 64)
        {
            const int v = base + lane;
            double2 q = make_double2(0.0, 0.0);
            if (v < ck)
                q = H.cand[from + v];
            if (v < ck)
                H.holes[to + v] = q;
        }
        CAPE_MP_SYNC();
        if (lane == 0)
            H.holeLen[k] = (unsigned short)ck;
        from += nk;
        to += ck;
    }
    CAPE_MP_SYNC();
    area = newArea;
    return cn;
}

// ---- the arrangement of the two rings (rings_union_outer)
struct UnionGraph
{
    int nNodes;
    uint32_t fail; // CAPE_UNION_HOST_* bits met on the way
    double eps;
};

// node_of: the first node within eps of p (lanes over the nodes, the lowest set lane of the first chunk with a hit), else a new one
__device__ __forceinline__ int union_node_of(const UnionLds& L, UnionGraph& G, const double2& p, int lane)
{
    for (int base = 0; base < G.nNodes; base += 64)
    {
        const int k = base + lane;
        const bool hit = k < G.nNodes && usame(L.nodes[k], p, G.eps);
        const unsigned long long m = __ballot(hit);
        if (m)
            return base + __ffsll((long long)m) - 1;
    }
    if (G.nNodes >= kUnionNodes)
    {
        G.fail |= CAPE_UNION_HOST_CAPACITY;
        return -1;
    }
    if (lane == 0)
    {
        L.nodes[G.nNodes] = p;
        L.deg[G.nNodes] = 0;
        L.seen[G.nNodes] = 0;
    }
    CAPE_MP_SYNC();
    return G.nNodes++;
}

// link: an undirected edge, once
__device__ __forceinline__ void union_link(const UnionLds& L, UnionGraph& G, int a, int b, int lane)
{
    if (a < 0 || b < 0 || a == b)
        return;
    const int da = uni(L.deg[a]), db = uni(L.deg[b]);
    for (int k = 0; k < da && k < kUnionDegree; ++k)
        if (L.adj[a * kUnionDegree + k] == (unsigned short)b)
            return;
    if (da >= kUnionDegree || db >= kUnionDegree)
    {
        G.fail |= CAPE_UNION_HOST_CAPACITY;
        return;
    }
    if (lane == 0)
    {
        L.adj[a * kUnionDegree + da] = (unsigned short)b;
        L.adj[b * kUnionDegree + db] = (unsigned short)a;
        L.deg[a] = (unsigned char)(da + 1);
        L.deg[b] = (unsigned char)(db + 1);
    }
    CAPE_MP_SYNC();
}

// next_of: the first neighbour of v met when rotating counter-clockwise from the direction `back`; `from` is the node the walk came
// from (-1: none).  Lanes over the neighbours; the choice runs in adjacency order with the host's strict <.  Returns the neighbour's
// slot in v's list, -1 for a node without neighbours.
__device__ __forceinline__ int union_next_of(const UnionLds& L, UnionGraph& G, int v, const double2& back, int from, int lane)
{
    const int dv = uni(L.deg[v]);
    const double ba = atan2(back.y, back.x);
    bool amb = false;
    double ang = 0.0;
    if (lane < dv && lane < kUnionDegree)
    {
        const int w = L.adj[v * kUnionDegree + lane];
        const double2 pv = L.nodes[v], pw = L.nodes[w < kUnionNodes ? w : 0];
        const double dx = pw.x - pv.x, dy = pw.y - pv.y;
        ang = union_angle(dy, dx, ba, w == from || union_axis_parallel(dx, dy, back.x, back.y), amb);
    }
    int best = -1;
    double bestAngle = 1e300;
    for (int k = 0; k < dv && k < kUnionDegree; ++k)
    {
        const double a = readlane_f64(ang, k);
        if (a < bestAngle)
        {
            bestAngle = a;
            best = k;
        }
    }
    // two candidates closer than the band: the device's atan2 and the host's may order them differently
    const bool close = lane < dv && lane < kUnionDegree && lane != best && fabs(ang - bestAngle) < kUnionAngleBand;
    if (__any(amb || close))
        G.fail |= CAPE_UNION_HOST_AMBIGUOUS;
    return best;
}

// walk_face: the face the directed edge (from -> its neighbour in slot `slot`) has on its right, into ring[0, kUnionOut); every edge
// walked is marked seen.  Returns the length, -1 if the walk does not close within the host's guard or outgrows the ring.
__device__ __forceinline__ int union_walk_face(const UnionLds& L, UnionGraph& G, int from, int slot, double2* ring, int lane)
{
    const int to = uni(L.adj[from * kUnionDegree + slot]);
    int cur = from, nxt = to, curSlot = slot, n = 0;
    for (int guard = 0; guard < 4 * G.nNodes + 8; ++guard)
    {
        if (n >= kUnionOut || nxt < 0 || nxt >= G.nNodes)
            return -1;
        const double2 pc = L.nodes[cur], pn = L.nodes[nxt];
        if (lane == 0)
        {
            ring[n] = pc;
            L.seen[cur] = (unsigned char)(L.seen[cur] | (1u << curSlot));
        }
        ++n;
        CAPE_MP_SYNC();
        const int afterSlot = union_next_of(L, G, nxt, make_double2(pc.x - pn.x, pc.y - pn.y), cur, lane);
        if (afterSlot < 0)
            return -1;
        cur = nxt;
        nxt = uni(L.adj[cur * kUnionDegree + afterSlot]);
        curSlot = afterSlot;
        if (cur == from && nxt == to)
            return n;
    }
    return -1;
}

// ---- the steps of a pair that every mode runs (union_pair, union_pair_rings)
// Steps 1 and 2.  L.ringA[0, nA) holds the map polygon's ring in its frame `fa` (oriented or not), L.ringB[0, nB) the detection's
// world ring in its frame `fb`; both end up oriented in `frame`: the target, or the map polygon's own where Polygon::project's
// isApprox shortcut holds.  Returns whether Polygon::project ran.
__device__ __forceinline__ bool union_place_operands(const UnionLds& L, int nA, int nB, const UnionFrame& fa, const UnionFrame& fb,
                                                     const UnionFrame& target, UnionFrame& frame, int lane)
{
    bool projected = false;
    // ---- 1. the map ring: as the host class holds it, then Polygon::project into the target unless its frame already is the target
    union_orient(L.ringA, nA, lane);
    frame = fa;
    if (!(union_is_approx3(fa.c, target.c) && union_is_approx3(fa.x, target.x) && union_is_approx3(fa.y, target.y)))
    {
        for (int v = lane; v < nA; v += 64)
            L.ringA[v] = union_project(L.ringA[v], fa, target);
        CAPE_MP_SYNC();
        union_orient(L.ringA, nA, lane);
        frame = target;
        projected = true;
    }
    // ---- 2. the detection: merge_union always projects it into this polygon's frame
    union_orient(L.ringB, nB, lane);
    for (int v = lane; v < nB; v += 64)
        L.ringB[v] = union_project(L.ringB[v], fb, frame);
    CAPE_MP_SYNC();
    union_orient(L.ringB, nB, lane);
    return projected;
}

struct UnionResult
{
    uint32_t flags;
    int n;          // vertices of the result ring
    int nNodes;
    double area;
    const double2* ring; // in LDS
};

// a pair that is the host's: its reason alone (a capacity outranks every other), and the nodes met
__device__ __forceinline__ UnionResult union_hosted(uint32_t bits, int nNodes)
{
    UnionResult r{};
    r.flags = (bits & CAPE_UNION_HOST_CAPACITY) ? (uint32_t)CAPE_UNION_HOST_CAPACITY : bits;
    r.nNodes = nNodes;
    return r;
}

// One pair on one wavefront.  L.ringA[0, nA) holds the map polygon's ring in its frame `fa` (oriented or not), L.ringB[0, nB) the
// detection's world ring in its frame `fb`; `target` is the fusion frame.  3 <= nA, nB <= kUnionRing.  `frame` receives the frame of
// the result (the target, or the map polygon's own where Polygon::project's shortcut holds).
__device__ inline UnionResult union_pair(const UnionLds& L, int nA, int nB, const UnionFrame& fa, const UnionFrame& fb, const UnionFrame& target,
                                         UnionFrame& frame, int lane)
{
    UnionResult res{};
    (void)union_place_operands(L, nA, nB, fa, fb, target, frame, lane);
    const double2 *A = L.ringA, *B = L.ringB;
    const double areaMap = union_area(A, nA); // Polygon::_area of the projected map polygon
    res.flags = CAPE_UNION_SERVED | CAPE_UNION_UNCHANGED;
    res.ring = A;
    res.n = nA;
    res.area = areaMap;
    if (nA < 3 || nB < 3)
        return res;
    // ---- 3. rings_union_outer(A, B, &holes, 0)
    UnionGraph G{};
    double scale = 1.0;
    for (int v = 0; v < nA; ++v)
        scale = umax(scale, umax(fabs(A[v].x), fabs(A[v].y)));
    for (int v = 0; v < nB; ++v)
        scale = umax(scale, umax(fabs(B[v].x), fabs(B[v].y)));
    const double eps = 1e-9 * scale;
    G.eps = eps;
    // the segment list without `same` endpoints, ring A's first (ballot compaction keeps ring order)
    int nSegA = 0, nSeg = 0;
    for (int r = 0; r < 2; ++r)
    {
        const double2* R = r ? B : A;
        const int nR = r ? nB : nA;
        for (int base = 0; base < nR; base += 64)
        {
            const int i = base + lane;
            const bool keep = i < nR && !usame(R[i], R[i + 1 == nR ? 0 : i + 1], eps);
            const unsigned long long kb = __ballot(keep);
            if (keep)
                L.segs[nSeg + __popcll(kb & ((1ull << lane) - 1ull))] = (unsigned short)((r << 8) | i);
            nSeg += __popcll(kb);
        }
        if (r == 0)
            nSegA = nSeg;
    }
    CAPE_MP_SYNC();
    const int nSegB = nSeg - nSegA;
    auto seg_a = [&](int s) {
        const unsigned e = L.segs[s];
        return (e >> 8) ? B[e & 0xFF] : A[e & 0xFF];
    };
    auto seg_b = [&](int s) {
        const unsigned e = L.segs[s];
        const int i = (int)(e & 0xFF);
        return (e >> 8) ? B[i + 1 == nB ? 0 : i + 1] : A[i + 1 == nA ? 0 : i + 1];
    };
    // the cuts of every (A segment, B segment): lanes over the pairs, six possible cuts each, appended in ballot order (the per-segment
    // sort below makes the order of arrival irrelevant)
    int nCuts = 0;
    bool cutOverflow = false;
    for (int base = 0; base < nSegA * nSegB; base += 64)
    {
        const int q = base + lane;
        const bool live = q < nSegA * nSegB;
        double t[6] = {0, 0, 0, 0, 0, 0};
        bool has[6] = {false, false, false, false, false, false};
        int si = 0, ui = 0;
        if (live)
        {
            si = q / nSegB;
            ui = nSegA + q % nSegB;
            const double2 sa = seg_a(si), sb = seg_b(si), ua = seg_a(ui), ub = seg_b(ui);
            has[0] = union_param_on(sa, sb, ua, eps, t[0]);
            has[1] = union_param_on(sa, sb, ub, eps, t[1]);
            has[3] = union_param_on(ua, ub, sa, eps, t[3]);
            has[4] = union_param_on(ua, ub, sb, eps, t[4]);
            bool ks = false, ku = false;
            if (union_crossing(sa, sb, ua, ub, eps, t[2], ks, t[5], ku))
            {
                has[2] = ks;
                has[5] = ku;
            }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c)
        {
            const unsigned long long m = __ballot(has[c]);
            const int at = nCuts + __popcll(m & ((1ull << lane) - 1ull));
            if (has[c] && at < kUnionCuts)
            {
                L.cutT[at] = t[c];
                L.cutSeg[at] = (unsigned short)(c < 3 ? si : ui);
            }
            nCuts += __popcll(m);
        }
        if (nCuts > kUnionCuts)
        {
            cutOverflow = true;
            break;
        }
    }
    CAPE_MP_SYNC();
    if (cutOverflow)
        return union_hosted(CAPE_UNION_HOST_CAPACITY, 0);
    // the cuts in (segment, parameter) order: a rank sort on the parameters' bit patterns (non-negative doubles: the numbers' order)
    for (int base = 0; base < nCuts; base += 64)
    {
        const int c = base + lane;
        if (c < nCuts)
        {
            const unsigned sc = L.cutSeg[c];
            const unsigned long long tc = (unsigned long long)__double_as_longlong(L.cutT[c]);
            int rank = 0;
            for (int k = 0; k < nCuts; ++k)
            {
                const unsigned sk = L.cutSeg[k];
                const unsigned long long tk = (unsigned long long)__double_as_longlong(L.cutT[k]);
                rank += (sk < sc || (sk == sc && (tk < tc || (tk == tc && k < c)))) ? 1 : 0;
            }
            L.sortT[rank] = L.cutT[c];
            L.sortSeg[rank] = (unsigned short)sc;
        }
    }
    CAPE_MP_SYNC();
    // nodes and undirected edges in the host's order: segments in order, cuts ascending, the first node within eps wins
    int at = 0;
    for (int s = 0; s < nSeg && !G.fail; ++s)
    {
        const double2 a = seg_a(s), b = seg_b(s);
        int prev = union_node_of(L, G, a, lane);
        while (at < nCuts && uni(L.sortSeg[at]) == s && !G.fail)
        {
            const int cur = union_node_of(L, G, union_cut_point(a, b, L.sortT[at]), lane);
            union_link(L, G, prev, cur, lane);
            prev = cur;
            ++at;
        }
        if (!G.fail)
            union_link(L, G, prev, union_node_of(L, G, b, lane), lane);
    }
    CAPE_MP_SYNC(); // (the sorted cuts are dead: the walked rings take their place)
    res.nNodes = G.nNodes;
    const auto hosted = [&](uint32_t bits) { return union_hosted(bits, G.nNodes); };
    if (G.fail)
        return hosted(G.fail);
    int nOuter = 0;
    bool newHole = false;
    if (G.nNodes >= 3)
    {
        // the outer face from the lowest of the leftmost nodes, reached heading south
        int start = 0;
        for (int k = 1; k < G.nNodes; ++k)
        {
            const double2 pk = L.nodes[k], ps = L.nodes[start];
            if (pk.x < ps.x - eps || (fabs(pk.x - ps.x) <= eps && pk.y < ps.y))
                start = k;
        }
        const int firstSlot = union_next_of(L, G, start, make_double2(0.0, 1.0), -1, lane);
        if (firstSlot >= 0)
        {
            nOuter = union_walk_face(L, G, start, firstSlot, L.outer, lane);
            if (nOuter < 0)
                return hosted(G.fail | CAPE_UNION_HOST_CAPACITY);
            // every other face: bounded, walked clockwise; a hole of the union is one whose inside belongs to neither operand
            for (int a = 0; a < G.nNodes && nOuter > 0; ++a)
            {
                const int da = uni(L.deg[a]);
                for (int k = 0; k < da && k < kUnionDegree; ++k)
                {
                    if ((uni(L.seen[a]) >> k) & 1)
                        continue;
                    int nf = union_walk_face(L, G, a, k, L.face, lane);
                    if (nf < 0)
                        return hosted(G.fail | CAPE_UNION_HOST_CAPACITY);
                    if (nf < 3 || ring_area_signed(L.face, nf) >= 0)
                        continue; // not a bounded face (or a degenerate spur)
                    // a point strictly inside the face: just right of the middle of one of its edges
                    bool found = false;
                    double2 probe = make_double2(0.0, 0.0);
                    for (int i = 0; i < nf && !found; ++i)
                    {
                        const double2 p = L.face[i], q = L.face[i + 1 == nf ? 0 : i + 1];
                        const double dx = q.x - p.x, dy = q.y - p.y, len = hypot(dx, dy);
                        if (len <= eps)
                            continue;
                        int step = 0;
                        for (double off = 1e-3; off >= 1e-7 && !found && step < 8; off *= 0.1, ++step)
                        {
                            probe = make_double2(0.5 * (p.x + q.x) + off * len * (dy / len), 0.5 * (p.y + q.y) - off * len * (dx / len));
                            found = union_point_in_ring(probe, L.face, nf, false, lane);
                        }
                    }
                    if (!found)
                        continue;
                    const bool inA = union_point_in_ring(probe, A, nA, true, lane), inB = union_point_in_ring(probe, B, nB, true, lane);
                    if (inA || inB)
                        continue;
                    // merge_union's own test of a hole: drop_collinear, then at least 3 vertices and simple
                    nf = union_drop_collinear(L.face, nf, lane);
                    if (nf >= 3 && union_ring_is_simple(L.face, nf, lane))
                        newHole = true;
                }
            }
        }
    }
    if (G.fail)
        return hosted(G.fail);
    // ---- 4. the outer ring: drop_collinear, the disjoint rule, ring_is_simple
    if (nOuter > 0)
        nOuter = union_drop_collinear(L.outer, nOuter, lane);
    const double outerArea = nOuter >= 3 ? fabs(ring_area_signed(L.outer, nOuter)) : 0.0;
    const double areaA = fabs(ring_area_signed(A, nA)), areaB = fabs(ring_area_signed(B, nB));
    // an operand none of whose vertices lies inside or on the outer face is a piece of its own (MergeInfo::disjoint); the rule below
    // catches that when the piece walked is the smaller one
    bool disjoint = nOuter >= 3 && (union_left_out(A, nA, L.outer, nOuter, lane) || union_left_out(B, nB, L.outer, nOuter, lane));
    double2* out = L.outer;
    bool rule = false; // merge_union's own `disjoint`
    if (outerArea + 1e-9 * umax(areaA, areaB) < umax(areaA, areaB))
    {
        disjoint = rule = true;
        if (areaA >= areaB) // area() >= o.area(): this polygon is the bigger piece, simplified as it is
        {
            res.flags = CAPE_UNION_SERVED | CAPE_UNION_DISJOINT;
            res.n = union_simplify(L, L.ringA, nA, L.face, res.area, lane);
            res.ring = L.ringA;
            return res;
        }
        for (int v = lane; v < nB; v += 64)
            out[v] = B[v];
        nOuter = nB;
        CAPE_MP_SYNC();
    }
    if (nOuter < 3 || !union_ring_is_simple(out, nOuter, lane))
    {
        res.flags |= disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u; // merge_union returned false: the projected map polygon stays
        return res;
    }
    // ---- 5. a face merge_union would add as a hole
    if (!rule && newHole)
        return hosted(CAPE_UNION_HOST_NEW_HOLE);
    // ---- 6. Polygon(ring, x, y, c): a repeated closing vertex goes, the ring is oriented; then simplify()
    if (nOuter > 1 && out[0].x == out[nOuter - 1].x && out[0].y == out[nOuter - 1].y)
        --nOuter;
    union_orient(out, nOuter, lane);
    res.flags = CAPE_UNION_SERVED | (disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u);
    res.n = union_simplify(L, out, nOuter, L.face, res.area, lane);
    res.ring = out;
    return res;
}

// ... and of the holes mode: the interior rings lie back to back in UnionHolesLds::holes, their lengths in holeLen
struct UnionHoleResult
{
    int nHoles;
    uint32_t holesNew, holesKept, holesCovered;
};

// The map plane's interior rings as the projected polygon holds them (the holes mode): H.src / srcOff / srcLen describe them.
struct UnionHoleFetch
{
    const UnionHolesLds& H;
    const UnionFrame& fa;
    const UnionFrame& target;
    bool projected; // Polygon::project ran: the isApprox shortcut did not keep the map polygon's frame
    int lane;
    // ring k into dst: the Polygon constructor's add_hole, then -- if projected -- project's vertices and its add_hole.  Returns its length.
    __device__ __forceinline__ int hole(int k, double2* dst) const
    {
        const unsigned off = (unsigned)uni((int)H.srcOff[k]);
        const int n = uni(H.srcLen[k]);
        for (int v = lane; v < n; v += 64)
            dst[v] = H.src[off + v];
        CAPE_MP_SYNC();
        union_orient(dst, n, lane, true);
        if (projected)
        {
            for (int v = lane; v < n; v += 64)
                dst[v] = union_project(dst[v], fa, target);
            CAPE_MP_SYNC();
            union_orient(dst, n, lane, true);
        }
        return n;
    }
    // all of them into H.holes, back to back; false if they outgrow it
    __device__ __forceinline__ bool all() const
    {
        int at = 0;
        for (int k = 0; k < H.nSrc; ++k)
        {
            const int n = uni(H.srcLen[k]);
            if (at + n > kUnionHoleVertices)
                return false;
            hole(k, H.holes + at);
            if (lane == 0)
                H.holeLen[k] = (unsigned short)n;
            at += n;
        }
        CAPE_MP_SYNC();
        return true;
    }
    // Polygon::area() of the projected map polygon with the outer ring A: its holes pass through `scratch` one by one
    __device__ __forceinline__ double map_area(const double2* A, int nA, double2* scratch) const
    {
        double a = fabs(ring_area_signed(A, nA));
        for (int k = 0; k < H.nSrc; ++k)
        {
            const int n = hole(k, scratch);
            a -= fabs(ring_area_signed(scratch, n));
            CAPE_MP_SYNC();
        }
        return a < 0 ? 0.0 : a;
    }
};

// ---- the cut mode (cape_map_union_cut, cape_debug_polygon_union_cut): the holes mode, and a hole of the map plane the detection
// covers in part is cut into its pieces by a second arrangement inside the pair.
// The carve is the holes mode's, byte for byte.  The one thing the second arrangement cannot keep where the first has it is the
// sorted cut list: L.sortT aliases L.outer, which holds the union's outer ring by then.  It goes, with its segment numbers, to the
// intersection's heights (`by`), dead between two rings_inter_area calls.  Everything else of an arrangement -- the segment list,
// the cuts, the nodes, the adjacency, the degrees, the seen bits -- lies in [segs, outer), which only the intersection borrows and
// which is dead once that has returned for the hole; the walked faces, the second outer face among them, go to L.face (the
// intersection's bk / inc, as dead).  Live throughout: L.ringB, L.outer, H.holes, H.holeLen, H.srcOff, H.srcLen.
struct UnionCutLdsLayout
{
    size_t sortT, sortSeg, bytes;
};
__host__ __device__ constexpr UnionCutLdsLayout union_cut_layout()
{
    constexpr UnionHolesLdsLayout h = union_holes_layout();
    UnionCutLdsLayout o{};
    Layout by; // [by, by + the heights)
    by.off = h.by;
    o.sortT = by.take<double>(kUnionCuts);
    o.sortSeg = by.take<unsigned short>(kUnionCuts);
    CAPE_LAYOUT_CHECK(by.off <= h.by + 128 * kUnionMpStack * sizeof(double));
    o.bytes = h.bytes;
    return o;
}
static_assert(kUnionCuts * (sizeof(double) + sizeof(unsigned short)) <= 128 * kUnionMpStack * sizeof(double), "the second arrangement's sorted cuts fit the heights' place");
static_assert(union_cut_layout().sortT >= union_layout().bytes, "the second arrangement's sorted cuts lie behind the first carve: clear of L.outer and L.face");
static_assert(union_cut_layout().bytes == union_holes_layout().bytes && 2 * union_cut_layout().bytes <= 160 * 1024, "two waves' carves fit the LDS of a CU");

struct UnionCutLds
{
    double* sortT; // the second arrangement's sorted cuts
    unsigned short* sortSeg;
};
__device__ __forceinline__ UnionCutLds union_cut_carve(unsigned char* smem)
{
    constexpr UnionCutLdsLayout o = union_cut_layout();
    UnionCutLds C;
    C.sortT = carve_at<double>(smem, o.sortT);
    C.sortSeg = carve_at<unsigned short>(smem, o.sortSeg);
    return C;
}

// One arrangement of two rings and its faces: rings_union_outer(A, B, &holes, rule) followed by what merge_union does with every
// face it returns.  Rule 0 on (map ring, detection) gives the union and its new holes, rule 1 on (hole, detection) the pieces of a
// partly covered hole; the cut mode calls it with rule 1 only, its first arrangement being union_pair_rings' own.  Everything rings_union_outer derives from its operands is derived here from
// S.A and S.B: scale and eps, the segment list, the cuts and their order, the nodes and links, the start node and its first slot.
struct UnionArrangeSpec
{
    const double2 *A, *B; // both operands in one frame
    int nA, nB;
    int rule;             // 0: a face inside neither operand (a hole of the union); 1: inside or on A and not inside or on B (a piece of A \ B)
    double tiny;          // rule 1: a piece's |signed area| exceeds it (carry_hole)
    double* sortT;        // the sorted cuts: kUnionCuts each, dead once the nodes are numbered
    unsigned short* sortSeg;
    double2* outer;       // where the outer face is walked (kUnionOut + 1)
};
// The faces that pass are oriented by add_hole and appended to H.holes / H.holeLen at (count, vertices): all of them counted, stored
// while they fit.  nOuter: the outer face's length.  Returns 0, or the CAPE_UNION_HOST_* bits that end the pair.
__device__ __forceinline__ uint32_t union_arrange(const UnionLds& L, const UnionHolesLds& H, const UnionArrangeSpec& S, UnionGraph& G, int& nOuter,
                                                  int& count, int& vertices, int lane)
{
    const double2 *A = S.A, *B = S.B;
    const int nA = S.nA, nB = S.nB;
    double scale = 1.0;
    for (int v = 0; v < nA; ++v)
        scale = umax(scale, umax(fabs(A[v].x), fabs(A[v].y)));
    for (int v = 0; v < nB; ++v)
        scale = umax(scale, umax(fabs(B[v].x), fabs(B[v].y)));
    const double eps = 1e-9 * scale;
    G.eps = eps;
    // the segment list without `same` endpoints, ring A's first (ballot compaction keeps ring order)
    int nSegA = 0, nSeg = 0;
    for (int r = 0; r < 2; ++r)
    {
        const double2* R = r ? B : A;
        const int nR = r ? nB : nA;
        for (int base = 0; base < nR; base += 64)
        {
            const int i = base + lane;
            const bool keep = i < nR && !usame(R[i], R[i + 1 == nR ? 0 : i + 1], eps);
            const unsigned long long kb = __ballot(keep);
            if (keep)
                L.segs[nSeg + __popcll(kb & ((1ull << lane) - 1ull))] = (unsigned short)((r << 8) | i);
            nSeg += __popcll(kb);
        }
        if (r == 0)
            nSegA = nSeg;
    }
    CAPE_MP_SYNC();
    const int nSegB = nSeg - nSegA;
    auto seg_a = [&](int s) {
        const unsigned e = L.segs[s];
        return (e >> 8) ? B[e & 0xFF] : A[e & 0xFF];
    };
    auto seg_b = [&](int s) {
        const unsigned e = L.segs[s];
        const int i = (int)(e & 0xFF);
        return (e >> 8) ? B[i + 1 == nB ? 0 : i + 1] : A[i + 1 == nA ? 0 : i + 1];
    };
    // the cuts of every (A segment, B segment): lanes over the pairs, six possible cuts each, appended in ballot order (the per-segment
    // sort below makes the order of arrival irrelevant)
    int nCuts = 0;
    bool cutOverflow = false;
    for (int base = 0; base < nSegA * nSegB; base += 64)
    {
        const int q = base + lane;
        const bool live = q < nSegA * nSegB;
        double t[6] = {0, 0, 0, 0, 0, 0};
        bool has[6] = {false, false, false, false, false, false};
        int si = 0, ui = 0;
        if (live)
        {
            si = q / nSegB;
            ui = nSegA + q % nSegB;
            const double2 sa = seg_a(si), sb = seg_b(si), ua = seg_a(ui), ub = seg_b(ui);
            has[0] = union_param_on(sa, sb, ua, eps, t[0]);
            has[1] = union_param_on(sa, sb, ub, eps, t[1]);
            has[3] = union_param_on(ua, ub, sa, eps, t[3]);
            has[4] = union_param_on(ua, ub, sb, eps, t[4]);
            bool ks = false, ku = false;
            if (union_crossing(sa, sb, ua, ub, eps, t[2], ks, t[5], ku))
            {
                has[2] = ks;
                has[5] = ku;
            }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c)
        {
            const unsigned long long m = __ballot(has[c]);
            const int at = nCuts + __popcll(m & ((1ull << lane) - 1ull));
            if (has[c] && at < kUnionCuts)
            {
                L.cutT[at] = t[c];
                L.cutSeg[at] = (unsigned short)(c < 3 ? si : ui);
            }
            nCuts += __popcll(m);
        }
        if (nCuts > kUnionCuts)
        {
            cutOverflow = true;
            break;
        }
    }
    CAPE_MP_SYNC();
    if (cutOverflow)
        return CAPE_UNION_HOST_CAPACITY;
    // the cuts in (segment, parameter) order: a rank sort on the parameters' bit patterns (non-negative doubles: the numbers' order)
    for (int base = 0; base < nCuts; base += 64)
    {
        const int c = base + lane;
        if (c < nCuts)
        {
            const unsigned sc = L.cutSeg[c];
            const unsigned long long tc = (unsigned long long)__double_as_longlong(L.cutT[c]);
            int rank = 0;
            for (int k = 0; k < nCuts; ++k)
            {
                const unsigned sk = L.cutSeg[k];
                const unsigned long long tk = (unsigned long long)__double_as_longlong(L.cutT[k]);
                rank += (sk < sc || (sk == sc && (tk < tc || (tk == tc && k < c)))) ? 1 : 0;
            }
            S.sortT[rank] = L.cutT[c];
            S.sortSeg[rank] = (unsigned short)sc;
        }
    }
    CAPE_MP_SYNC();
    // nodes and undirected edges in the host's order: segments in order, cuts ascending, the first node within eps wins
    int at = 0;
    for (int s = 0; s < nSeg && !G.fail; ++s)
    {
        const double2 a = seg_a(s), b = seg_b(s);
        int prev = union_node_of(L, G, a, lane);
        while (at < nCuts && uni(S.sortSeg[at]) == s && !G.fail)
        {
            const int cur = union_node_of(L, G, union_cut_point(a, b, S.sortT[at]), lane);
            union_link(L, G, prev, cur, lane);
            prev = cur;
            ++at;
        }
        if (!G.fail)
            union_link(L, G, prev, union_node_of(L, G, b, lane), lane);
    }
    CAPE_MP_SYNC(); // (the sorted cuts are dead)
    if (G.fail)
        return G.fail;
    nOuter = 0;
    if (G.nNodes >= 3)
    {
        // the outer face from the lowest of the leftmost nodes, reached heading south
        int start = 0;
        for (int k = 1; k < G.nNodes; ++k)
        {
            const double2 pk = L.nodes[k], ps = L.nodes[start];
            if (pk.x < ps.x - eps || (fabs(pk.x - ps.x) <= eps && pk.y < ps.y))
                start = k;
        }
        const int firstSlot = union_next_of(L, G, start, make_double2(0.0, 1.0), -1, lane);
        if (firstSlot >= 0)
        {
            nOuter = union_walk_face(L, G, start, firstSlot, S.outer, lane);
            if (nOuter < 0)
                return G.fail | CAPE_UNION_HOST_CAPACITY;
            // every other face: bounded, walked clockwise, judged by the rule on a point strictly inside it
            for (int a = 0; a < G.nNodes && nOuter > 0; ++a)
            {
                const int da = uni(L.deg[a]);
                for (int k = 0; k < da && k < kUnionDegree; ++k)
                {
                    if ((uni(L.seen[a]) >> k) & 1)
                        continue;
                    int nf = union_walk_face(L, G, a, k, L.face, lane);
                    if (nf < 0)
                        return G.fail | CAPE_UNION_HOST_CAPACITY;
                    if (nf < 3 || ring_area_signed(L.face, nf) >= 0)
                        continue; // not a bounded face (or a degenerate spur)
                    // a point strictly inside the face: just right of the middle of one of its edges
                    bool found = false;
                    double2 probe = make_double2(0.0, 0.0);
                    for (int i = 0; i < nf && !found; ++i)
                    {
                        const double2 p = L.face[i], q = L.face[i + 1 == nf ? 0 : i + 1];
                        const double dx = q.x - p.x, dy = q.y - p.y, len = hypot(dx, dy);
                        if (len <= eps)
                            continue;
                        int step = 0;
                        for (double off = 1e-3; off >= 1e-7 && !found && step < 8; off *= 0.1, ++step)
                        {
                            probe = make_double2(0.5 * (p.x + q.x) + off * len * (dy / len), 0.5 * (p.y + q.y) - off * len * (dx / len));
                            found = union_point_in_ring(probe, L.face, nf, false, lane);
                        }
                    }
                    if (!found)
                        continue;
                    const bool inA = union_point_in_ring(probe, A, nA, true, lane), inB = union_point_in_ring(probe, B, nB, true, lane);
                    if (S.rule == 0 ? (inA || inB) : (!inA || inB))
                        continue;
                    // merge_union's own test of a hole, carry_hole's of a piece: drop_collinear, then at least 3 vertices, simple
                    // and -- a piece -- more than `tiny`
                    nf = union_drop_collinear(L.face, nf, lane);
                    if (nf >= 3 && union_ring_is_simple(L.face, nf, lane) && (S.rule == 0 || fabs(ring_area_signed(L.face, nf)) > S.tiny))
                    {
                        if (count < kUnionHoles && vertices + nf <= kUnionHoleVertices)
                        {
                            union_orient(L.face, nf, lane, true); // add_hole
                            for (int v = lane; v < nf; v += 64)
                                H.holes[vertices + v] = L.face[v];
                            if (lane == 0)
                                H.holeLen[count] = (unsigned short)nf;
                            CAPE_MP_SYNC();
                        }
                        ++count;
                        vertices += nf;
                    }
                }
            }
        }
    }
    return G.fail;
}

// The same pair in the modes with rings: the holes mode (Cuts = false: cape_map_union_holes, cape_debug_polygon_union) and the cut
// mode (Cuts = true: cape_map_union_cut, cape_debug_polygon_union_cut), one text with `if constexpr (Cuts)` at the three places they
// differ.  union_pair's steps -- the shared ones through the same functions, step 3 and the face test restated (see the head of this
// file) -- with the host's hole statements between them.  H.src / srcOff / srcLen describe the map plane's interior rings (H.nSrc <=
// kUnionHoles of 3 .. kUnionRing vertices each, inside their buffer: the caller has checked), which are fetched, oriented and
// projected where the host's statements read them; faces the union encloses and holes the detection leaves alone become the result's
// interior rings (`holes`; the rings in H.holes / H.holeLen).  A hole the detection covers in part is the host's in the holes mode
// (HOST_HOLE_CUT); in the cut mode union_arrange runs on (the hole as fetch.hole put it into L.ringA, the detection) with rule 1 and
// the sorted cuts in C, and its pieces follow the interior rings stored so far, so that the rings stand as merge_union appends them.
// A pair without such a hole computes the same result in both modes, bit for bit.  C is read in the cut mode only.  Never
// HOST_MAP_HOLES or HOST_NEW_HOLE; never HOST_HOLE_CUT in the cut mode.
template <bool Cuts>
__device__ inline UnionResult union_pair_rings(const UnionLds& L, const UnionHolesLds& H, const UnionCutLds& C, int nA, int nB, const UnionFrame& fa,
                                               const UnionFrame& fb, const UnionFrame& target, UnionFrame& frame, UnionHoleResult& holes, int lane)
{
    UnionResult res{};
    const bool projected = union_place_operands(L, nA, nB, fa, fb, target, frame, lane);
    const double2 *A = L.ringA, *B = L.ringB;
    const UnionHoleFetch fetch{H, fa, target, projected, lane};
    const double areaMap = union_area(A, nA); // Polygon::_area of the projected map polygon (without holes)
    res.flags = CAPE_UNION_SERVED | CAPE_UNION_UNCHANGED;
    res.ring = A;
    res.n = nA;
    res.area = areaMap;
    if (nA < 3 || nB < 3)
        return res;
    // ---- 3. rings_union_outer(A, B, &holes, 0)
    UnionGraph G{};
    double scale = 1.0;
    for (int v = 0; v < nA; ++v)
        scale = umax(scale, umax(fabs(A[v].x), fabs(A[v].y)));
    for (int v = 0; v < nB; ++v)
        scale = umax(scale, umax(fabs(B[v].x), fabs(B[v].y)));
    const double eps = 1e-9 * scale;
    G.eps = eps;
    // the segment list without `same` endpoints, ring A's first (ballot compaction keeps ring order)
    int nSegA = 0, nSeg = 0;
    for (int r = 0; r < 2; ++r)
    {
        const double2* R = r ? B : A;
        const int nR = r ? nB : nA;
        for (int base = 0; base < nR; base += 64)
        {
            const int i = base + lane;
            const bool keep = i < nR && !usame(R[i], R[i + 1 == nR ? 0 : i + 1], eps);
            const unsigned long long kb = __ballot(keep);
            if (keep)
                L.segs[nSeg + __popcll(kb & ((1ull << lane) - 1ull))] = (unsigned short)((r << 8) | i);
            nSeg += __popcll(kb);
        }
        if (r == 0)
            nSegA = nSeg;
    }
    CAPE_MP_SYNC();
    const int nSegB = nSeg - nSegA;
    auto seg_a = [&](int s) {
        const unsigned e = L.segs[s];
        return (e >> 8) ? B[e & 0xFF] : A[e & 0xFF];
    };
    auto seg_b = [&](int s) {
        const unsigned e = L.segs[s];
        const int i = (int)(e & 0xFF);
        return (e >> 8) ? B[i + 1 == nB ? 0 : i + 1] : A[i + 1 == nA ? 0 : i + 1];
    };
    // the cuts of every (A segment, B segment): lanes over the pairs, six possible cuts each, appended in ballot order (the per-segment
    // sort below makes the order of arrival irrelevant)
    int nCuts = 0;
    bool cutOverflow = false;
    for (int base = 0; base < nSegA * nSegB; base += 64)
    {
        const int q = base + lane;
        const bool live = q < nSegA * nSegB;
        double t[6] = {0, 0, 0, 0, 0, 0};
        bool has[6] = {false, false, false, false, false, false};
        int si = 0, ui = 0;
        if (live)
        {
            si = q / nSegB;
            ui = nSegA + q % nSegB;
            const double2 sa = seg_a(si), sb = seg_b(si), ua = seg_a(ui), ub = seg_b(ui);
            has[0] = union_param_on(sa, sb, ua, eps, t[0]);
            has[1] = union_param_on(sa, sb, ub, eps, t[1]);
            has[3] = union_param_on(ua, ub, sa, eps, t[3]);
            has[4] = union_param_on(ua, ub, sb, eps, t[4]);
            bool ks = false, ku = false;
            if (union_crossing(sa, sb, ua, ub, eps, t[2], ks, t[5], ku))
            {
                has[2] = ks;
                has[5] = ku;
            }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c)
        {
            const unsigned long long m = __ballot(has[c]);
            const int at = nCuts + __popcll(m & ((1ull << lane) - 1ull));
            if (has[c] && at < kUnionCuts)
            {
                L.cutT[at] = t[c];
                L.cutSeg[at] = (unsigned short)(c < 3 ? si : ui);
            }
            nCuts += __popcll(m);
        }
        if (nCuts > kUnionCuts)
        {
            cutOverflow = true;
            break;
        }
    }
    CAPE_MP_SYNC();
    if (cutOverflow)
        return union_hosted(CAPE_UNION_HOST_CAPACITY, 0);
    // the cuts in (segment, parameter) order: a rank sort on the parameters' bit patterns (non-negative doubles: the numbers' order)
    for (int base = 0; base < nCuts; base += 64)
    {
        const int c = base + lane;
        if (c < nCuts)
        {
            const unsigned sc = L.cutSeg[c];
            const unsigned long long tc = (unsigned long long)__double_as_longlong(L.cutT[c]);
            int rank = 0;
            for (int k = 0; k < nCuts; ++k)
            {
                const unsigned sk = L.cutSeg[k];
                const unsigned long long tk = (unsigned long long)__double_as_longlong(L.cutT[k]);
                rank += (sk < sc || (sk == sc && (tk < tc || (tk == tc && k < c)))) ? 1 : 0;
            }
            L.sortT[rank] = L.cutT[c];
            L.sortSeg[rank] = (unsigned short)sc;
        }
    }
    CAPE_MP_SYNC();
    // nodes and undirected edges in the host's order: segments in order, cuts ascending, the first node within eps wins
    int at = 0;
    for (int s = 0; s < nSeg && !G.fail; ++s)
    {
        const double2 a = seg_a(s), b = seg_b(s);
        int prev = union_node_of(L, G, a, lane);
        while (at < nCuts && uni(L.sortSeg[at]) == s && !G.fail)
        {
            const int cur = union_node_of(L, G, union_cut_point(a, b, L.sortT[at]), lane);
            union_link(L, G, prev, cur, lane);
            prev = cur;
            ++at;
        }
        if (!G.fail)
            union_link(L, G, prev, union_node_of(L, G, b, lane), lane);
    }
    CAPE_MP_SYNC(); // (the sorted cuts are dead: the walked rings take their place)
    res.nNodes = G.nNodes;
    const auto hosted = [&](uint32_t bits) { return union_hosted(bits, G.nNodes); };
    if (G.fail)
        return hosted(G.fail);
    int nOuter = 0;
    int nNew = 0, newVertices = 0; // faces added as holes: all of them counted, stored while they fit
    if (G.nNodes >= 3)
    {
        // the outer face from the lowest of the leftmost nodes, reached heading south
        int start = 0;
        for (int k = 1; k < G.nNodes; ++k)
        {
            const double2 pk = L.nodes[k], ps = L.nodes[start];
            if (pk.x < ps.x - eps || (fabs(pk.x - ps.x) <= eps && pk.y < ps.y))
                start = k;
        }
        const int firstSlot = union_next_of(L, G, start, make_double2(0.0, 1.0), -1, lane);
        if (firstSlot >= 0)
        {
            nOuter = union_walk_face(L, G, start, firstSlot, L.outer, lane);
            if (nOuter < 0)
                return hosted(G.fail | CAPE_UNION_HOST_CAPACITY);
            // every other face: bounded, walked clockwise; a hole of the union is one whose inside belongs to neither operand
            for (int a = 0; a < G.nNodes && nOuter > 0; ++a)
            {
                const int da = uni(L.deg[a]);
                for (int k = 0; k < da && k < kUnionDegree; ++k)
                {
                    if ((uni(L.seen[a]) >> k) & 1)
                        continue;
                    int nf = union_walk_face(L, G, a, k, L.face, lane);
                    if (nf < 0)
                        return hosted(G.fail | CAPE_UNION_HOST_CAPACITY);
                    if (nf < 3 || ring_area_signed(L.face, nf) >= 0)
                        continue; // not a bounded face (or a degenerate spur)
                    // a point strictly inside the face: just right of the middle of one of its edges
                    bool found = false;
                    double2 probe = make_double2(0.0, 0.0);
                    for (int i = 0; i < nf && !found; ++i)
                    {
                        const double2 p = L.face[i], q = L.face[i + 1 == nf ? 0 : i + 1];
                        const double dx = q.x - p.x, dy = q.y - p.y, len = hypot(dx, dy);
                        if (len <= eps)
                            continue;
                        int step = 0;
                        for (double off = 1e-3; off >= 1e-7 && !found && step < 8; off *= 0.1, ++step)
                        {
                            probe = make_double2(0.5 * (p.x + q.x) + off * len * (dy / len), 0.5 * (p.y + q.y) - off * len * (dx / len));
                            found = union_point_in_ring(probe, L.face, nf, false, lane);
                        }
                    }
                    if (!found)
                        continue;
                    const bool inA = union_point_in_ring(probe, A, nA, true, lane), inB = union_point_in_ring(probe, B, nB, true, lane);
                    if (inA || inB)
                        continue;
                    // merge_union's own test of a hole: drop_collinear, then at least 3 vertices and simple
                    nf = union_drop_collinear(L.face, nf, lane);
                    if (nf >= 3 && union_ring_is_simple(L.face, nf, lane))
                    {
                        if (nNew < kUnionHoles && newVertices + nf <= kUnionHoleVertices)
                        {
                            union_orient(L.face, nf, lane, true); // add_hole
                            for (int v = lane; v < nf; v += 64)
                                H.holes[newVertices + v] = L.face[v];
                            if (lane == 0)
                                H.holeLen[nNew] = (unsigned short)nf;
                            CAPE_MP_SYNC();
                        }
                        ++nNew;
                        newVertices += nf;
                    }
                }
            }
        }
    }
    if (G.fail)
        return hosted(G.fail);
    // ---- 4. the outer ring: drop_collinear, the disjoint rule, ring_is_simple
    if (nOuter > 0)
        nOuter = union_drop_collinear(L.outer, nOuter, lane);
    const double outerArea = nOuter >= 3 ? fabs(ring_area_signed(L.outer, nOuter)) : 0.0;
    const double areaA = fabs(ring_area_signed(A, nA)), areaB = fabs(ring_area_signed(B, nB));
    // an operand none of whose vertices lies inside or on the outer face is a piece of its own (MergeInfo::disjoint); the rule below
    // catches that when the piece walked is the smaller one
    bool disjoint = nOuter >= 3 && (union_left_out(A, nA, L.outer, nOuter, lane) || union_left_out(B, nB, L.outer, nOuter, lane));
    double2* out = L.outer;
    bool rule = false; // merge_union's own `disjoint`
    if (outerArea + 1e-9 * umax(areaA, areaB) < umax(areaA, areaB))
    {
        disjoint = rule = true;
        // area() >= o.area(), where area() counts the holes out: this polygon is the bigger piece, simplified as it is, holes and all
        if (fetch.map_area(A, nA, L.face) >= areaB)
        {
            res.flags = CAPE_UNION_SERVED | CAPE_UNION_DISJOINT;
            if (!fetch.all()) // (the faces stored there are no holes of this result)
                return hosted(CAPE_UNION_HOST_CAPACITY);
            holes.nHoles = H.nSrc;
            res.flags |= H.nSrc > 0 ? (uint32_t)CAPE_UNION_HOLES : 0u;
            res.n = union_simplify_holed(L, H, L.ringA, nA, H.nSrc, L.face, res.area, lane);
            res.ring = L.ringA;
            return res;
        }
        for (int v = lane; v < nB; v += 64)
            out[v] = B[v];
        nOuter = nB;
        CAPE_MP_SYNC();
    }
    if (nOuter < 3 || !union_ring_is_simple(out, nOuter, lane))
    {
        res.flags |= disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u; // merge_union returned false: the projected map polygon stays
        if (!fetch.all()) // ... with its projected holes
            return hosted(CAPE_UNION_HOST_CAPACITY);
        holes.nHoles = H.nSrc;
        res.flags |= H.nSrc > 0 ? (uint32_t)CAPE_UNION_HOLES : 0u;
        res.area = union_area_holed(A, nA, H.holes, H.holeLen, H.nSrc);
        return res;
    }
    // ---- 5. Polygon(ring, x, y, c): a repeated closing vertex goes, the ring is oriented; then simplify()
    if (nOuter > 1 && out[0].x == out[nOuter - 1].x && out[0].y == out[nOuter - 1].y)
        --nOuter;
    union_orient(out, nOuter, lane);
    res.flags = CAPE_UNION_SERVED | (disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u);
    res.ring = out;
    // ---- 6. the interior rings.  The detection is the bigger piece of two: none (it has none).  Otherwise the faces stored
    // above, then the map plane's holes in their order (carry_hole): kept where the detection covers at most `tiny` of them,
    // gone where it covers them; where it covers a part, the host's in the holes mode, and in the cut mode the pieces of
    // rings_union_outer(hole, detection, &pieces, 1) in face-walk order.  Everything is counted, stored while it fits, and judged
    // at the end: a partly covered hole of the holes mode first, then the capacities.
    int nHoles = 0, holeVertices = 0;
    bool cut = false;
    if (!rule)
    {
        nHoles = nNew;
        holeVertices = newVertices;
        holes.holesNew = (uint32_t)nNew;
        const double tiny = 1e-12 * umax(areaA, areaB); // (of the first pair of operands, for every hole)
        for (int k = 0; k < H.nSrc; ++k)
        {
            const int nh = fetch.hole(k, L.ringA); // (ring A is dead: the outer ring stands in L.outer)
            const double inter = union_boxes_apart(L.ringA, nh, B, nB) ? 0.0 : rings_inter_area<kUnionMpStack, kUnionMpXs>(H.mp, nh, nB, lane);
            if (inter != inter) // one of its capacities
                return hosted(CAPE_UNION_HOST_CAPACITY);
            const double covered = inter < 0 ? 0.0 : inter;
            if (covered <= tiny)
            {
                if (nHoles < kUnionHoles && holeVertices + nh <= kUnionHoleVertices)
                {
                    for (int v = lane; v < nh; v += 64)
                        H.holes[holeVertices + v] = L.ringA[v];
                    if (lane == 0)
                        H.holeLen[nHoles] = (unsigned short)nh;
                }
                ++nHoles;
                holeVertices += nh;
                ++holes.holesKept;
            }
            else if (inter < fabs(ring_area_signed(L.ringA, nh)) - tiny)
            {
                cut = true;
                if constexpr (Cuts)
                {
                    CAPE_MP_SYNC(); // (the intersection's arrays are dead: the second arrangement takes their place)
                    UnionGraph G2{};
                    int nOuter2 = 0;
                    const UnionArrangeSpec second{L.ringA, B, nh, nB, 1, tiny, C.sortT, C.sortSeg, L.face};
                    const uint32_t bits = union_arrange(L, H, second, G2, nOuter2, nHoles, holeVertices, lane);
                    if (bits)
                        return hosted(bits);
                }
            }
            else
                ++holes.holesCovered;
            CAPE_MP_SYNC();
        }
    }
    if constexpr (!Cuts)
        if (cut)
            return hosted(CAPE_UNION_HOST_HOLE_CUT);
    if (nHoles > kUnionHoles || holeVertices > kUnionHoleVertices)
        return hosted(CAPE_UNION_HOST_CAPACITY);
    holes.nHoles = nHoles;
    res.flags |= nHoles > 0 ? (uint32_t)CAPE_UNION_HOLES : 0u;
    if constexpr (Cuts)
        res.flags |= cut ? (uint32_t)CAPE_UNION_HOLE_PIECES : 0u;
    res.n = union_simplify_holed(L, H, out, nOuter, nHoles, L.face, res.area, lane);
    return res;
}


} // namespace

} // namespace cape
#endif // __HIPCC__

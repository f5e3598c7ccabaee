// The plain per-lane functions of csrc/cape_map_union.h (projection, cut parameters, crossing points, the angle choice with its guard
// band, the collinear test, the point-in-ring edge test, segments_intersect and the Douglas-Peucker distance) compiled for the HOST and
// compared bit for bit with host/boundary_polygon.cpp on random inputs, under the address and undefined-behaviour sanitizers.  A
// stand-alone program: tests/host/hip_stub stands in for the HIP runtime header, so the first part of the device header compiles as
// plain C++ (its second part, the wave's, is left out without __HIPCC__).  boundary_polygon.cpp is included as text, which makes the
// functions of its anonymous namespaces callable here: segment_distance2, segments_intersect, point_in_ring and drop_collinear are
// called directly, Polygon::project through the class; param_on, the crossing and next_of's angle are lambdas inside
// rings_union_outer and are restated below, statement for statement, as the reference.  Build and run from rgb-d-slam_amd/csrc:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I../../tests/host/hip_stub -I. -I../host -I../host/compat \
//       -o ../lib/map_union_algebra.exe ../../tests/host/map_union_algebra.cpp && ../lib/map_union_algebra.exe
//
// What needs the wave and is therefore covered on the GPU only (tests/test_gpu_map_union.py): the ballot-ordered cut list, node_of's
// search, link, the face walks, the probe loop, every barrier and the LDS carve.  The rank sort, ring_is_simple's lane loop,
// drop_collinear's erase and the Douglas-Peucker reduction are restated below in the wave's shape (seq::), and run on the named long
// pairs of tests/test_map_union_host.py, whose flags, vertex counts and node counts the program prints and checks.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../rgb-d-slam_amd/host/boundary_polygon.cpp"

#include "cape_map_union.h"

namespace ref = rgbd_slam::utils;
using rgbd_slam::vector2;
using rgbd_slam::vector3;

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// ---- The per-pair order of statements of csrc/cape_map_union.h's union_pair, one lane at a time: the same per-lane functions in the
// same order (the cut list in pair order instead of ballot order, which the sort makes irrelevant).  What the device's two modes have in common
// stands once here: seq::Arrangement and seq::dp_candidate also serve holes::pair of map_union_holes_algebra.cpp, which includes
// this file.  Four loops keep the wave's
// shape, 64 lanes at a time, because their chunking decides the result: the rank sort of the cuts, ring_is_simple's rounds with
// every other one reversed, drop_collinear's erase and the Douglas-Peucker reduction with its tie rule.  It checks that the
// restatement -- cuts ranked on their bit patterns, edges marked seen while they are walked, a hole judged as soon as its face is
// known, the closing-vertex and orientation rules of the constructor, the disjoint fact -- is the host class's merge_union and
// simplify, on random pairs and on the named long pairs below, whose node counts it also yields; the wave's mechanics (ballots,
// barriers, LDS) are the GPU tests'.
namespace seq {
using cape::usame;
typedef std::vector<double2> Ring2;
struct Out
{
    uint32_t flags = 0;
    std::vector<double2> ring;
    double area = 0;
    int nNodes = 0; // the arrangement's nodes: what the device reports as n_nodes (counted on, not capped, beyond its capacity)
};
static double signed_area(const std::vector<double2>& r)
{
    double s = 0;
    for (size_t i = 0, j = r.size() - 1; i < r.size(); j = i++)
        s += (r[j].x * r[i].y - r[i].x * r[j].y);
    return 0.5 * s;
}
static double area_of(const std::vector<double2>& r) { return r.size() < 3 ? 0.0 : std::abs(signed_area(r)); }
static void orient(std::vector<double2>& r)
{
    if (signed_area(r) > 0)
        std::reverse(r.begin(), r.end());
}
static bool in_ring(const double2& p, const std::vector<double2>& r, bool closed)
{
    bool on = false, inside = false;
    for (size_t i = 0; i < r.size(); ++i)
    {
        const int e = cape::union_point_edge(p, r[i], r[i == 0 ? r.size() - 1 : i - 1]);
        on = on || e == 2;
        inside = inside != (e == 1);
    }
    return on ? closed : inside;
}
static bool simple(const std::vector<double2>& r)
{
    const size_t n = r.size();
    if (n < 3)
        return false;
    // the device's lanes: 64 first edges at a time, every other round with the lanes reversed; a lane that met a pair stops looking
    bool bad[64] = {};
    for (size_t base = 0, round = 0; base < n; base += 64, ++round)
        for (size_t lane = 0; lane < 64; ++lane)
        {
            const size_t i = base + ((round & 1) ? 63 - lane : lane);
            if (i >= n)
                continue;
            for (size_t j = i + 1; j < n && !bad[lane]; ++j)
            {
                if (j == i + 1 || (i == 0 && j == n - 1))
                    continue;
                bad[lane] = cape::union_segments_intersect(r[i], r[(i + 1) % n], r[j], r[(j + 1) % n]);
            }
        }
    if (std::any_of(bad, bad + 64, [](bool b) { return b; }))
        return false;
    return std::abs(signed_area(r)) > 0;
}
static void drop(std::vector<double2>& r)
{
    bool changed = true;
    while (changed && r.size() > 3)
    {
        changed = false;
        for (size_t i = 0; i < r.size() && r.size() > 3; ++i)
            if (cape::union_collinear(r[(i + r.size() - 1) % r.size()], r[i], r[(i + 1) % r.size()]))
            {
                // the device's erase: the tail moves down 64 vertices at a time, every lane reading before any lane writes
                const size_t n = r.size();
                for (size_t base = i; base + 1 < n; base += 64)
                {
                    double2 v[64];
                    for (size_t lane = 0; lane < 64; ++lane)
                        v[lane] = base + lane + 1 < n ? r[base + lane + 1] : make_double2(0.0, 0.0);
                    for (size_t lane = 0; lane < 64; ++lane)
                        if (base + lane + 1 < n)
                            r[base + lane] = v[lane];
                }
                r.pop_back();
                changed = true;
                --i;
            }
    }
}
// union_dp_candidate: the closed ring, the lanes' first largest, the lowest index among the lanes that hold the wave's largest
static Ring2 dp_candidate(const Ring2& ring, double eps)
{
    const int n = (int)ring.size();
    Ring2 closed = ring;
    closed.push_back(ring[0]);
    std::vector<char> keep(n + 1, 0);
    keep[0] = keep[n] = 1;
    std::vector<std::pair<int, int>> stack {{0, n}};
    while (!stack.empty())
    {
        const auto [a, b] = stack.back();
        stack.pop_back();
        if (b <= a + 1)
            continue;
        // the device's lanes: lane l looks at a + 1 + l, a + 1 + l + 64, ... and keeps its first largest; the wave takes the largest
        // of the lanes' and, among the lanes that hold it, the lowest index: the host's strict > over the whole span
        uint64_t laneBest[64] = {}, best = 0;
        int laneIdx[64], idx = 0x7FFFFFFF;
        for (int lane = 0; lane < 64; ++lane)
        {
            laneIdx[lane] = 0x7FFFFFFF;
            for (int i = a + 1 + lane; i < b; i += 64)
            {
                const double d = cape::union_segment_distance2(closed[i], closed[a], closed[b]);
                uint64_t db;
                std::memcpy(&db, &d, sizeof db);
                if (laneIdx[lane] == 0x7FFFFFFF || db > laneBest[lane])
                    laneBest[lane] = db, laneIdx[lane] = i;
            }
            best = std::max(best, laneBest[lane]);
        }
        for (int lane = 0; lane < 64; ++lane)
            if (laneIdx[lane] != 0x7FFFFFFF && laneBest[lane] == best)
                idx = std::min(idx, laneIdx[lane]);
        double dmax;
        std::memcpy(&dmax, &best, sizeof dmax);
        if (dmax > eps * eps && idx > a && idx < b)
        {
            keep[idx] = 1;
            stack.push_back({a, idx});
            stack.push_back({idx, b});
        }
    }
    Ring2 cand;
    for (int i = 0; i < n; ++i)
        if (keep[i])
            cand.push_back(closed[i]);
    return cand;
}
static void simplify(Ring2& ring, double& area)
{
    area = area_of(ring);
    if (ring.size() < 4)
        return;
    const Ring2 cand = dp_candidate(ring, cape::umax(area / 1e5, 10.0));
    if (cand.size() >= 3 && simple(cand))
    {
        const double newArea = area_of(cand);
        if (newArea > area * 0.75)
        {
            ring = cand;
            area = newArea;
        }
    }
}
// is every vertex of q outside `outer` (not inside, not on it)?  union_left_out
static bool left_out(const Ring2& q, const Ring2& outer)
{
    for (const double2& p : q)
        if (in_ring(p, outer, true))
            return false;
    return true;
}

// The arrangement of both modes (step 3 of union_pair and union_pair_holes with union_node_of, union_link, union_next_of and
// union_walk_face, the start of the outer walk and the test of a walked face): seq::pair and holes::pair both run it, so an edit to
// the order of the device's statements is mirrored here once.
struct Arrangement
{
    static constexpr int kDeg = 8, kNodes = 512, kOut = 512, kCuts = 1024;
    double eps = 0;
    std::vector<double2> nodes; // counted on, not capped, beyond kNodes
    std::vector<std::vector<int>> adj;
    std::vector<unsigned> seen; // bit k: the directed edge to neighbour k has been walked
    bool capacity = false, ambiguous = false;

    int node_of(const double2& p)
    {
        for (size_t k = 0; k < nodes.size(); ++k)
            if (usame(nodes[k], p, eps))
                return (int)k;
        capacity = capacity || (int)nodes.size() >= kNodes;
        nodes.push_back(p);
        adj.emplace_back();
        return (int)nodes.size() - 1;
    }
    void link(int a, int b)
    {
        if (a == b || std::find(adj[a].begin(), adj[a].end(), b) != adj[a].end())
            return;
        adj[a].push_back(b);
        adj[b].push_back(a);
        capacity = capacity || (int)adj[a].size() > kDeg || (int)adj[b].size() > kDeg;
    }
    // A, B: both operands in one frame, oriented.  False when the cuts outgrow their list (nothing is numbered then).
    bool build(const Ring2& A, const Ring2& B)
    {
        double scale = 1.0;
        for (const auto* r : {&A, &B})
            for (const double2& p : *r)
                scale = cape::umax(scale, cape::umax(std::fabs(p.x), std::fabs(p.y)));
        eps = 1e-9 * scale;
        struct Seg { double2 a, b; };
        std::vector<Seg> segs;
        int nSegA = 0;
        for (int r = 0; r < 2; ++r)
        {
            const auto& R = r ? B : A;
            for (size_t i = 0; i < R.size(); ++i)
                if (!usame(R[i], R[(i + 1) % R.size()], eps))
                    segs.push_back({R[i], R[(i + 1) % R.size()]});
            if (r == 0)
                nSegA = (int)segs.size();
        }
        // the cuts in pair order instead of ballot order, which the sort makes irrelevant
        struct Cut { unsigned seg; uint64_t t; };
        std::vector<Cut> cuts;
        auto push = [&](unsigned seg, double t) {
            uint64_t b;
            std::memcpy(&b, &t, sizeof b);
            cuts.push_back({seg, b});
        };
        for (int i = 0; i < nSegA; ++i)
            for (int j = nSegA; j < (int)segs.size(); ++j)
            {
                const Seg &s = segs[i], &u = segs[j];
                double t;
                if (cape::union_param_on(s.a, s.b, u.a, eps, t)) push(i, t);
                if (cape::union_param_on(s.a, s.b, u.b, eps, t)) push(i, t);
                if (cape::union_param_on(u.a, u.b, s.a, eps, t)) push(j, t);
                if (cape::union_param_on(u.a, u.b, s.b, eps, t)) push(j, t);
                double ts, tu;
                bool ks, ku;
                if (cape::union_crossing(s.a, s.b, u.a, u.b, eps, ts, ks, tu, ku))
                {
                    if (ks) push(i, ts);
                    if (ku) push(j, tu);
                }
            }
        if ((int)cuts.size() > kCuts)
            return false;
        // the device's rank sort, statement for statement: a cut's place is the number of cuts before it in (segment, parameter,
        // arrival) order.  A slot no cut claims keeps a segment that does not exist, which ends the node numbering early.
        {
            std::vector<Cut> sorted(cuts.size(), Cut {0xFFFFu, ~0ull});
            for (size_t c = 0; c < cuts.size(); ++c)
            {
                size_t rank = 0;
                for (size_t k = 0; k < cuts.size(); ++k)
                    rank += (cuts[k].seg < cuts[c].seg || (cuts[k].seg == cuts[c].seg && (cuts[k].t < cuts[c].t || (cuts[k].t == cuts[c].t && k < c)))) ? 1 : 0;
                sorted[rank] = cuts[c];
            }
            cuts = sorted;
        }
        size_t at = 0;
        for (size_t s = 0; s < segs.size(); ++s)
        {
            int prev = node_of(segs[s].a);
            for (; at < cuts.size() && cuts[at].seg == s; ++at)
            {
                double t;
                std::memcpy(&t, &cuts[at].t, sizeof t);
                const int cur = node_of(cape::union_cut_point(segs[s].a, segs[s].b, t));
                link(prev, cur);
                prev = cur;
            }
            link(prev, node_of(segs[s].b));
        }
        seen.assign(nodes.size(), 0);
        return true;
    }
    int next_of(int v, const double2& back, int from)
    {
        const double ba = std::atan2(back.y, back.x);
        int best = -1;
        double bestAngle = 1e300;
        std::vector<double> angs;
        for (size_t k = 0; k < adj[v].size(); ++k)
        {
            const int w = adj[v][k];
            const double dx = nodes[w].x - nodes[v].x, dy = nodes[w].y - nodes[v].y;
            const double ang = cape::union_angle(dy, dx, ba, w == from || cape::union_axis_parallel(dx, dy, back.x, back.y), ambiguous);
            angs.push_back(ang);
            if (ang < bestAngle)
                bestAngle = ang, best = (int)k;
        }
        for (size_t k = 0; k < angs.size(); ++k)
            ambiguous = ambiguous || ((int)k != best && std::fabs(angs[k] - bestAngle) < cape::kUnionAngleBand);
        return best;
    }
    // the face the directed edge (from -> its neighbour in slot `slot`) has on its right; edges are marked seen while they are walked
    bool walk(int from, int slot, Ring2& ring)
    {
        ring.clear();
        const int to = adj[from][slot];
        int cur = from, nxt = to, curSlot = slot;
        for (size_t guard = 0; guard < 4 * nodes.size() + 8; ++guard)
        {
            if ((int)ring.size() >= kOut)
                return false;
            ring.push_back(nodes[cur]);
            seen[cur] |= 1u << curSlot;
            const int after = next_of(nxt, make_double2(nodes[cur].x - nodes[nxt].x, nodes[cur].y - nodes[nxt].y), cur);
            if (after < 0)
                return false;
            cur = nxt;
            nxt = adj[cur][after];
            curSlot = after;
            if (cur == from && nxt == to)
                return true;
        }
        return false;
    }
    // the lowest of the leftmost nodes, left heading south: the slot of the outer walk's first neighbour
    int start_slot(int& start)
    {
        start = 0;
        for (size_t k = 1; k < nodes.size(); ++k)
            if (nodes[k].x < nodes[start].x - eps || (std::fabs(nodes[k].x - nodes[start].x) <= eps && nodes[k].y < nodes[start].y))
                start = (int)k;
        return next_of(start, make_double2(0.0, 1.0), -1);
    }
    // a hole judged as soon as its face is known: bounded, its inside in neither operand, then merge_union's own test after `drop`
    bool face_is_hole(Ring2& face, const Ring2& A, const Ring2& B) const
    {
        if (face.size() < 3 || signed_area(face) >= 0)
            return false;
        bool found = false;
        double2 probe = make_double2(0, 0);
        for (size_t i = 0; i < face.size() && !found; ++i)
        {
            const double2 p = face[i], q = face[(i + 1) % face.size()];
            const double dx = q.x - p.x, dy = q.y - p.y, len = std::hypot(dx, dy);
            if (len <= eps)
                continue;
            for (double off = 1e-3; off >= 1e-7 && !found; off *= 0.1)
            {
                probe = make_double2(0.5 * (p.x + q.x) + off * len * (dy / len), 0.5 * (p.y + q.y) - off * len * (dx / len));
                found = in_ring(probe, face, false);
            }
        }
        if (!found || in_ring(probe, A, true) || in_ring(probe, B, true))
            return false;
        drop(face);
        return face.size() >= 3 && simple(face);
    }
};

// union_pair.  A, B: both operands in one frame, oriented
static Out pair(Ring2 A, Ring2 B)
{
    Out out;
    out.flags = CAPE_UNION_SERVED | CAPE_UNION_UNCHANGED;
    out.ring = A;
    out.area = area_of(A);
    Arrangement G;
    const auto hosted = [&](uint32_t f) {
        Out o;
        o.flags = f;
        o.nNodes = (int)G.nodes.size();
        return o;
    };
    if (!G.build(A, B))
        return hosted(CAPE_UNION_HOST_CAPACITY);
    out.nNodes = (int)G.nodes.size();
    if (G.capacity)
        return hosted(CAPE_UNION_HOST_CAPACITY);
    Ring2 outer;
    bool newHole = false;
    if (G.nodes.size() >= 3)
    {
        int start = 0;
        const int first = G.start_slot(start);
        if (first >= 0)
        {
            if (!G.walk(start, first, outer))
                return hosted(CAPE_UNION_HOST_CAPACITY);
            Ring2 face;
            for (size_t a = 0; a < G.nodes.size() && !outer.empty(); ++a)
                for (size_t k = 0; k < G.adj[a].size(); ++k)
                {
                    if ((G.seen[a] >> k) & 1u)
                        continue;
                    if (!G.walk((int)a, (int)k, face))
                        return hosted(CAPE_UNION_HOST_CAPACITY);
                    if (G.face_is_hole(face, A, B))
                        newHole = true;
                }
        }
    }
    if (G.ambiguous)
        return hosted(CAPE_UNION_HOST_AMBIGUOUS);
    if (!outer.empty())
        drop(outer);
    const double outerArea = outer.size() >= 3 ? std::abs(signed_area(outer)) : 0.0;
    const double areaA = std::abs(signed_area(A)), areaB = std::abs(signed_area(B));
    bool disjoint = outer.size() >= 3 && (left_out(A, outer) || left_out(B, outer)), rule = false;
    if (outerArea + 1e-9 * cape::umax(areaA, areaB) < cape::umax(areaA, areaB))
    {
        disjoint = rule = true;
        if (areaA >= areaB)
        {
            out.flags = CAPE_UNION_SERVED | CAPE_UNION_DISJOINT;
            simplify(out.ring, out.area);
            return out;
        }
        outer = B;
    }
    if (outer.size() < 3 || !simple(outer))
    {
        out.flags |= disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u;
        return out;
    }
    if (!rule && newHole)
        return hosted(CAPE_UNION_HOST_NEW_HOLE);
    if (outer.size() > 1 && outer.front().x == outer.back().x && outer.front().y == outer.back().y)
        outer.pop_back();
    orient(outer);
    out.flags = CAPE_UNION_SERVED | (disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u);
    out.ring = outer;
    simplify(out.ring, out.area);
    return out;
}
} // namespace seq

// one pair through the host class (merge_union with its info) and through seq::pair: flags, ring and area bit for bit
static long compare_pair(const std::vector<vector2>& a, const std::vector<vector2>& b, long counts[4], seq::Out* port = nullptr)
{
    const vector3 X(1, 0, 0), Y(0, 1, 0), C0(0, 0, 0);
    ref::Polygon pa(a, {}, X, Y, C0);
    const ref::Polygon pb(b, {}, X, Y, C0);
    std::vector<double2> A, B;
    for (const vector2& p : pa.boundary())
        A.push_back(make_double2(p[0], p[1]));
    for (const vector2& p : pb.boundary())
        B.push_back(make_double2(p[0], p[1]));
    ref::Polygon::MergeInfo info;
    const bool merged = pa.merge_union(pb, &info);
    const seq::Out mine = seq::pair(A, B);
    if (port)
        *port = mine;
    if (mine.flags & (CAPE_UNION_HOST_CAPACITY | CAPE_UNION_HOST_AMBIGUOUS))
    {
        ++counts[3];
        return 0;
    }
    if (!pa.interior_rings().empty())
    {
        ++counts[2];
        return mine.flags == CAPE_UNION_HOST_NEW_HOLE ? 0 : 1;
    }
    const uint32_t want = CAPE_UNION_SERVED | (merged ? 0u : (uint32_t)CAPE_UNION_UNCHANGED) | (info.disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u);
    counts[info.disjoint ? 1 : 0]++;
    bool eq = mine.flags == want && mine.ring.size() == pa.boundary().size() && same_bits(mine.area, pa.get_area());
    for (size_t i = 0; eq && i < mine.ring.size(); ++i)
        eq = same_bits(mine.ring[i].x, pa.boundary()[i][0]) && same_bits(mine.ring[i].y, pa.boundary()[i][1]);
    return eq ? 0 : 1;
}

// ---- The long pairs of tests/test_map_union_host.py (LONG_PAIRS, with its generators restated), and the two 128-gons of HAND_BUILT:
// operands of more than 64 vertices.  Each pair goes through the host class and through seq::pair like the pairs above; the port's
// flags, vertex count and node count are printed and checked against the table.  The node counts are the reference for the device's
// n_nodes (LONG_NODES in the Python table); where the arithmetic is plain it is given.
namespace named {
using Ring = std::vector<vector2>;
static Ring rect(double x0, double x1, double y0, double y1) { return {{x0, y0}, {x0, y1}, {x1, y1}, {x1, y0}}; }
static Ring ngon(int n, double r, double cx, double cy, double phase)
{
    Ring o;
    for (int i = 0; i < n; ++i)
    {
        const double t = phase + 2 * M_PI * i / n;
        o.emplace_back(cx + r * std::cos(t), cy + r * std::sin(t));
    }
    return o;
}
static Ring comb(int teeth = 30, double pitch = 100, double width = 50, double spine = 100, double length = 3000)
{
    Ring o {{0, 0}, {(teeth - 1) * pitch + width, 0}};
    for (int k = teeth - 1; k >= 0; --k)
    {
        const double x = k * pitch;
        o.insert(o.end(), {{x + width, spine}, {x + width, length}, {x, length}, {x, spine}});
    }
    return o;
}
static Ring cog(double even = 1000, double odd = 700, int n = 128)
{
    Ring o;
    for (int i = 0; i < n; ++i)
    {
        const double t = 2 * M_PI * i / n, r = i % 2 == 0 ? even : odd;
        o.emplace_back(r * std::cos(t), r * std::sin(t));
    }
    return o;
}
static Ring subdivided(const Ring& ring, int parts = 32)
{
    Ring o;
    for (size_t i = 0; i < ring.size(); ++i)
        for (int k = 0; k < parts; ++k)
        {
            const vector2 &a = ring[i], &b = ring[(i + 1) % ring.size()];
            o.emplace_back(a[0] + (b[0] - a[0]) * k / parts, a[1] + (b[1] - a[1]) * k / parts);
        }
    return o;
}
static Ring saw(int teeth = 60)
{
    Ring o {{0, 0}, {100.0 * teeth, 0}};
    for (int k = teeth; k >= 1; --k)
        o.insert(o.end(), {{100.0 * k, 1000}, {100.0 * (k - 0.5), 2000}});
    o.emplace_back(0, 1000);
    return o;
}
// (p - c) M + c for row vectors
static Ring about(const Ring& ring, double cx, double cy, double m00, double m01, double m10, double m11)
{
    Ring o;
    for (const vector2& p : ring)
        o.emplace_back((p[0] - cx) * m00 + (p[1] - cy) * m10 + cx, (p[0] - cx) * m01 + (p[1] - cy) * m11 + cy);
    return o;
}
static Ring mirrored(const Ring& ring, double dx, double dy)
{
    Ring o;
    for (const vector2& p : ring)
        o.emplace_back(p[0] + dx, -p[1] + dy);
    return o;
}
static Ring rake()
{
    Ring o;
    for (const vector2& p : comb(3, 100, 50, 100, 3200))
        o.emplace_back(p[1] - 150, p[0] + 1000);
    Ring extra;
    for (int k = 1; k < 18; ++k)
        extra.emplace_back(-150.0, 1000 + 10.0 * k);
    o.insert(o.begin() + 1, extra.begin(), extra.end());
    return o;
}
static Ring snag(int teeth = 32)
{
    Ring o {{-100, -100}, {130, -100}, {130, 1000}, {30, 1000}, {30, 505}, {-8, 500}, {30, 495}, {30, 0},
            {0, 0}, {0, 480}, {-9, 490}, {-9, 510}, {0, 520}, {0, 1000}, {-50, 1050}};
    const double pitch = 600.0 / teeth;
    for (int k = 0; k < teeth; ++k)
    {
        o.emplace_back(-200.0, 1000 - pitch * (k + 0.5));
        if (k + 1 < teeth)
            o.emplace_back(-100.0, 1000 - pitch * (k + 1));
    }
    return o;
}
static Ring snag_plate(int teeth = 32)
{
    Ring o {{-50, -80}, {-50, 380}, {-150, 380}};
    const double pitch = 460.0 / teeth;
    for (int k = 0; k < teeth; ++k)
        o.insert(o.end(), {{-300.0, 380 - pitch * (k + 0.5)}, {-150.0, 380 - pitch * (k + 1)}});
    return o;
}
struct Pair
{
    const char* name;
    Ring a, b;
    uint32_t flags; // the port's
    int count;      // vertices of the served ring, -1: none
    int nodes;
};
static std::vector<Pair> table()
{
    const Ring pinch8 {{0, 0}, {400, 400}, {800, 0}, {800, 800}, {400, 400}, {0, 800}};
    const Ring pinch10 {{0, 0}, {400, 400}, {800, 0}, {900, 400}, {400, 400}, {800, 800}, {400, 900}, {400, 400}, {0, 800}};
    const Ring turned = about(pinch8, 400, 400, .6, .8, -.8, .6);
    const uint32_t S = CAPE_UNION_SERVED, H = CAPE_UNION_HOST_NEW_HOLE, C = CAPE_UNION_HOST_CAPACITY;
    return {
        {"two 128-gons", ngon(128, 1000, 0, 0, 0.01), ngon(128, 1000, 700, 100, 0.01), S, 18, 258},             // 256 vertices, 2 crossings
        {"half-step 128-gons", ngon(128, 1000, 0, 0, 0), ngon(128, 1000, 0, 0, M_PI / 128), S, 16, 512},        // 256 vertices, every edge crossed twice
        {"mirrored cogs", cog(), mirrored(cog(), 150, 40), S, 188, 386},
        {"half-step cogs", cog(), cog(700, 1000), S, 256, 384},                                                  // 256 vertices, every edge crossed once
        {"subdivided squares", subdivided(rect(0, 400, 0, 400)), subdivided(rect(200, 600, 200, 600)), S, 8, 254}, // 256 vertices, two shared
        {"comb and foot", comb(), rect(-50, 100, -50, 50), S, 124, 122 + 4 + 2},
        {"saw and bar", saw(), rect(100, 5900, 500, 1500), S, 122, 123 + 4 + 116},
        {"comb of 9 and bar", comb(9), rect(-100, 1000, 1500, 1600), H, -1, 38 + 4 + 36},                      // each tooth crossed 4 times
        {"comb of 10 and bar", comb(10), rect(-100, 1100, 1500, 1600), H, -1, 42 + 4 + 40},
        {"comb of 30 and bar", comb(), rect(-100, 3100, 1500, 1600), H, -1, 122 + 4 + 120},
        {"pinched rings, degree 8", pinch8, turned, S, 16, 15},   // 5 + 5 distinct vertices, the centre shared, 6 crossings
        {"pinched rings, degree 10", pinch10, turned, C, -1, 15}, // 7 + 5 distinct vertices, the centre shared, 4 crossings
        {"comb and rake, 513 nodes", comb(), rake(), C, -1, 122 + 31 + 360},
        {"snag at candidate edge 127", snag(), snag_plate(), S, 159, 177}, // (the last tooth's lower edge runs down to the corner through the plate's teeth)
    };
}
} // namespace named

int main()
{
    std::mt19937_64 gen(2024);
    std::normal_distribution<double> normal(0.0, 1.0);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    long bad = 0;
    auto unit3 = [&](double* v) {
        double n = 0;
        for (int k = 0; k < 3; ++k)
            v[k] = normal(gen), n += v[k] * v[k];
        for (int k = 0; k < 3; ++k)
            v[k] /= std::sqrt(n);
    };
    auto frame = [&](cape::UnionFrame& f) {
        double n[3];
        unit3(n);
        const auto axes = ref::get_plane_coordinate_system(vector3(n[0], n[1], n[2]));
        for (int k = 0; k < 3; ++k)
            f.x[k] = axes.first[k], f.y[k] = axes.second[k], f.c[k] = 3000 * normal(gen);
    };
    auto point = [&](double scale) { return make_double2(scale * (2 * uni(gen) - 1), scale * (2 * uni(gen) - 1)); };
    auto v2 = [](const double2& p) { return vector2(p.x, p.y); };

    // ---- Polygon::project, vertex by vertex (the class orients the result: compare in either direction)
    long nProject = 0;
    for (int c = 0; c < 20000; ++c)
    {
        cape::UnionFrame from, to;
        frame(from);
        frame(to);
        const int n = 3 + (int)(uni(gen) * 20);
        std::vector<vector2> ring;
        for (int i = 0; i < n; ++i)
            ring.push_back(v2(point(2000)));
        const ref::Polygon poly(ring, {}, vector3(from.x[0], from.x[1], from.x[2]), vector3(from.y[0], from.y[1], from.y[2]),
                                vector3(from.c[0], from.c[1], from.c[2]));
        const ref::Polygon out = poly.project(vector3(to.x[0], to.x[1], to.x[2]), vector3(to.y[0], to.y[1], to.y[2]), vector3(to.c[0], to.c[1], to.c[2]));
        std::vector<double2> mine;
        for (const vector2& p : poly.boundary())
            mine.push_back(cape::union_project(make_double2(p[0], p[1]), from, to));
        bool fwd = true, rev = true;
        for (int i = 0; i < n; ++i)
        {
            fwd = fwd && same_bits(mine[i].x, out.boundary()[i][0]) && same_bits(mine[i].y, out.boundary()[i][1]);
            rev = rev && same_bits(mine[n - 1 - i].x, out.boundary()[i][0]) && same_bits(mine[n - 1 - i].y, out.boundary()[i][1]);
        }
        bad += !(fwd || rev);
        ++nProject;
    }

    // ---- param_on and the proper crossing (rings_union_outer's lambdas, restated)
    long nOn = 0, nCross = 0, nCuts = 0;
    for (int c = 0; c < 400000; ++c)
    {
        const double scale = std::pow(10.0, 4 * uni(gen));
        const double eps = 1e-9 * std::max(1.0, scale);
        double2 sa = point(scale), sb = point(scale), ua = point(scale), ub = point(scale);
        if (c % 4 == 1) // an endpoint on (or within a few eps of) the other segment
        {
            const double t = uni(gen);
            ua = make_double2(sa.x + t * (sb.x - sa.x) + eps * normal(gen), sa.y + t * (sb.y - sa.y) + eps * normal(gen));
        }
        if (c % 4 == 2) // a shared end within eps
            ua = make_double2(sa.x + eps * normal(gen), sa.y + eps * normal(gen));
        auto same = [&](const vector2& a, const vector2& b) { return std::abs(a[0] - b[0]) <= eps && std::abs(a[1] - b[1]) <= eps; };
        auto cross2 = [](const vector2& o, const vector2& a, const vector2& b) {
            return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0]);
        };
        auto param_on = [&](const vector2& a, const vector2& b, const vector2& p, double& t) {
            const double dx = b[0] - a[0], dy = b[1] - a[1];
            const double len2 = dx * dx + dy * dy;
            const double cr = cross2(a, b, p);
            if (std::abs(cr) > eps * std::sqrt(len2))
                return false;
            t = ((p[0] - a[0]) * dx + (p[1] - a[1]) * dy) / len2;
            return t > 0 && t < 1 && !same(p, a) && !same(p, b);
        };
        double tr = 0, tm = 0;
        const bool r = param_on(v2(sa), v2(sb), v2(ua), tr), m = cape::union_param_on(sa, sb, ua, eps, tm);
        bad += r != m || (r && !same_bits(tr, tm));
        nOn += r;
        ++nCuts;
        // the crossing
        const double d1 = cross2(v2(ua), v2(ub), v2(sa)), d2 = cross2(v2(ua), v2(ub), v2(sb));
        const double d3 = cross2(v2(sa), v2(sb), v2(ua)), d4 = cross2(v2(sa), v2(sb), v2(ub));
        const bool proper = ((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0));
        double ts = 0, tu = 0;
        bool ks = false, ku = false;
        const bool mine = cape::union_crossing(sa, sb, ua, ub, eps, ts, ks, tu, ku);
        bad += mine != proper;
        if (proper && mine)
        {
            const double rs = d1 / (d1 - d2), ru = d3 / (d3 - d4);
            const vector2 x {sa.x + rs * (sb.x - sa.x), sa.y + rs * (sb.y - sa.y)};
            bad += !same_bits(rs, ts) || !same_bits(ru, tu) || ks != (!same(x, v2(sa)) && !same(x, v2(sb))) ||
                   ku != (!same(x, v2(ua)) && !same(x, v2(ub)));
            const double2 cp = cape::union_cut_point(sa, sb, ts);
            bad += !same_bits(cp.x, x[0]) || !same_bits(cp.y, x[1]);
            ++nCross;
        }
    }

    // ---- next_of's angle (restated), and the guard band: set exactly where an unwrapped angle is within 1e-10 of the wrap line
    long nAngles = 0, nBand = 0;
    for (int c = 0; c < 400000; ++c)
    {
        const double bx = normal(gen), by = normal(gen);
        double dx = normal(gen), dy = normal(gen);
        if (c % 8 == 1) // straight back: the wrap line itself
            dx = bx, dy = by;
        if (c % 8 == 2) // a hair off it
            dx = bx + 1e-11 * normal(gen), dy = by + 1e-11 * normal(gen);
        const double ba = std::atan2(by, bx);
        double ang = std::atan2(dy, dx) - ba;
        bool nearLine = std::abs(ang - 1e-12) < 1e-10;
        while (ang <= 1e-12)
        {
            ang += 2 * M_PI;
            nearLine = nearLine || std::abs(ang - 1e-12) < 1e-10;
        }
        bool amb = false;
        const double mine = cape::union_angle(dy, dx, ba, false, amb);
        bad += !same_bits(mine, ang) || amb != nearLine;
        bool ambFrom = false;
        bad += !same_bits(cape::union_angle(dy, dx, ba, true, ambFrom), ang) || ambFrom;
        nBand += amb;
        ++nAngles;
    }

    // ---- segment_distance2, segments_intersect, the point-in-ring edge test, drop_collinear's test
    long nDist = 0, nMeet = 0, nInside = 0, nDropped = 0;
    for (int c = 0; c < 300000; ++c)
    {
        double2 p = point(1000), a = point(1000), b = point(1000), q = point(1000);
        if (c % 5 == 1)
            b = a; // a degenerate segment
        if (c % 5 == 2)
            p = make_double2(a.x + 0.5 * (b.x - a.x), a.y + 0.5 * (b.y - a.y)); // on the segment
        if (c % 5 == 3)
            q = a; // a shared endpoint
        bad += !same_bits(cape::union_segment_distance2(p, a, b), ref::segment_distance2(v2(p), v2(a), v2(b)));
        const bool meet = ref::segments_intersect(v2(a), v2(b), v2(p), v2(q));
        bad += cape::union_segments_intersect(a, b, p, q) != meet;
        nMeet += meet;
        ++nDist;
    }
    for (int c = 0; c < 20000; ++c)
    {
        const int n = 3 + (int)(uni(gen) * 30);
        std::vector<vector2> ring;
        std::vector<double2> mine;
        for (int i = 0; i < n; ++i)
        {
            const double t = 2 * M_PI * (i + 0.8 * uni(gen)) / n, r = 500 + 500 * uni(gen);
            double2 v = make_double2(std::round(r * std::cos(t)), std::round(r * std::sin(t)));
            if (i >= 2 && c % 3 == 0 && uni(gen) < 0.3) // a vertex on the line of the two before it
                v = make_double2(2 * mine[i - 1].x - mine[i - 2].x, 2 * mine[i - 1].y - mine[i - 2].y);
            mine.push_back(v);
            ring.push_back(v2(v));
        }
        for (int k = 0; k < 20; ++k)
        {
            double2 p = point(1100);
            if (k % 4 == 1)
                p = mine[k % n]; // a vertex
            if (k % 4 == 2)
                p = make_double2(0.5 * (mine[0].x + mine[1].x), 0.5 * (mine[0].y + mine[1].y));
            for (int closed = 0; closed < 2; ++closed)
            {
                bool on = false, inside = false;
                for (int i = 0; i < n; ++i)
                {
                    const int e = cape::union_point_edge(p, mine[i], mine[i == 0 ? n - 1 : i - 1]);
                    on = on || e == 2;
                    inside = inside != (e == 1);
                }
                const bool got = on ? closed != 0 : inside;
                const bool want = ref::point_in_ring(v2(p), ring, closed != 0);
                bad += got != want;
                nInside += want;
            }
        }
        // drop_collinear: the host's loop with the device's test in its place
        std::vector<vector2> dropped = ring;
        ref::drop_collinear(dropped);
        std::vector<double2> r = mine;
        bool changed = true;
        while (changed && r.size() > 3)
        {
            changed = false;
            for (size_t i = 0; i < r.size() && r.size() > 3; ++i)
                if (cape::union_collinear(r[(i + r.size() - 1) % r.size()], r[i], r[(i + 1) % r.size()]))
                {
                    r.erase(r.begin() + static_cast<long>(i));
                    changed = true;
                    --i;
                }
        }
        bool eq = r.size() == dropped.size();
        for (size_t i = 0; eq && i < r.size(); ++i)
            eq = same_bits(r[i].x, dropped[i][0]) && same_bits(r[i].y, dropped[i][1]);
        bad += !eq;
        nDropped += (long)(mine.size() - r.size());
    }
    // is_approx3
    for (int c = 0; c < 100000; ++c)
    {
        double a[3], b[3];
        unit3(a);
        for (int k = 0; k < 3; ++k)
            b[k] = a[k] * (1 + (c % 2 ? 1e-12 : 1e-13) * normal(gen));
        const double e0 = a[0] - b[0], e1 = a[1] - b[1], e2 = a[2] - b[2];
        const double diff = (e0 * e0 + e1 * e1) + e2 * e2;
        const double na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], nb = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
        bad += cape::union_is_approx3(a, b) != (diff <= 1e-12 * 1e-12 * std::min(na, nb));
    }
    // ---- whole pairs: stars of 8 and 24 vertices, squares in every relation, a C shape closed by a bar
    long pairCounts[4] = {0, 0, 0, 0}, nPairs = 0;
    auto star = [&](int n, double cx, double cy) {
        std::vector<double> t(n);
        for (double& v : t)
            v = 2 * M_PI * uni(gen);
        std::sort(t.begin(), t.end());
        std::vector<vector2> r;
        for (int i = 0; i < n; ++i)
        {
            const double rad = 1000 * (0.5 + 0.5 * uni(gen));
            r.emplace_back(cx + rad * std::cos(t[i]), cy + rad * std::sin(t[i]));
        }
        return r;
    };
    auto rect = [](double x0, double x1, double y0, double y1) { return std::vector<vector2> {{x0, y0}, {x0, y1}, {x1, y1}, {x1, y0}}; };
    for (int c = 0; c < 3000; ++c, ++nPairs)
        bad += compare_pair(star(c % 2 ? 8 : 24, 0, 0), star(c % 2 ? 8 : 24, 1200 * uni(gen) - 600, 1200 * uni(gen) - 600), pairCounts);
    for (int c = 0; c < 3000; ++c, ++nPairs)
    {
        // integer rectangles: shared edges, T junctions, containment, disjoint pieces, equal rings
        auto r = [&] { return std::floor(8 * uni(gen)) * 100; };
        const double x0 = r(), y0 = r(), x1 = r(), y1 = r();
        bad += compare_pair(rect(x0, x0 + 100 + r(), y0, y0 + 100 + r()), rect(x1, x1 + 100 + r(), y1, y1 + 100 + r()), pairCounts);
    }
    bad += compare_pair({{0, 0}, {3000, 0}, {3000, 1000}, {1000, 1000}, {1000, 2000}, {3000, 2000}, {3000, 3000}, {0, 3000}},
                        rect(2500, 4000, 0, 3000), pairCounts);
    ++nPairs;
    // ---- the named long pairs
    long namedCounts[4] = {0, 0, 0, 0};
    for (const named::Pair& c : named::table())
    {
        seq::Out port;
        const long differs = compare_pair(c.a, c.b, namedCounts, &port);
        const int count = (port.flags & CAPE_UNION_SERVED) ? (int)port.ring.size() : -1;
        const bool asTable = port.flags == c.flags && count == c.count && port.nNodes == c.nodes;
        std::printf("%-27s flags 0x%02x  vertices %3d  nodes %3d%s%s\n", c.name, port.flags, count, port.nNodes,
                    differs ? "  DIFFERS from the host class" : "", asTable ? "" : "  NOT the table's");
        bad += differs + !asTable;
    }
    std::printf("pairs: %ld (served %ld, disjoint %ld, new hole %ld, capacity or ambiguous %ld)\n", nPairs, pairCounts[0], pairCounts[1],
                pairCounts[2], pairCounts[3]);
    bad += pairCounts[3] != 0 || pairCounts[0] < 1000 || pairCounts[1] < 10 || pairCounts[2] < 10;
    std::printf("project: %ld rings; param_on: %ld of %ld on a segment; crossings: %ld; angles: %ld (%ld inside the band); distances: %ld, "
                "%ld segment pairs meet; %ld points inside; %ld collinear vertices dropped; mismatches: %ld\n",
                nProject, nOn, nCuts, nCross, nAngles, nBand, nDist, nMeet, nInside, nDropped, bad);
    return bad == 0 && nOn > 1000 && nCross > 1000 && nBand > 1000 && nMeet > 1000 && nDropped > 1000 ? 0 : 1;
}

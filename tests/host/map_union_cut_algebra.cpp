// The cut mode of csrc/cape_map_union.h (union_arrange, union_pair_rings<true>) one lane at a time, compared bit for bit with
// host/boundary_polygon.cpp's merge_union and simplify on map polygons whose holes the detection covers in part, under the address and
// undefined-behaviour sanitizers.  A stand-alone program.  tests/host/map_union_holes_algebra.cpp is included as text with its main
// renamed, as that file includes tests/host/map_union_algebra.cpp: together they bring the host class, the per-lane functions of the
// device header, the arrangement of every mode (seq::Arrangement: the rank sort, node_of, link, next_of with its guard band, the
// walks), the wave-shaped loops (seq::simple, seq::drop, seq::dp_candidate), the ring generators, and holes::pair -- the one pair
// function of the modes with rings, as union_pair_rings is on the device -- with its helpers (orient_hole, area_holed, vertices_of,
// simplify_holed).  New here, in the device's order of statements: cut::arrange, which is union_arrange -- one arrangement per
// call, built from ITS operands (its own scale and eps, segment list, cuts, nodes, start node and first slot), the outer face walked
// and dropped, every other face tested by the rule (0: in neither operand, 1: in or on the first and not in or on the second) on the
// probe point, then drop_collinear, >= 3 vertices, simple and -- rule 1 -- more than `tiny`, oriented like add_hole and appended
// while it fits, counted either way.  holes::pair runs it through cut::pieces with rule 1 on (a partly covered hole, the detection)
// and the tiny of the FIRST pair of operands, the pieces following the rings stored so far; the capacities are judged at the end.
// Rule 0 is the pair function's own first arrangement restated: cut::compare runs cut::arrange(A, B, rule 0) beside every pair and
// holds its count of faces against the pair's new holes.  What needs the wave -- the second sorted cut list in the intersection's
// heights, the second outer face in L.face, the barriers -- is tests/test_gpu_map_union_cut.py's.  Build and run from the repository
// root:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Itests/host/hip_stub -Irgb-d-slam_amd/csrc -Irgb-d-slam_amd/host \
//       -Irgb-d-slam_amd/host/compat -o map_union_cut_algebra.exe tests/host/map_union_cut_algebra.cpp && ./map_union_cut_algebra.exe
#define MAP_UNION_HOLES_ALGEBRA_MAIN map_union_holes_algebra_main
#include "map_union_holes_algebra.cpp"

namespace cut {
using holes::kHoleVertices;
using holes::kHoles;
using holes::orient_hole;
using holes::Out;
using seq::drop;
using seq::in_ring;
using seq::Ring2;
using seq::signed_area;
using seq::simple;

// ---- the cut mode's own
static int largestSecond = 0; // nodes of the largest second arrangement met

// the test of a walked face (union_arrange): bounded, the probe point by the rule, then merge_union's / carry_hole's own filter
static bool face_passes(const seq::Arrangement& G, Ring2& face, const Ring2& A, const Ring2& B, int rule, double tiny)
{
    if (face.size() < 3 || signed_area(face) >= 0)
        return false;
    bool found = false;
    double2 probe = make_double2(0, 0);
    for (size_t i = 0; i < face.size() && !found; ++i)
    {
        const double2 p = face[i], q = face[(i + 1) % face.size()];
        const double dx = q.x - p.x, dy = q.y - p.y, len = std::hypot(dx, dy);
        if (len <= G.eps)
            continue;
        for (double off = 1e-3; off >= 1e-7 && !found; off *= 0.1)
        {
            probe = make_double2(0.5 * (p.x + q.x) + off * len * (dy / len), 0.5 * (p.y + q.y) - off * len * (dx / len));
            found = in_ring(probe, face, false);
        }
    }
    if (!found)
        return false;
    const bool inA = in_ring(probe, A, true), inB = in_ring(probe, B, true);
    if (rule == 0 ? (inA || inB) : (!inA || inB))
        return false;
    drop(face);
    return face.size() >= 3 && simple(face) && (rule == 0 || std::abs(signed_area(face)) > tiny);
}

// union_arrange.  Returns 0 or the bits that end the pair; the faces that pass go to `stored` while they fit (count, vertices)
static uint32_t arrange(const Ring2& A, const Ring2& B, int rule, double tiny, Ring2& outer, std::vector<Ring2>& stored, int& count, int& vertices,
                        int& nNodes)
{
    seq::Arrangement G; // everything derived from A and B: nothing is carried over from another arrangement
    outer.clear();
    if (!G.build(A, B))
        return CAPE_UNION_HOST_CAPACITY;
    nNodes = (int)G.nodes.size();
    if (G.capacity)
        return CAPE_UNION_HOST_CAPACITY;
    if (G.nodes.size() >= 3)
    {
        int start = 0;
        const int first = G.start_slot(start);
        if (first >= 0)
        {
            if (!G.walk(start, first, outer)) // (marks its edges seen; rule 1 drops the ring)
                return CAPE_UNION_HOST_CAPACITY;
            Ring2 face;
            for (size_t a = 0; a < G.nodes.size() && !outer.empty(); ++a)
                for (size_t k = 0; k < G.adj[a].size(); ++k)
                {
                    if ((G.seen[a] >> k) & 1u)
                        continue;
                    if (!G.walk((int)a, (int)k, face))
                        return CAPE_UNION_HOST_CAPACITY;
                    if (face_passes(G, face, A, B, rule, tiny))
                    {
                        if (count < kHoles && vertices + (int)face.size() <= kHoleVertices)
                        {
                            orient_hole(face);
                            stored.push_back(face);
                        }
                        ++count;
                        vertices += (int)face.size();
                    }
                }
        }
    }
    return G.ambiguous ? (uint32_t)CAPE_UNION_HOST_AMBIGUOUS : 0u;
}

// the second arrangement of holes::pair's cut mode: union_arrange(hole, detection, rule 1)
static uint32_t pieces(const Ring2& hole, const Ring2& B, double tiny, std::vector<Ring2>& hs, int& nHoles, int& holeVertices)
{
    Ring2 outer2; // walked for its edges' marks only
    int nodes2 = 0;
    const uint32_t bits = arrange(hole, B, 1, tiny, outer2, hs, nHoles, holeVertices, nodes2);
    largestSecond = std::max(largestSecond, nodes2);
    return bits;
}

// counts: served without a cut hole, served with HOLE_PIECES, capacity on both sides, handed away by the port alone, differing
enum { kPlain, kPieces, kCapacity, kHandedAway, kCounts };

// one pair through the host class and through the port: flags (as the twins derive them), every ring, the area, the counts.
// `handsAway`: the answer the port is expected to give where the host class serves (0: none).  `lengths`: the ring lengths.
static long compare(const char* name, const named::Ring& a, const std::vector<named::Ring>& holesA, const named::Ring& b, long counts[kCounts],
                    uint32_t handsAway = 0, std::vector<size_t>* lengths = nullptr)
{
    const vector3 X(1, 0, 0), Y(0, 1, 0), C0(0, 0, 0);
    ref::Polygon pa(a, holesA, X, Y, C0);
    const ref::Polygon pb(b, {}, X, Y, C0);
    auto ring2 = [](const std::vector<vector2>& r) {
        Ring2 o;
        for (const vector2& p : r)
            o.push_back(make_double2(p[0], p[1]));
        return o;
    };
    const Ring2 A = ring2(pa.boundary()), B = ring2(pb.boundary());
    std::vector<Ring2> H;
    size_t before = 0;
    for (const auto& h : pa.interior_rings())
    {
        H.push_back(ring2(h));
        before += h.size();
    }
    ref::Polygon::MergeInfo info;
    const bool merged = pa.merge_union(pb, &info);
    const Out mine = holes::pair(A, B, H, pieces);
    // rule 0: where the pair got as far as its interior rings with every face of the first arrangement a new hole, union_arrange finds them
    {
        Ring2 outer0;
        std::vector<Ring2> faces0;
        int n0 = 0, vertices0 = 0, nodes0 = 0;
        const uint32_t bits0 = arrange(A, B, 0, 0.0, outer0, faces0, n0, vertices0, nodes0);
        if ((mine.flags & CAPE_UNION_SERVED) && !(mine.flags & (CAPE_UNION_UNCHANGED | CAPE_UNION_DISJOINT)) && (bits0 != 0 || (unsigned)n0 != mine.holesNew))
        {
            std::printf("DIFFERS: %s: rule 0 finds %d faces (bits %#x), the pair %u new holes\n", name, n0, bits0, mine.holesNew);
            return 1;
        }
    }
    const bool fits = pa.boundary().size() <= CAPE_MAP_MAX_RING && pa.interior_rings().size() <= CAPE_MAP_MAX_HOLES;
    uint32_t want;
    if (!fits || (merged ? info.holeVertices : before) > CAPE_MAP_UNION_HOLE_VERTICES)
        want = CAPE_UNION_HOST_CAPACITY;
    else
        want = CAPE_UNION_SERVED | (merged ? 0u : (uint32_t)CAPE_UNION_UNCHANGED) | (info.disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u) |
               (pa.interior_rings().empty() ? 0u : (uint32_t)CAPE_UNION_HOLES) | (info.holeCut ? (uint32_t)CAPE_UNION_HOLE_PIECES : 0u);
    if (lengths)
    {
        lengths->clear();
        lengths->push_back(pa.boundary().size());
        for (const auto& h : pa.interior_rings())
            lengths->push_back(h.size());
    }
    if ((want & CAPE_UNION_SERVED) && !(mine.flags & CAPE_UNION_SERVED))
    {
        ++counts[kHandedAway];
        const bool expected = handsAway != 0 && mine.flags == handsAway;
        if (!expected)
            std::printf("HANDED AWAY: %s: port flags %#x, host class %#x\n", name, mine.flags, want);
        return expected ? 0 : 1;
    }
    if (handsAway != 0)
    {
        std::printf("NOT HANDED AWAY: %s: port flags %#x, expected %#x\n", name, mine.flags, handsAway);
        return 1;
    }
    ++counts[want == CAPE_UNION_HOST_CAPACITY ? kCapacity : (want & CAPE_UNION_HOLE_PIECES) ? kPieces : kPlain];
    bool eq = mine.flags == want;
    if (eq && (want & CAPE_UNION_SERVED))
    {
        eq = mine.rings.size() == 1 + pa.interior_rings().size() && same_bits(mine.area, pa.get_area()) && mine.holesNew == info.holesNew &&
             mine.holesKept == info.holesKept && mine.holesCovered == info.holesCovered;
        for (size_t k = 0; eq && k < mine.rings.size(); ++k)
        {
            const auto& theirs = k == 0 ? pa.boundary() : pa.interior_rings()[k - 1];
            eq = mine.rings[k].size() == theirs.size();
            for (size_t i = 0; eq && i < theirs.size(); ++i)
                eq = same_bits(mine.rings[k][i].x, theirs[i][0]) && same_bits(mine.rings[k][i].y, theirs[i][1]);
        }
    }
    if (!eq)
        std::printf("DIFFERS: %s: port flags %#x, host class %#x, rings %zu / %zu\n", name, mine.flags, want, mine.rings.size(),
                    1 + pa.interior_rings().size());
    return eq ? 0 : 1;
}
} // namespace cut

int main()
{
    using named::Ring;
    using named::rect;
    long bad = 0, counts[cut::kCounts] = {0, 0, 0, 0};
    // ---- the table of tests/map_union_cut_cases.py
    const Ring cShape = {{0, 0}, {3000, 0}, {3000, 1000}, {1000, 1000}, {1000, 2000}, {3000, 2000}, {3000, 3000}, {0, 3000}};
    const Ring map = rect(0, 1000, 0, 1000), mid = rect(400, 500, 400, 500);
    const Ring fork = {{300, 300}, {300, 1200}, {700, 1200}, {700, 300}, {600, 300}, {600, 1100}, {400, 1100}, {400, 300}};
    std::vector<Ring> eight;
    for (int k = 0; k < 8; ++k)
        eight.push_back(rect(100 + 90 * k, 150 + 90 * k, 100, 150));
    auto some_of_eight = [&](int n) {
        std::vector<Ring> hs(eight.begin(), eight.begin() + n);
        hs.push_back(rect(200, 800, 400, 500));
        return hs;
    };
    auto shifted = [](Ring r, double dx, double dy) {
        for (auto& p : r)
            p = vector2(p[0] + dx, p[1] + dy);
        return r;
    };
    // two combs across each other inside a map plane so large (tiny = 0.04) that what the detection's thick teeth leave of the hole's
    // thin ones (0.001 x 5 each) is no piece, while what they cover (0.001 x 95 each) is more than tiny: the hole's 11 teeth stand
    // upright, the detection's 11 lie across them, each pair of teeth crosses four times -- 46 + 46 + 484 = 576 nodes, 968 cuts
    const Ring upright = named::comb(11, 100, 0.001, 100, 1590);
    Ring lying;
    for (const vector2& p : named::comb(11, 100, 95, 100, 2000))
        lying.emplace_back(p[1] - 500, p[0] + 500);
    const Ring huge = rect(-1e5, 1e5, -1e5, 1e5);
    // four holes of 126 vertices, 504 in all, each cut in two by a bar that passes between their vertices: 4 crossings each, 520
    std::vector<Ring> four;
    for (int k = 0; k < 4; ++k)
        four.push_back(named::ngon(126, 100, 150 + 230 * k, 200, M_PI / 126));
    struct Case { const char* name; Ring a; std::vector<Ring> holes; Ring b; std::vector<size_t> lengths; uint32_t handsAway; };
    const uint32_t CAP = CAPE_UNION_HOST_CAPACITY;
    std::vector<Case> table = {
        {"an L-shaped piece", map, {mid}, rect(450, 1200, 450, 1200), {8, 6}, 0},
        {"a bar cuts the hole in two", map, {mid}, rect(440, 460, 300, 1200), {8, 4, 4}, 0},
        {"a fork: a new hole, then three pieces", map, {rect(100, 900, 400, 500)}, fork, {8, 4, 4, 4, 4}, 0},
        {"the detection's edge on the hole's edge line", map, {mid}, rect(450, 1200, 400, 1200), {8, 4}, 0},
        {"kept: the edge runs along the hole's side", map, {mid}, rect(500, 1200, 300, 1200), {8, 4}, 0},
        {"covered: the corner on the hole's corner", map, {mid}, rect(400, 1200, 400, 1200), {8}, 0},
        {"a triangular piece", map, {mid}, {{390, 510}, {390, 1200}, {1200, 1200}, {1200, 300}, {510, 300}, {510, 390}}, {8, 3}, 0},
        {"a tilted bar", map, {mid}, {{430, 300}, {450, 300}, {470, 1200}, {450, 1200}}, {8, 4, 4}, 0},
        {"kept, cut and covered", map, {rect(100, 200, 100, 200), mid, rect(700, 800, 700, 800)}, rect(450, 1200, 450, 1200), {8, 4, 6}, 0},
        {"new, kept and a piece", cShape, {rect(100, 200, 100, 200), rect(2400, 2600, 100, 200)}, rect(2500, 4000, 0, 3000), {4, 4, 4, 4}, 0},
        {"exactly eight interior rings", map, some_of_eight(6), rect(440, 460, 300, 1200), {8, 4, 4, 4, 4, 4, 4, 4, 4}, 0},
        {"nine interior rings", map, some_of_eight(7), rect(440, 460, 300, 1200), {}, 0},
        {"a sliver piece falls to drop_collinear", map, {mid}, rect(400.0000001, 1200, 300, 1200), {8}, 0},
        {"a sliver just above tiny", rect(-512, 512, -512, 512), {rect(-100, 0, -100, 0)}, rect(-100 + std::ldexp(1.0, -20), 600, -600, 600), {8, 4}, 0},
        {"99 interior vertices before simplify", map, {named::ngon(128, 200, 300, 300, 0.01)}, rect(300, 1400, 300, 1400), {8, 8}, 0},
        // (on the device the intersection of this hole and the cog exceeds its 16 edges of a ring over one slab: the port takes the
        // intersection from the host class and serves the row, the next one is its sibling within that capacity)
        {"a cog across a 128-gon", rect(0, 4000, 0, 4000), {named::ngon(128, 500, 1000, 1000, 0.01)}, shifted(named::cog(900, 700), 1700, 1000), {4, 8, 85, 7}, 0},
        {"a cog of 64 vertices across a 128-gon", rect(0, 4000, 0, 4000), {named::ngon(128, 500, 1000, 1000, 0.01)}, shifted(named::cog(900, 700, 64), 1700, 1000), {4, 11, 73, 10}, 0},
        // tiny = 4e-4 and the first eps = 1e-5 from the map plane, the second eps = 6e-7 from the hole and the detection
        {"a second piece below tiny", rect(-1e4, 1e4, -1e4, 1e4), {rect(-100, 0, -1, 0)}, rect(-100 + std::ldexp(1.0, -12), -50, -600, 600), {4, 4}, 0},
        {"a sliver narrower than the first eps", rect(-1e4, 1e4, -1e4, 1e4), {rect(-100, 0, -200, 0)}, rect(-100 + std::ldexp(1.0, -18), 600, -600, 600), {4, 4}, 0},
        {"crossed combs: the second arrangement beyond 512 nodes", huge, {upright}, lying, {4, 44}, CAP},
        {"four holes cut in two: 520 interior vertices", rect(0, 1000, 0, 400), four, rect(20, 1200, 199, 201), {}, 0},
    };
    for (const Case& c : table)
    {
        std::vector<size_t> lengths;
        const long before = counts[cut::kCapacity];
        bad += cut::compare(c.name, c.a, c.holes, c.b, counts, c.handsAway, &lengths);
        const bool capacity = counts[cut::kCapacity] != before;
        std::printf("  %-58s", c.name);
        if (capacity)
            std::printf(" capacity");
        else
            for (size_t n : lengths)
                std::printf(" %zu", n);
        std::printf("\n");
        if (capacity ? !c.lengths.empty() : lengths != c.lengths)
        {
            std::printf("OUTCOME: %s: not the table's ring lengths\n", c.name);
            ++bad;
        }
    }
    std::printf("table: %zu pairs; served without / with pieces %ld / %ld, capacity %ld, handed away by the port alone %ld\n", table.size(),
                counts[cut::kPlain], counts[cut::kPieces], counts[cut::kCapacity], counts[cut::kHandedAway]);
    std::printf("table: the largest second arrangement has %d nodes\n", cut::largestSecond);
    // ---- the 2 200 star pairs of tests/host/map_union_holes_algebra.cpp: the same generator, draw for draw
    std::mt19937_64 rng(2024);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long stars = 0, sc[cut::kCounts] = {0, 0, 0, 0};
    cut::largestSecond = 0;
    for (int n : {8, 24})
        for (int k = 0; k < 1100; ++k)
        {
            auto star = [&](double cx, double cy) {
                std::vector<double> t(n);
                for (double& v : t)
                    v = 6.283185307179586 * U(rng);
                std::sort(t.begin(), t.end());
                Ring r;
                for (double v : t)
                {
                    const double rad = 1000 * (0.5 + 0.5 * U(rng));
                    r.emplace_back(cx + rad * std::cos(v), cy + rad * std::sin(v));
                }
                return r;
            };
            const Ring a = star(0, 0), b = star(1200 * U(rng) - 600, 1200 * U(rng) - 600);
            double mx = 0, my = 0;
            for (const auto& p : a)
                mx += p[0], my += p[1];
            mx /= n, my /= n;
            std::vector<Ring> hs;
            if (k % 5)
                hs.push_back(rect(mx - 20, mx + 20, my - 20, my + 20));
            char name[64];
            std::snprintf(name, sizeof name, "%d-vertex star pair %d", n, k);
            bad += cut::compare(name, a, hs, b, sc);
            ++stars;
        }
    std::printf("stars: %ld pairs; served without / with pieces %ld / %ld, capacity %ld, handed away by the port alone %ld\n", stars, sc[cut::kPlain],
                sc[cut::kPieces], sc[cut::kCapacity], sc[cut::kHandedAway]);
    std::printf("stars: the largest second arrangement has %d nodes\n", cut::largestSecond);
    std::printf("pairs that differ from the host class in a bit: %ld\n", bad);
    return (bad == 0 && counts[cut::kHandedAway] == 1 && stars == 2200 && sc[cut::kPieces] == 142 && sc[cut::kHandedAway] == 0) ? 0 : 1;
}

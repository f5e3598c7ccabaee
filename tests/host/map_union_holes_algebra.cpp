// The holes mode of csrc/cape_map_union.h (union_pair_rings<false>, union_simplify_holed) one lane at a time, compared bit for bit with
// host/boundary_polygon.cpp's merge_union and simplify on map polygons that have interior rings and unions that create some, under the
// address and undefined-behaviour sanitizers.  A stand-alone program.  tests/host/map_union_algebra.cpp is included as text with its
// main renamed: it brings the host class (boundary_polygon.cpp as text), the plain per-lane functions of the device header over
// tests/host/hip_stub, what the port of the mode without holes shares with this one, as the device header shares it (seq::Arrangement
// with the rank sort, the walks and the face test, seq::dp_candidate, seq::simple, seq::drop, seq::in_ring) and the ring
// generators of the Python tables (named::).  New here, in the device's order of statements: the faces that become holes, stored in
// face-walk order and oriented like add_hole; Polygon::area() in the disjoint rule; the carried holes with the bounding-box test of the
// device header (union_boxes_apart, compiled here, like union_point_in_or_on of simplify's in-ring check) in front of the host's rings_inter_area, which the device restates elsewhere
// (cape_ring_area.h, the matchers' tests); a partly covered hole before every capacity; simplify() over all rings or none with the
// 3-vertex skip, the in-ring check and the tolerance from the area without the holes.  The frames are canonical: the projection of an
// interior ring is union_project, covered by map_union_algebra.cpp, and its order on the wave by tests/test_gpu_map_union_holes.py,
// which also covers what needs the wave: the LDS carve and its borrowed regions, the barriers, the ballots.  holes::pair also holds
// the cut mode, as union_pair_rings does: given the second arrangement (`pieces`), a partly covered hole is cut into its pieces instead
// of handed to the host.  tests/host/map_union_cut_algebra.cpp includes this file as text for it, as this file includes
// map_union_algebra.cpp, with MAP_UNION_HOLES_ALGEBRA_MAIN naming this program's main.  Build and run from the repository root:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Itests/host/hip_stub -Irgb-d-slam_amd/csrc -Irgb-d-slam_amd/host \
//       -Irgb-d-slam_amd/host/compat -o map_union_holes_algebra.exe tests/host/map_union_holes_algebra.cpp && ./map_union_holes_algebra.exe
#define main map_union_algebra_main
#include "map_union_algebra.cpp"
#undef main
#ifndef MAP_UNION_HOLES_ALGEBRA_MAIN
#define MAP_UNION_HOLES_ALGEBRA_MAIN main
#endif

namespace holes {
using seq::area_of;
using seq::dp_candidate;
using seq::drop;
using seq::in_ring;
using seq::signed_area;
using seq::simple;
using seq::Ring2;
const int kHoles = CAPE_MAP_MAX_HOLES, kHoleVertices = CAPE_MAP_UNION_HOLE_VERTICES;

struct Out
{
    uint32_t flags = 0;
    std::vector<Ring2> rings; // outer, holes
    double area = 0;
    unsigned holesNew = 0, holesKept = 0, holesCovered = 0;
};

static void orient_hole(Ring2& r) // add_hole
{
    if (signed_area(r) < 0)
        std::reverse(r.begin(), r.end());
}
static double area_holed(const Ring2& ring, const std::vector<Ring2>& hs) // Polygon::area
{
    if (ring.size() < 3)
        return 0.0;
    double a = std::abs(signed_area(ring));
    for (const Ring2& h : hs)
        a -= std::abs(signed_area(h));
    return a < 0 ? 0.0 : a;
}
static size_t vertices_of(const std::vector<Ring2>& hs)
{
    size_t n = 0;
    for (const Ring2& h : hs)
        n += h.size();
    return n;
}
// union_simplify_holed
static void simplify_holed(Ring2& ring, std::vector<Ring2>& hs, double& area)
{
    area = area_holed(ring, hs);
    if (ring.size() < 4)
        return;
    const double eps = cape::umax(area / 1e5, 10.0);
    const Ring2 cand = dp_candidate(ring, eps);
    bool valid = cand.size() >= 3 && simple(cand);
    std::vector<Ring2> chs = hs;
    for (size_t k = 0; valid && k < hs.size(); ++k)
    {
        if (hs[k].size() < 4)
            continue;
        chs[k] = dp_candidate(hs[k], eps);
        valid = chs[k].size() >= 3 && simple(chs[k]);
        for (size_t i = 0; valid && i < chs[k].size(); ++i)
            valid = cape::union_point_in_or_on(chs[k][i], cand.data(), (int)cand.size());
    }
    if (!valid)
        return;
    const double newArea = area_holed(cand, chs);
    if (newArea > area * 0.75)
    {
        ring = cand;
        hs = chs;
        area = newArea;
    }
}

// The cut mode's second arrangement (union_arrange with rule 1 on a partly covered hole and the detection): the pieces of hole minus
// B follow the rings in `hs` while they fit, counted either way.  Returns 0 or the bits that end the pair.
typedef uint32_t (*Pieces)(const Ring2& hole, const Ring2& B, double tiny, std::vector<Ring2>& hs, int& nHoles, int& holeVertices);

// union_pair_rings: A, B oriented in one frame, mapHoles as the (projected) map polygon holds them.  The arrangement, the walks and
// the face test are seq::Arrangement's, as on the device; what is the modes' own stands here.  Without `pieces` the holes mode (a
// partly covered hole is the host's), with it the cut mode.
static Out pair(Ring2 A, Ring2 B, const std::vector<Ring2>& mapHoles, Pieces pieces = nullptr)
{
    Out out;
    const auto hosted = [](uint32_t f) { // union_hosted
        Out o;
        o.flags = (f & CAPE_UNION_HOST_CAPACITY) ? (uint32_t)CAPE_UNION_HOST_CAPACITY : f;
        return o;
    };
    seq::Arrangement G;
    if (!G.build(A, B) || G.capacity)
        return hosted(CAPE_UNION_HOST_CAPACITY);
    Ring2 outer;
    std::vector<Ring2> stored; // the faces that are holes, while they fit; all of them counted
    int nNew = 0, newVertices = 0;
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
                    {
                        if (nNew < kHoles && newVertices + (int)face.size() <= kHoleVertices)
                        {
                            orient_hole(face);
                            stored.push_back(face);
                        }
                        ++nNew;
                        newVertices += (int)face.size();
                    }
                }
        }
    }
    if (G.ambiguous)
        return hosted(CAPE_UNION_HOST_AMBIGUOUS);
    if (!outer.empty())
        drop(outer);
    const double outerArea = outer.size() >= 3 ? std::abs(signed_area(outer)) : 0.0;
    const double areaA = std::abs(signed_area(A)), areaB = std::abs(signed_area(B));
    bool disjoint = outer.size() >= 3 && (seq::left_out(A, outer) || seq::left_out(B, outer)), rule = false;
    if (outerArea + 1e-9 * cape::umax(areaA, areaB) < cape::umax(areaA, areaB))
    {
        disjoint = rule = true;
        if (area_holed(A, mapHoles) >= areaB)
        {
            if (vertices_of(mapHoles) > (size_t)kHoleVertices)
                return hosted(CAPE_UNION_HOST_CAPACITY);
            out.flags = CAPE_UNION_SERVED | CAPE_UNION_DISJOINT | (mapHoles.empty() ? 0u : (uint32_t)CAPE_UNION_HOLES);
            std::vector<Ring2> hs = mapHoles;
            simplify_holed(A, hs, out.area);
            out.rings.push_back(A);
            out.rings.insert(out.rings.end(), hs.begin(), hs.end());
            return out;
        }
        outer = B;
    }
    if (outer.size() < 3 || !simple(outer))
    {
        if (vertices_of(mapHoles) > (size_t)kHoleVertices)
            return hosted(CAPE_UNION_HOST_CAPACITY);
        out.flags = CAPE_UNION_SERVED | CAPE_UNION_UNCHANGED | (disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u) |
                    (mapHoles.empty() ? 0u : (uint32_t)CAPE_UNION_HOLES);
        out.rings.push_back(A);
        out.rings.insert(out.rings.end(), mapHoles.begin(), mapHoles.end());
        out.area = area_holed(A, mapHoles);
        return out;
    }
    if (outer.size() > 1 && outer.front().x == outer.back().x && outer.front().y == outer.back().y)
        outer.pop_back();
    seq::orient(outer);
    std::vector<Ring2> hs;
    int nHoles = 0, holeVertices = 0;
    bool cut = false;
    if (!rule)
    {
        hs = stored;
        nHoles = nNew;
        holeVertices = newVertices;
        out.holesNew = (unsigned)nNew;
        const double tiny = 1e-12 * cape::umax(areaA, areaB); // of the first pair of operands, for every hole
        std::vector<vector2> rb;
        for (const double2& p : B)
            rb.emplace_back(p.x, p.y);
        for (const Ring2& h : mapHoles)
        {
            std::vector<vector2> rh;
            for (const double2& p : h)
                rh.emplace_back(p.x, p.y);
            const double inter = cape::union_boxes_apart(h.data(), (int)h.size(), B.data(), (int)B.size()) ? 0.0 : ref::rings_inter_area(rh, rb);
            const double covered = inter < 0 ? 0.0 : inter;
            if (covered <= tiny)
            {
                if (nHoles < kHoles && holeVertices + (int)h.size() <= kHoleVertices)
                    hs.push_back(h);
                ++nHoles;
                holeVertices += (int)h.size();
                ++out.holesKept;
            }
            else if (inter < std::abs(signed_area(h)) - tiny)
            {
                cut = true;
                if (pieces)
                    if (const uint32_t bits = pieces(h, B, tiny, hs, nHoles, holeVertices))
                        return hosted(bits);
            }
            else
                ++out.holesCovered;
        }
    }
    if (!pieces && cut)
        return hosted(CAPE_UNION_HOST_HOLE_CUT);
    if (nHoles > kHoles || holeVertices > kHoleVertices)
        return hosted(CAPE_UNION_HOST_CAPACITY);
    out.flags = CAPE_UNION_SERVED | (disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u) | (nHoles > 0 ? (uint32_t)CAPE_UNION_HOLES : 0u) |
                (pieces && cut ? (uint32_t)CAPE_UNION_HOLE_PIECES : 0u);
    simplify_holed(outer, hs, out.area);
    out.rings.push_back(outer);
    out.rings.insert(out.rings.end(), hs.begin(), hs.end());
    return out;
}

// one pair through the host class and through the port: flags (as the twins derive them), every ring, the area, the counts
static long compare(const char* name, const named::Ring& a, const std::vector<named::Ring>& holesA, const named::Ring& b, long counts[5])
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
    for (const auto& h : pa.interior_rings())
        H.push_back(ring2(h));
    size_t before = 0;
    for (const auto& h : pa.interior_rings())
        before += h.size();
    ref::Polygon::MergeInfo info;
    const bool merged = pa.merge_union(pb, &info);
    const Out mine = pair(A, B, H);
    if (mine.flags & CAPE_UNION_HOST_AMBIGUOUS)
    {
        ++counts[4];
        return 0;
    }
    bool fits = pa.boundary().size() <= CAPE_MAP_MAX_RING && pa.interior_rings().size() <= CAPE_MAP_MAX_HOLES;
    uint32_t want;
    if (info.holeCut)
        want = CAPE_UNION_HOST_HOLE_CUT, ++counts[2];
    else if (!fits || (merged ? info.holeVertices : before) > CAPE_MAP_UNION_HOLE_VERTICES)
        want = CAPE_UNION_HOST_CAPACITY, ++counts[3];
    else
    {
        want = CAPE_UNION_SERVED | (merged ? 0u : (uint32_t)CAPE_UNION_UNCHANGED) | (info.disjoint ? (uint32_t)CAPE_UNION_DISJOINT : 0u) |
               (pa.interior_rings().empty() ? 0u : (uint32_t)CAPE_UNION_HOLES);
        ++counts[pa.interior_rings().empty() ? 0 : 1];
    }
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
} // namespace holes

int MAP_UNION_HOLES_ALGEBRA_MAIN()
{
    using named::Ring;
    using named::rect;
    long bad = 0, counts[5] = {0, 0, 0, 0, 0};
    // ---- the tables of tests/map_union_hole_cases.py
    const Ring cShape = {{0, 0}, {3000, 0}, {3000, 1000}, {1000, 1000}, {1000, 2000}, {3000, 2000}, {3000, 3000}, {0, 3000}};
    const Ring map = rect(0, 1000, 0, 1000), mid = rect(400, 500, 400, 500), det = rect(600, 1400, 600, 1400);
    std::vector<Ring> eight, cogs;
    for (int k = 0; k < 8; ++k)
        eight.push_back(rect(100 + 90 * k, 150 + 90 * k, 100, 150));
    for (int k = 0; k < 4; ++k)
    {
        Ring c = named::cog(500.0, 480.0);
        for (auto& p : c)
            p = vector2(p[0] + 1500.0 + 2000.0 * k, p[1] + 5000.0);
        cogs.push_back(c);
    }
    const Ring triangle = {{100, 100}, {200, 100}, {150, 200}}, dented = {{100, 100}, {100, 200}, {150, 200.5}, {200, 200}, {200, 100}};
    auto bar = [](int teeth) { return named::rect(-100, 100 * teeth + 100, 1500, 1600); };
    struct Case { const char* name; Ring a; std::vector<Ring> holes; Ring b; };
    std::vector<Case> table = {
        {"C shape and bar", cShape, {}, rect(2500, 4000, 0, 3000)},
        {"comb of 2 and bar", named::comb(2), {}, rect(-100, 300, 1500, 1600)},
        {"comb of 3 and bar", named::comb(3), {}, bar(3)},
        {"comb of 9 and bar", named::comb(9), {}, bar(9)},
        {"comb of 10 and bar", named::comb(10), {}, bar(10)},
        {"comb of 30 and bar", named::comb(30), {}, bar(30)},
        {"a hole clear of the detection", map, {rect(100, 200, 100, 200)}, det},
        {"a hole touching the detection in a corner", map, {rect(500, 600, 500, 600)}, det},
        {"a covered hole", map, {mid}, rect(300, 1200, 300, 1200)},
        {"a partly covered hole", map, {mid}, rect(450, 1200, 450, 1200)},
        {"disjoint, the holed map bigger", map, {mid}, rect(5000, 5100, 0, 100)},
        {"disjoint, the holed map bigger, the rule fires", map, {mid}, rect(-5100, -5000, 0, 100)},
        {"disjoint, the detection bigger, on the right", rect(0, 400, 0, 400), {rect(100, 200, 100, 200)}, rect(5000, 6000, 0, 1000)},
        {"the outer face is the detection's", rect(0, 400, 0, 400), {rect(100, 200, 100, 200)}, rect(-6000, -5000, 0, 1000)},
        {"eight holes", map, eight, rect(900, 1400, 0, 1000)},
        {"eight holes and a new one", cShape, eight, rect(2500, 4000, 0, 3000)},
        {"Douglas-Peucker drops a hole's vertex", map, {dented}, det},
        {"a triangular hole", map, {triangle}, det},
        {"a hole of 128 vertices", map, {named::ngon(128, 200, 300, 300, 0.01)}, det},
        {"a new hole before a kept one", cShape, {rect(100, 200, 100, 200)}, rect(2500, 4000, 0, 3000)},
        {"a hole covered by exactly tiny", rect(-512, 512, -512, 512), {rect(-100, 0, -100, 0)}, rect(-std::ldexp(1.0, -10), 600, -1e-12 * std::ldexp(1.0, 30), 600)},
        {"a small triangle under a dented outer ring", {{0, 0}, {0, 1000}, {300, 1000.5}, {1000, 1000}, {1000, 0}}, {{{100, 100}, {105, 100}, {102, 105}}}, det},
        {"an invalid candidate keeps every ring", map, {dented, rect(700, 705, 100, 105)}, det},
        {"the tolerance counts the holes out", rect(0, 4000, 0, 4000), {{{500, 500}, {500, 3500}, {2000, 3600}, {3500, 3500}, {3500, 500}}}, rect(3800, 4500, 0, 4000)},
        {"four cog holes, 512 vertices", rect(0, 10000, 0, 10000), cogs, rect(9000, 11000, 0, 10000)},
    };
    {
        std::vector<Ring> five = cogs;
        five.push_back(triangle);
        table.push_back({"four cog holes and a triangle, 515 vertices", rect(0, 10000, 0, 10000), five, rect(9000, 11000, 0, 10000)});
    }
    for (const Case& c : table)
        bad += holes::compare(c.name, c.a, c.holes, c.b, counts);
    std::printf("tables: %zu pairs; served without / with interior rings %ld / %ld, partly covered %ld, capacity %ld, ambiguous %ld\n", table.size(),
                counts[0], counts[1], counts[2], counts[3], counts[4]);
    const long tableServed = counts[0] + counts[1];
    // ---- random stars of 8 and 24 vertices with a 40 x 40 hole at ring a's vertex mean, and every fifth pair without one
    std::mt19937_64 rng(2024);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long stars = 0, sc[5] = {0, 0, 0, 0, 0};
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
            bad += holes::compare(name, a, hs, b, sc);
            ++stars;
        }
    std::printf("stars: %ld pairs; served without / with interior rings %ld / %ld, partly covered %ld, capacity %ld, ambiguous %ld\n", stars, sc[0],
                sc[1], sc[2], sc[3], sc[4]);
    std::printf("pairs that differ from the host class in a bit: %ld\n", bad);
    return (bad == 0 && tableServed >= 18 && counts[2] == 1 && counts[3] == 4 && stars >= 2000 && sc[1] >= 200 && sc[2] >= 20 && sc[4] * 20 <= stars) ? 0 : 1;
}

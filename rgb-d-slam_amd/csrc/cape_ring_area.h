// Shared by the intersection kernels of the polygon matchers and of the visibility kernels (cape_match_polygon.hip,
// cape_match_wide.hip: consecutive frames; cape_match_map.hip: a persistent map; cape_map_visibility.hip; what stands around the
// intersection in them: cape_pair_list.h): the capacity tiers, the LDS carve and rings_inter_area / rings_inter_area_coop -- this repo's host
// algorithm (host/boundary_polygon.cpp: rings_inter_area) statement for statement, see the header of cape_match_polygon.hip.
// Every file compiles its own copy (anonymous namespace; no device symbol crosses a file).
#pragma once
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_layout.h"
#include "cape_wave.h"

namespace cape {

namespace {

// Three instances of the intersection kernel, by capacity: vertices of one ring (simplified polygons: 13 on average, 90 at
// most on the test streams), slab boundaries (vertices of both rings + edge crossings), edges of one ring over one slab,
// independent waves per workgroup.  The capacities only size the LDS carve, i.e. how many waves a CU holds: the work is one
// wave's dependent LDS round trips and only other waves fill the gaps.  The small instance takes ~95 % of the pairs; a pair
// that exceeds one of an instance's capacities moves to the next one's work list.
template <int TIER> struct Tier;
#ifndef CAPE_MP_T0_STACK
#define CAPE_MP_T0_STACK 6
#endif
#ifndef CAPE_MP_T0_XS
#define CAPE_MP_T0_XS 256
#endif
#ifndef CAPE_MP_T0_GROUPS
#define CAPE_MP_T0_GROUPS 4
#endif
// kCoop (round 6): the four waves of a workgroup work on ONE pair -- the tiers behind the first hold the long pairs (an outline of
// 70 vertices over 145 slabs: 0.1 ms on a lone wave), whose edge-pair crossings, boundary sort and (edge, slab) incidences are
// data-parallel; only the final sum of the slab terms is ordered.  Same LDS per pair as before (the carve is shared), a quarter of
// the time for the parallel phases.  CAPE_MP_COOP=0: one wave per pair in every tier (the round-5 kernel, A/B builds).
#ifndef CAPE_MP_COOP
#define CAPE_MP_COOP 1
#endif
#ifndef CAPE_MP_COOP0
#define CAPE_MP_COOP0 0 // the first tier cooperative as well (A/B builds: -DCAPE_MP_COOP0=1 -DCAPE_MP_T0_GROUPS=8)
#endif
template <> struct Tier<0>
{
    static constexpr bool kCoop = CAPE_MP_COOP0 != 0;
    static constexpr int kRing = 32, kXs = CAPE_MP_T0_XS, kStack = CAPE_MP_T0_STACK, kWavesPerGroup = kCoop ? 4 : 2, kGroupsPerCu = CAPE_MP_T0_GROUPS;
};
template <> struct Tier<1>
{
    static constexpr bool kCoop = CAPE_MP_COOP != 0;
    static constexpr int kRing = 128, kXs = 1024, kStack = 16, kWavesPerGroup = kCoop ? 4 : 1, kGroupsPerCu = 2;
};
template <> struct Tier<2> // the comb-shaped outline that comes along once in a few thousand frames
{
    static constexpr bool kCoop = CAPE_MP_COOP != 0;
    static constexpr int kRing = 128, kXs = 1024, kStack = 32, kWavesPerGroup = kCoop ? 4 : 1, kGroupsPerCu = 1;
};
template <> struct Tier<3> // outlines of more than 128 vertices: the 64 x 48 cell grid of 1280 x 960 frames shows them (207 on the
{                          // TUM-like stream, profiles/r04_capacity_probe.txt); 145 KB of LDS, one workgroup per CU
    static constexpr bool kCoop = CAPE_MP_COOP != 0;
    static constexpr int kRing = 512, kXs = 2048, kStack = 32, kWavesPerGroup = kCoop ? 4 : 1, kGroupsPerCu = 1;
};
constexpr int kTiers = 4;
// The boundary array of a tier: rings_inter_area writes the na + nb <= 2 * kRing vertex abscissae before it checks any capacity, and
// sort_xs pads the boundaries to a power of two -- a kXs below 2 * kRing, or one that is no power of two (-DCAPE_MP_T0_XS=192),
// would overrun the array without a word.
template <int TIER> constexpr bool tier_xs_holds_its_rings() { return (Tier<TIER>::kXs & (Tier<TIER>::kXs - 1)) == 0 && Tier<TIER>::kXs >= 64 && Tier<TIER>::kXs >= 2 * Tier<TIER>::kRing; }
static_assert(tier_xs_holds_its_rings<0>() && tier_xs_holds_its_rings<1>() && tier_xs_holds_its_rings<2>() && tier_xs_holds_its_rings<3>(),
              "every tier's kXs must be a power of two (sort_xs pads to one, from 64 up) and at least 2 * kRing (the vertex abscissae are written before any capacity check)");
// the largest capacity any LATER tier offers (a pair beyond a tier's capacity moves on while one of them can hold it)
template <int TIER> constexpr int later_ring() { return TIER + 1 < kTiers ? (Tier<(TIER + 1 < kTiers ? TIER + 1 : TIER)>::kRing > later_ring<TIER + 1>() ? Tier<(TIER + 1 < kTiers ? TIER + 1 : TIER)>::kRing : later_ring<TIER + 1>()) : 0; }
template <> constexpr int later_ring<kTiers>() { return 0; }
template <int TIER> constexpr int later_xs() { return TIER + 1 < kTiers ? (Tier<(TIER + 1 < kTiers ? TIER + 1 : TIER)>::kXs > later_xs<TIER + 1>() ? Tier<(TIER + 1 < kTiers ? TIER + 1 : TIER)>::kXs : later_xs<TIER + 1>()) : 0; }
template <> constexpr int later_xs<kTiers>() { return 0; }
template <int TIER> constexpr int later_stack() { return TIER + 1 < kTiers ? (Tier<(TIER + 1 < kTiers ? TIER + 1 : TIER)>::kStack > later_stack<TIER + 1>() ? Tier<(TIER + 1 < kTiers ? TIER + 1 : TIER)>::kStack : later_stack<TIER + 1>()) : 0; }
template <> constexpr int later_stack<kTiers>() { return 0; }

#define CAPE_MP_SYNC()                                                                                        \
    do                                                                                                       \
    {                                                                                                        \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");                                               \
        __builtin_amdgcn_s_waitcnt(0);                                                                       \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");                                               \
    } while (0)

struct Edge // a.x < b.x
{
    double2 a, b;
};

struct MpLds
{
    int ringCap;
    double2* ringA; // ringCap
    double2* ringB; // ringCap
    Edge* ea;       // ringCap
    Edge* eb;       // ringCap
    double* xs;     // the tier's kXs
    double* terms;  // 64 x CAP (the intervals of a ring over a slab are disjoint: two sorted families of CAP/2 overlap in < CAP pairs)
    // the edges of both rings as ONE list: ring A's at [0, nea), ring B's at [ringCap, ringCap + neb)
    int* elo;             // 2 x ringCap: first slab an edge spans (index of a.x among the boundaries)
    int* ehi;             // 2 x ringCap: one past the last (index of b.x)
    int* pre;             // 2 x ringCap + 1: exclusive prefix of the edges' slab counts inside the current window
    int* cnt;             // 2 x 64: edges over each slab of the window, per ring
    double* by;           // 2 x 64 x CAP: their heights at the middle of the slab, in arrival order
    unsigned short* bk;   // 2 x 64 x CAP: their edge indices
    unsigned short* inc;  // 2 x 64 x CAP: where each (edge, slab) incidence of the window went: bucket << 8 | position
    unsigned char* sidx;  // 2 x 64 x CAP: positions in sorted order
    int* sh;              // 8 words the waves of a cooperative workgroup hand uniform values over in (kCoop tiers)
};

// ---- the LDS carve of a tier (one per wave; one per workgroup in the cooperative tiers), in byte offsets
struct MpLdsLayout
{
    size_t ringA, ringB, ea, eb, xs, terms, by, elo, ehi, pre, cnt, bk, inc, sidx, sh, bytes;
};
template <int TIER> __host__ __device__ constexpr MpLdsLayout mp_layout()
{
    using T = Tier<TIER>;
    Layout l;
    MpLdsLayout o{};
    o.ringA = l.take<double2>(T::kRing);
    o.ringB = l.take<double2>(T::kRing);
    o.ea = l.take<Edge>(T::kRing);
    o.eb = l.take<Edge>(T::kRing);
    o.xs = l.take<double>(T::kXs);
    o.terms = l.take<double>(64 * T::kStack);
    o.by = l.take<double>(128 * T::kStack);
    o.elo = l.take<int>(2 * T::kRing);
    o.ehi = l.take<int>(2 * T::kRing);
    o.pre = l.take<int>(2 * T::kRing + 2);
    o.cnt = l.take<int>(128);
    o.bk = l.take<unsigned short>(128 * T::kStack);
    o.inc = l.take<unsigned short>(128 * T::kStack);
    o.sidx = l.take<unsigned char>(128 * T::kStack);
    o.sh = l.take<int>(8, 16);
    o.bytes = l.end(16);
    return o;
}
template <int TIER> __device__ inline MpLds mp_carve(unsigned char* smem)
{
    constexpr MpLdsLayout o = mp_layout<TIER>();
    MpLds L;
    L.ringCap = Tier<TIER>::kRing;
    L.ringA = carve_at<double2>(smem, o.ringA);
    L.ringB = carve_at<double2>(smem, o.ringB);
    L.ea = carve_at<Edge>(smem, o.ea);
    L.eb = carve_at<Edge>(smem, o.eb);
    L.xs = carve_at<double>(smem, o.xs);
    L.terms = carve_at<double>(smem, o.terms);
    L.by = carve_at<double>(smem, o.by);
    L.elo = carve_at<int>(smem, o.elo);
    L.ehi = carve_at<int>(smem, o.ehi);
    L.pre = carve_at<int>(smem, o.pre);
    L.cnt = carve_at<int>(smem, o.cnt);
    L.bk = carve_at<unsigned short>(smem, o.bk);
    L.inc = carve_at<unsigned short>(smem, o.inc);
    L.sidx = carve_at<unsigned char>(smem, o.sidx);
    L.sh = carve_at<int>(smem, o.sh);
    return L;
}

__device__ __forceinline__ double y_at(const Edge& e, double x) { return e.a.y + (e.b.y - e.a.y) * ((x - e.a.x) / (e.b.x - e.a.x)); }

// ring_area_signed of a ring in LDS (ordered sum; every lane walks it)
__device__ __forceinline__ double ring_area_signed(const double2* r, int n)
{
    double s = 0;
    for (int i = 0, j = n - 1; i < n; j = i++)
        s += (r[j].x * r[i].y - r[i].x * r[j].y);
    return 0.5 * s;
}

// edges_of: the non-vertical edges (r[i-1], r[i]) in ring order, left end first.  Sequential compaction in ring order
// (every lane runs it, lane 0 writes): the order of the edges decides ties of the stable sort below.
__device__ __forceinline__ int edges_of(const double2* r, int n, Edge* out, int lane)
{
    int cnt = 0;
    for (int base = 0; base < n; base += 64)
    {
        const int i = base + lane;
        bool keep = false;
        Edge e;
        e.a = e.b = make_double2(0, 0);
        if (i < n)
        {
            double2 p = r[i == 0 ? n - 1 : i - 1], q = r[i];
            keep = !(p.x == q.x); // vertical edges bound no area in x
            if (p.x > q.x)
            {
                const double2 t = p;
                p = q;
                q = t;
            }
            e.a = p;
            e.b = q;
        }
        const unsigned long long kb = __ballot(keep);
        if (keep)
            out[cnt + __popcll(kb & ((1ull << lane) - 1ull))] = e;
        cnt += __popcll(kb);
    }
    CAPE_MP_SYNC();
    return cnt;
}

// bitonic sort of xs[0, n) ascending, padded with +inf to a power of two
__device__ inline void sort_xs(double* xs, int n, int lane)
{
    int np = 64;
    while (np < n)
        np <<= 1;
    for (int i = n + lane; i < np; i += 64)
        xs[i] = __builtin_inf();
    CAPE_MP_SYNC();
    for (int size = 2; size <= np; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1)
        {
            for (int t = lane; t < np / 2; t += 64)
            {
                const int lo = (t / stride) * (2 * stride) + (t % stride), hi = lo + stride;
                const bool up = ((lo / size) & 1) == 0;
                const double a = xs[lo], b = xs[hi];
                if ((b < a) == up && a != b)
                {
                    xs[lo] = b;
                    xs[hi] = a;
                }
            }
            CAPE_MP_SYNC();
        }
}

// index of the value v among the sorted, distinct boundaries xs[0, n) (v is one of them)
__device__ __forceinline__ int boundary_index(const double* xs, int n, double v)
{
    int lo = 0, hi = n - 1;
    while (lo < hi)
    {
        const int mid = (lo + hi) >> 1;
        if (xs[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// why a pair has no area (quiet NaNs told apart by their payload)
__device__ __forceinline__ double nan_code(int code) { return __longlong_as_double(0x7ff8000000000000ll | code); }
constexpr int kNanRing = 1, kNanSlabs = 2, kNanStack = 3, kNanPending = 4;
__device__ __forceinline__ bool is_nan_code(double v, int code) { return __double_as_longlong(v) == (0x7ff8000000000000ll | code); }

// rings_inter_area(A, B): A, B in LDS.  Returns the area, or NaN if a capacity of this kernel was exceeded (the caller flags
// the pair; the host class has no such limit).
#ifdef CAPE_MP_PROFILE
#define CAPE_MP_TICK(k) (prof[k] = __builtin_amdgcn_s_memtime())
#else
#define CAPE_MP_TICK(k)
#endif
template <int kStackCap, int kXsCap>
__device__ inline double rings_inter_area(const MpLds& L, int na, int nb, int lane, unsigned long long* prof = nullptr)
{
    constexpr int kTermsPerSlab = kStackCap;
    CAPE_MP_TICK(0);
    if (na < 3 || nb < 3)
        return 0.0;
    const int nea = edges_of(L.ringA, na, L.ea, lane), neb = edges_of(L.ringB, nb, L.eb, lane);
    // slab boundaries: every vertex, every isolated edge crossing
    int nx = 0;
    for (int i = lane; i < na; i += 64)
        L.xs[i] = L.ringA[i].x;
    for (int i = lane; i < nb; i += 64)
        L.xs[na + i] = L.ringB[i].x;
    nx = na + nb;
    bool overflow = false;
    const int pairs = nea * neb;
    for (int base = 0; base < pairs; base += 64)
    {
        const int q = base + lane;
        bool has = false;
        double x = 0.0;
        if (q < pairs)
        {
            const Edge e = L.ea[q / neb], f = L.eb[q % neb];
            const double d1x = e.b.x - e.a.x, d1y = e.b.y - e.a.y, d2x = f.b.x - f.a.x, d2y = f.b.y - f.a.y;
            const double den = d1x * d2y - d1y * d2x;
            if (den != 0) // parallel / collinear: no isolated crossing
            {
                const double t = ((f.a.x - e.a.x) * d2y - (f.a.y - e.a.y) * d2x) / den;
                const double u = ((f.a.x - e.a.x) * d1y - (f.a.y - e.a.y) * d1x) / den;
                if (t > 0 && t < 1 && u > 0 && u < 1)
                {
                    has = true;
                    x = e.a.x + t * d1x;
                }
            }
        }
        const unsigned long long hb = __ballot(has);
        const int add = __popcll(hb);
        if (nx + add > kXsCap)
        {
            overflow = true;
            break;
        }
        if (has)
            L.xs[nx + __popcll(hb & ((1ull << lane) - 1ull))] = x;
        nx += add;
    }
    if (overflow)
        return nan_code(kNanSlabs);
    CAPE_MP_SYNC();
    CAPE_MP_TICK(1);
#ifdef CAPE_MP_PROFILE
    prof[5] = (unsigned long long)nx;
#endif
    sort_xs(L.xs, nx, lane);
    // std::unique
    {
        int n = 0;
        for (int base = 0; base < nx; base += 64)
        {
            const int i = base + lane;
            double v = 0.0;
            bool keep = false;
            if (i < nx)
            {
                v = L.xs[i];
                keep = i == 0 || !(L.xs[i - 1] == v);
            }
            const unsigned long long kb = __ballot(keep);
            CAPE_MP_SYNC();
            if (keep)
                L.xs[n + __popcll(kb & ((1ull << lane) - 1ull))] = v;
            n += __popcll(kb);
            CAPE_MP_SYNC();
        }
        nx = n;
    }
    CAPE_MP_TICK(2);
#ifdef CAPE_MP_PROFILE
    prof[6] = (unsigned long long)nx;
#endif
    // Every boundary is a vertex abscissa or a crossing, so an edge spans exactly the slabs between the boundary at its left end
    // and the one at its right end (`a.x <= x0 && b.x >= x1` of the host loop)
    const int R = L.ringCap;
    for (int k = lane; k < 2 * R; k += 64)
    {
        const bool isB = k >= R;
        const int kk = isB ? k - R : k;
        int lo = 0, hi = 0;
        if (kk < (isB ? neb : nea))
        {
            const Edge e = isB ? L.eb[kk] : L.ea[kk];
            lo = boundary_index(L.xs, nx, e.a.x);
            hi = boundary_index(L.xs, nx, e.b.x);
        }
        L.elo[k] = lo;
        L.ehi[k] = hi;
    }
    CAPE_MP_SYNC();
    // slabs, 64 at a time.  The (edge, slab) incidences of the window are spread over the lanes: each computes the height of its
    // edge at the middle of its slab and drops it into the slab's bucket; a second pass ranks every entry inside its bucket by
    // (height, edge index) -- the order the host's stable sort by height leaves; then lane l computes the trapezoids of slab
    // base + l from the sorted stacks and the terms are added in slab order.
    double area = 0.0;
    for (int base = 0; base + 1 < nx; base += 64)
    {
        const int top = (base + 64 < nx - 1) ? base + 64 : nx - 1; // slabs [base, top)
        // incidences per edge, exclusive prefix
        int carry = 0;
        for (int kb = 0; kb < 2 * R; kb += 64)
        {
            const int k = kb + lane;
            int c = 0;
            if (k < 2 * R)
            {
                const int lo = L.elo[k] > base ? L.elo[k] : base, hi = L.ehi[k] < top ? L.ehi[k] : top;
                c = hi > lo ? hi - lo : 0;
            }
            const int incl = wave_scan_i32(c);
            if (k < 2 * R)
                L.pre[k] = carry + incl - c;
            carry += __builtin_amdgcn_readlane(incl, 63);
        }
        const int total = carry;
        if (lane == 0)
            L.pre[2 * R] = total;
        for (int q = lane; q < 128; q += 64)
            L.cnt[q] = 0;
        CAPE_MP_SYNC();
        if (total > 2 * 64 * kStackCap)
            return nan_code(kNanStack); // (some bucket must overflow)
        bool over = false;
        for (int t = lane; t < total; t += 64)
        {
            // the edge of incidence t: the last k with pre[k] <= t
            int lo = 0, hi = 2 * R;
            while (hi - lo > 1)
            {
                const int mid = (lo + hi) >> 1;
                if (L.pre[mid] <= t)
                    lo = mid;
                else
                    hi = mid;
            }
            const int k = lo;
            const bool isB = k >= R;
            const int kk = isB ? k - R : k;
            const int first = L.elo[k] > base ? L.elo[k] : base;
            const int sl = first + (t - L.pre[k]) - base;
            const Edge e = isB ? L.eb[kk] : L.ea[kk];
            const double x0 = L.xs[base + sl], x1 = L.xs[base + sl + 1], xm = 0.5 * (x0 + x1);
            const double y = y_at(e, xm);
            const int bucket = (isB ? 64 : 0) + sl;
            const int pos = atomicAdd(&L.cnt[bucket], 1);
            if (pos < kStackCap)
            {
                L.by[bucket * kStackCap + pos] = y;
                L.bk[bucket * kStackCap + pos] = (unsigned short)kk;
                L.inc[t] = (unsigned short)((bucket << 8) | pos);
            }
            else
                over = true;
        }
        CAPE_MP_SYNC();
        if (__any(over))
            return nan_code(kNanStack);
        for (int t = lane; t < total; t += 64)
        {
            const int bucket = L.inc[t] >> 8, pos = L.inc[t] & 255;
            const double y = L.by[bucket * kStackCap + pos];
            const int kk = L.bk[bucket * kStackCap + pos];
            const int c = L.cnt[bucket];
            int rank = 0;
            for (int m = 0; m < c; ++m)
            {
                const double y2 = L.by[bucket * kStackCap + m];
                const int k2 = L.bk[bucket * kStackCap + m];
                rank += (y2 < y || (y2 == y && k2 < kk)) ? 1 : 0;
            }
            L.sidx[bucket * kStackCap + rank] = (unsigned char)pos;
        }
        CAPE_MP_SYNC();
        const int s = base + lane;
        int myTerms = 0;
        if (s < top)
        {
            const double x0 = L.xs[s], x1 = L.xs[s + 1];
            const int ca = L.cnt[lane], cb = L.cnt[64 + lane];
            const int oa = lane * kStackCap, ob = (64 + lane) * kStackCap;
            for (int i = 0; i + 1 < ca; i += 2)
            {
                const int pa0 = L.sidx[oa + i], pa1 = L.sidx[oa + i + 1];
                const double ya0 = L.by[oa + pa0], ya1 = L.by[oa + pa1];
                for (int j = 0; j + 1 < cb; j += 2)
                {
                    const int pb0 = L.sidx[ob + j], pb1 = L.sidx[ob + j + 1];
                    const double yb0 = L.by[ob + pb0], yb1 = L.by[ob + pb1];
                    const bool loA = ya0 > yb0;
                    const double loY = loA ? ya0 : yb0;
                    const bool hiA = ya1 < yb1;
                    const double hiY = hiA ? ya1 : yb1;
                    if (!(hiY <= loY))
                    {
                        const Edge lo = loA ? L.ea[L.bk[oa + pa0]] : L.eb[L.bk[ob + pb0]];
                        const Edge hi = hiA ? L.ea[L.bk[oa + pa1]] : L.eb[L.bk[ob + pb1]];
                        const double h0 = y_at(hi, x0) - y_at(lo, x0);
                        const double h1 = y_at(hi, x1) - y_at(lo, x1);
                        if (myTerms < kTermsPerSlab)
                            L.terms[lane * kTermsPerSlab + myTerms] = 0.5 * (h0 + h1) * (x1 - x0);
                        ++myTerms;
                    }
                }
            }
        }
        CAPE_MP_SYNC();
        if (__any(myTerms > kTermsPerSlab))
            return nan_code(kNanStack); // (cannot happen with simple rings)
        // the ordered sum: slab by slab, term by term.  The first two terms of a slab travel through registers (a slab of two
        // convex-ish outlines has one), the rest through LDS
        const double t0 = myTerms > 0 ? L.terms[lane * kTermsPerSlab] : 0.0, t1 = myTerms > 1 ? L.terms[lane * kTermsPerSlab + 1] : 0.0;
        const int slabs = top - base;
        for (int l = 0; l < slabs; ++l)
        {
            const int c = __builtin_amdgcn_readlane(myTerms, l);
            if (c > 0)
                area += readlane_f64(t0, l);
            if (c > 1)
                area += readlane_f64(t1, l);
            for (int t = 2; t < c; ++t)
                area += L.terms[l * kTermsPerSlab + t];
        }
        CAPE_MP_SYNC();
    }
    CAPE_MP_TICK(3);
    return area;
}

// rings_inter_area for the FOUR waves of a workgroup on one pair (Tier::kCoop): the same statements, the data-parallel loops
// spread over 256 threads, the wave-collective ones (ordered compaction of the edges, std::unique, the prefix over the edges'
// slab counts, the slabs' trapezoids and the ordered sum) on wave 0, workgroup barriers between them.  Uniform values travel
// through L.sh.  The area is wave 0's (thread 0 stores it); every thread returns the same NaN code when a capacity is exceeded.
template <int kStackCap, int kXsCap>
__device__ inline double rings_inter_area_coop(const MpLds& L, int na, int nb, int tid)
{
    constexpr int kTermsPerSlab = kStackCap;
    constexpr int NT = 256;
    const int lane = tid & 63, wave = tid >> 6;
    int* sh = L.sh;
    if (na < 3 || nb < 3)
        return 0.0;
    if (wave == 0)
    {
        const int nea0 = edges_of(L.ringA, na, L.ea, lane), neb0 = edges_of(L.ringB, nb, L.eb, lane);
        if (lane == 0)
        {
            sh[0] = nea0;
            sh[1] = neb0;
            sh[2] = na + nb; // boundaries so far: every vertex
            sh[3] = 0;       // overflow
        }
    }
    for (int i = tid; i < na; i += NT)
        L.xs[i] = L.ringA[i].x;
    for (int i = tid; i < nb; i += NT)
        L.xs[na + i] = L.ringB[i].x;
    __syncthreads();
    const int nea = sh[0], neb = sh[1];
    // isolated edge crossings: every wave takes its share of the edge pairs and reserves room for what it finds with one atomic
    // (the boundaries are sorted afterwards: their arrival order is free)
    const int pairs = nea * neb;
    for (int base = 64 * wave; base < pairs; base += NT)
    {
        const int q = base + lane;
        bool has = false;
        double x = 0.0;
        if (q < pairs)
        {
            const Edge e = L.ea[q / neb], f = L.eb[q % neb];
            const double d1x = e.b.x - e.a.x, d1y = e.b.y - e.a.y, d2x = f.b.x - f.a.x, d2y = f.b.y - f.a.y;
            const double den = d1x * d2y - d1y * d2x;
            if (den != 0) // parallel / collinear: no isolated crossing
            {
                const double t = ((f.a.x - e.a.x) * d2y - (f.a.y - e.a.y) * d2x) / den;
                const double u = ((f.a.x - e.a.x) * d1y - (f.a.y - e.a.y) * d1x) / den;
                if (t > 0 && t < 1 && u > 0 && u < 1)
                {
                    has = true;
                    x = e.a.x + t * d1x;
                }
            }
        }
        const unsigned long long hb = __ballot(has);
        const int add = __popcll(hb);
        if (add)
        {
            int at = 0;
            if (lane == 0)
                at = atomicAdd(&sh[2], add);
            at = __builtin_amdgcn_readfirstlane(at);
            if (at + add > kXsCap)
            {
                if (lane == 0)
                    sh[3] = 1;
            }
            else if (has)
                L.xs[at + __popcll(hb & ((1ull << lane) - 1ull))] = x;
        }
    }
    __syncthreads();
    if (sh[3])
        return nan_code(kNanSlabs);
    int nx = sh[2];
    // bitonic sort of the boundaries over the workgroup
    {
        int np = 64;
        while (np < nx)
            np <<= 1;
        for (int i = nx + tid; i < np; i += NT)
            L.xs[i] = __builtin_inf();
        __syncthreads();
        for (int size = 2; size <= np; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1)
            {
                for (int t = tid; t < np / 2; t += NT)
                {
                    const int lo = (t / stride) * (2 * stride) + (t % stride), hi = lo + stride;
                    const bool up = ((lo / size) & 1) == 0;
                    const double a = L.xs[lo], b = L.xs[hi];
                    if ((b < a) == up && a != b)
                    {
                        L.xs[lo] = b;
                        L.xs[hi] = a;
                    }
                }
                __syncthreads();
            }
    }
    // std::unique (wave 0, in order)
    if (wave == 0)
    {
        int n = 0;
        for (int base = 0; base < nx; base += 64)
        {
            const int i = base + lane;
            double v = 0.0;
            bool keep = false;
            if (i < nx)
            {
                v = L.xs[i];
                keep = i == 0 || !(L.xs[i - 1] == v);
            }
            const unsigned long long kb = __ballot(keep);
            CAPE_MP_SYNC();
            if (keep)
                L.xs[n + __popcll(kb & ((1ull << lane) - 1ull))] = v;
            n += __popcll(kb);
            CAPE_MP_SYNC();
        }
        if (lane == 0)
            sh[2] = n;
    }
    __syncthreads();
    nx = sh[2];
    const int R = L.ringCap;
    for (int k = tid; k < 2 * R; k += NT)
    {
        const bool isB = k >= R;
        const int kk = isB ? k - R : k;
        int lo = 0, hi = 0;
        if (kk < (isB ? neb : nea))
        {
            const Edge e = isB ? L.eb[kk] : L.ea[kk];
            lo = boundary_index(L.xs, nx, e.a.x);
            hi = boundary_index(L.xs, nx, e.b.x);
        }
        L.elo[k] = lo;
        L.ehi[k] = hi;
    }
    __syncthreads();
    double area = 0.0; // (wave 0's)
    for (int base = 0; base + 1 < nx; base += 64)
    {
        const int top = (base + 64 < nx - 1) ? base + 64 : nx - 1; // slabs [base, top)
        if (wave == 0)
        {
            int carry = 0;
            for (int kb = 0; kb < 2 * R; kb += 64)
            {
                const int k = kb + lane;
                int c = 0;
                if (k < 2 * R)
                {
                    const int lo = L.elo[k] > base ? L.elo[k] : base, hi = L.ehi[k] < top ? L.ehi[k] : top;
                    c = hi > lo ? hi - lo : 0;
                }
                const int incl = wave_scan_i32(c);
                if (k < 2 * R)
                    L.pre[k] = carry + incl - c;
                carry += __builtin_amdgcn_readlane(incl, 63);
            }
            if (lane == 0)
            {
                L.pre[2 * R] = carry;
                sh[4] = carry;
                sh[5] = 0; // a bucket overflowed
                sh[6] = 0; // more terms than a slab holds
            }
        }
        for (int q = tid; q < 128; q += NT)
            L.cnt[q] = 0;
        __syncthreads();
        const int total = sh[4];
        if (total > 2 * 64 * kStackCap)
            return nan_code(kNanStack); // (some bucket must overflow)
        bool over = false;
        for (int t = tid; t < total; t += NT)
        {
            int lo = 0, hi = 2 * R;
            while (hi - lo > 1)
            {
                const int mid = (lo + hi) >> 1;
                if (L.pre[mid] <= t)
                    lo = mid;
                else
                    hi = mid;
            }
            const int k = lo;
            const bool isB = k >= R;
            const int kk = isB ? k - R : k;
            const int first = L.elo[k] > base ? L.elo[k] : base;
            const int sl = first + (t - L.pre[k]) - base;
            const Edge e = isB ? L.eb[kk] : L.ea[kk];
            const double x0 = L.xs[base + sl], x1 = L.xs[base + sl + 1], xm = 0.5 * (x0 + x1);
            const double y = y_at(e, xm);
            const int bucket = (isB ? 64 : 0) + sl;
            const int pos = atomicAdd(&L.cnt[bucket], 1);
            if (pos < kStackCap)
            {
                L.by[bucket * kStackCap + pos] = y;
                L.bk[bucket * kStackCap + pos] = (unsigned short)kk;
                L.inc[t] = (unsigned short)((bucket << 8) | pos);
            }
            else
                over = true;
        }
        if (over)
            sh[5] = 1;
        __syncthreads();
        if (sh[5])
            return nan_code(kNanStack);
        for (int t = tid; t < total; t += NT)
        {
            const int bucket = L.inc[t] >> 8, pos = L.inc[t] & 255;
            const double y = L.by[bucket * kStackCap + pos];
            const int kk = L.bk[bucket * kStackCap + pos];
            const int c = L.cnt[bucket];
            int rank = 0;
            for (int m = 0; m < c; ++m)
            {
                const double y2 = L.by[bucket * kStackCap + m];
                const int k2 = L.bk[bucket * kStackCap + m];
                rank += (y2 < y || (y2 == y && k2 < kk)) ? 1 : 0;
            }
            L.sidx[bucket * kStackCap + rank] = (unsigned char)pos;
        }
        __syncthreads();
        if (wave == 0)
        {
            const int s = base + lane;
            int myTerms = 0;
            if (s < top)
            {
                const double x0 = L.xs[s], x1 = L.xs[s + 1];
                const int ca = L.cnt[lane], cb = L.cnt[64 + lane];
                const int oa = lane * kStackCap, ob = (64 + lane) * kStackCap;
                for (int i = 0; i + 1 < ca; i += 2)
                {
                    const int pa0 = L.sidx[oa + i], pa1 = L.sidx[oa + i + 1];
                    const double ya0 = L.by[oa + pa0], ya1 = L.by[oa + pa1];
                    for (int j = 0; j + 1 < cb; j += 2)
                    {
                        const int pb0 = L.sidx[ob + j], pb1 = L.sidx[ob + j + 1];
                        const double yb0 = L.by[ob + pb0], yb1 = L.by[ob + pb1];
                        const bool loA = ya0 > yb0;
                        const double loY = loA ? ya0 : yb0;
                        const bool hiA = ya1 < yb1;
                        const double hiY = hiA ? ya1 : yb1;
                        if (!(hiY <= loY))
                        {
                            const Edge lo = loA ? L.ea[L.bk[oa + pa0]] : L.eb[L.bk[ob + pb0]];
                            const Edge hi = hiA ? L.ea[L.bk[oa + pa1]] : L.eb[L.bk[ob + pb1]];
                            const double h0 = y_at(hi, x0) - y_at(lo, x0);
                            const double h1 = y_at(hi, x1) - y_at(lo, x1);
                            if (myTerms < kTermsPerSlab)
                                L.terms[lane * kTermsPerSlab + myTerms] = 0.5 * (h0 + h1) * (x1 - x0);
                            ++myTerms;
                        }
                    }
                }
            }
            CAPE_MP_SYNC();
            if (__any(myTerms > kTermsPerSlab))
            {
                if (lane == 0)
                    sh[6] = 1;
            }
            else
            {
                const double t0 = myTerms > 0 ? L.terms[lane * kTermsPerSlab] : 0.0, t1 = myTerms > 1 ? L.terms[lane * kTermsPerSlab + 1] : 0.0;
                const int slabs = top - base;
                for (int l = 0; l < slabs; ++l)
                {
                    const int c = __builtin_amdgcn_readlane(myTerms, l);
                    if (c > 0)
                        area += readlane_f64(t0, l);
                    if (c > 1)
                        area += readlane_f64(t1, l);
                    for (int t = 2; t < c; ++t)
                        area += L.terms[l * kTermsPerSlab + t];
                }
            }
        }
        __syncthreads();
        if (sh[6])
            return nan_code(kNanStack); // (cannot happen with simple rings)
    }
    return area;
}

// the kept planes of a frame (output plane whose polygon Primitive_Detection keeps), in segment order: lane k < count holds
// the segment index of plane k
// hostOnly: some output plane of the frame has no device polygon (CAPE_POLY_OVERFLOW: its outline is left to the host class,
// which may well keep it) -- the kept-plane indices of such a frame cannot be told here, so the caller flags it
__device__ __forceinline__ int valid_planes(const cape_frame_record& rec, const cape_polygon* pol, int lane, int& mySeg, bool& hostOnly)
{
    int nSeg = rec.header.n_plane_segments;
    nSeg = nSeg < 0 ? 0 : (nSeg > CAPE_MAX_PLANES ? CAPE_MAX_PLANES : nSeg);
    const bool isOut = lane < nSeg && rec.segments[lane].is_output != 0;
    const unsigned flags = isOut ? pol[lane].flags : 0u;
    const bool ok = isOut && (flags & CAPE_POLY_VALID) != 0 && pol[lane].vertex_count >= 3;
    // (a frame that continues in spill records -- more than 64 plane segments -- is the host class's as well: its kept planes are
    // not all in this record)
    hostOnly = __ballot(isOut && (flags & CAPE_POLY_OVERFLOW) != 0) != 0ull || rec.header.next_record >= 0;
    const unsigned long long m = __ballot(ok);
    // lane k takes the k-th set bit
    int seg = -1;
    unsigned long long mm = m;
    for (int k = 0; k <= lane && mm; ++k, mm &= mm - 1)
        if (k == lane)
            seg = __ffsll((long long)mm) - 1;
    mySeg = seg;
    return __popcll(m);
}

} // namespace

template <int TIER> static size_t tier_lds_bytes() { return mp_layout<TIER>().bytes; }

} // namespace cape

// "Next" row N2 with the reference's own area measure: MapPlane::find_matches (reference
// src/map_management/map_features/map_primitive.cpp:91-161, driven by feature_map.hpp:647-670) between CONSECUTIVE frames of a
// batch, on the boundary polygons built by cape_build_polygons -- `detectedPolygon.inter_area(projectedPolygon)` in mm^2
// (map_primitive.cpp:137 -> src/utils/polygon.cpp:525-545) instead of the shared cells of the label grids that
// cape_match_consecutive counts.  The planes of frame f-1 play the map planes, seen through the identity pose.
//
//   cape_polygon_gate_kernel   : one wavefront per frame: the kept planes of the frame and of its predecessor, the gates
//        is_distance_similar / is_normal_similar (shape_primitives.cpp:66-86) of every (previous plane j, plane i) pair, and
//        the work list of the pairs to intersect.
//   cape_polygon_inter_kernel  : persistent wavefronts, one pair at a time: the polygon of j -- with a pose, through to_camera_space
//        (camera_frame / to_camera_vertex, cape_map_camera.h) -- is projected into the frame of i (Polygon::project: project_ring_b,
//        cape_pair_list.h) and oriented (orient_ring), and the area of the intersection of the two rings is computed.  Four
//        instances by capacity (LDS carve); a pair beyond one's capacities moves to the next one's list.  The walk over the 32-bit
//        lists, their front/back fill and the A/B knobs are this file's own (the 64-bit lists' walk: cape_pair_list.h).
//   cape_polygon_select_kernel : one wavefront per frame: the selection loop (greatest intersection above the overlap
//        threshold, is-matched flags updated between previous planes, the `selectedIndex <= 0` quirk).
//
// The intersection is this repo's host algorithm (host/boundary_polygon.cpp: rings_inter_area), statement for statement: the
// plane is cut into vertical slabs at every vertex and every edge crossing; inside a slab each ring is a stack of edges sorted
// by height and the overlap of the two stacks is a sum of trapezoids, added in slab order.  Lanes take the edge pairs (for the
// crossings), the compare-exchanges of a bitonic sort (slab boundaries), the (edge, slab) incidences of a window of 64 slabs
// (heights into per-slab buckets, then their ranks) and one slab each for the trapezoids, which are then added to the running
// area in order: the sum's rounding is observable.  + - x / and comparisons only: the areas are compared BIT FOR BIT with the
// host class (tests/test_gpu_match_polygon.py).
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_map_camera.h"
#include "cape_pair_list.h"
#include "cape_ring_area.h"
#include "cape_wave.h"

namespace cape {

namespace {

constexpr int kWaves = 2; // frames per workgroup of the gate / select kernels

constexpr int MP = CAPE_MATCH_MAX_PLANES;

// (the capacity tiers and the intersection itself: cape_ring_area.h)

// a pair of the work lists
__device__ __forceinline__ unsigned pack_pair(int frame, int j, int i) { return ((unsigned)frame << 8) | ((unsigned)j << 4) | (unsigned)i; }

} // namespace

// One wavefront per frame, sixteen frames per workgroup: the kept planes of the frame and of its predecessor, the gates of every (previous plane j, plane i)
// pair (Plane::is_distance_similar / is_normal_similar on the planes' parametrisations, shape_primitives.cpp:66-86) and the
// work list of the pairs whose polygons are to be intersected.  A pair the gates reject holds -1.
constexpr int kGateFrames = 16; // frames (waves) of a gate workgroup
__global__ __launch_bounds__(64 * kGateFrames) void cape_polygon_gate_kernel(MatchPolygonParams p, int nFrames)
{
    __shared__ unsigned s_count[kGateFrames];
    __shared__ unsigned s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frameRaw = blockIdx.x * kGateFrames + wave;
    const bool live = frameRaw < nFrames;
    const int frame = live ? frameRaw : nFrames - 1; // (idle waves of the last workgroup shadow a real frame and store nothing)
    cape_frame_match_exact& out = p.matches[frame];
    const cape_frame_record& recC = p.records[frame];
    const cape_polygon* polC = p.polygons + (size_t)frame * CAPE_MAX_PLANES;
    int segC = -1, segP = -1;
    bool hostOnlyC = false, hostOnlyP = false;
    const int nCur = valid_planes(recC, polC, lane, segC, hostOnlyC);
    const int nPrev = frame > 0 ? valid_planes(p.records[frame - 1], polC - CAPE_MAX_PLANES, lane, segP, hostOnlyP) : 0;
    const bool fits = nCur <= MP && nPrev <= MP && !hostOnlyC && !hostOnlyP;
    if (live && lane == 0)
    {
        out.n_prev = nPrev;
        out.n_cur = nCur;
        out.flags = fits ? 0u : (uint32_t)CAPE_MATCH_EXACT_OVERFLOW;
        out.pad = 0;
    }
    if (live && lane < MP)
    {
        out.match[lane] = -1;
        out.seg_prev[lane] = (lane < nPrev) ? segP : -1;
        out.seg_cur[lane] = (lane < nCur) ? segC : -1;
    }
    // my plane's parametrisation, read once (lane k: plane k of either frame)
    double cn[3] = {0, 0, 0}, cd = 0, pn[3] = {0, 0, 0}, pd = 0;
    if (segC >= 0)
    {
        const cape_plane_segment& S = recC.segments[segC];
        cn[0] = S.out_normal[0], cn[1] = S.out_normal[1], cn[2] = S.out_normal[2], cd = S.d;
    }
    if (segP >= 0)
    {
        const cape_plane_segment& Q = p.records[frame - 1].segments[segP];
        pn[0] = Q.out_normal[0], pn[1] = Q.out_normal[1], pn[2] = Q.out_normal[2], pd = Q.d;
        if (p.poses)
        {
            // the map plane seen from this frame's camera: PlaneWorldCoordinates::to_camera_coordinates (plane_coordinates.cpp:20-24)
            // with the plane matrix of camera_transformation.cpp:53-71, [R 0; -t^T R 1]; the PlaneCameraCoordinates constructor
            // normalises the rotated normal (host: utils::plane_to_camera)
            const double* T = p.poses + (size_t)frame * 16;
            const double r0 = (T[0] * pn[0] + T[1] * pn[1]) + T[2] * pn[2], r1 = (T[4] * pn[0] + T[5] * pn[1]) + T[6] * pn[2],
                         r2 = (T[8] * pn[0] + T[9] * pn[1]) + T[10] * pn[2];
            const double t0 = T[3], t1 = T[7], t2 = T[11];
            const double m0 = -((t0 * T[0] + t1 * T[4]) + t2 * T[8]), m1 = -((t0 * T[1] + t1 * T[5]) + t2 * T[9]),
                         m2 = -((t0 * T[2] + t1 * T[6]) + t2 * T[10]);
            pd = ((m0 * pn[0] + m1 * pn[1]) + m2 * pn[2]) + pd;
            const double nn = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
            pn[0] = r0, pn[1] = r1, pn[2] = r2;
            if (nn > 0)
                pn[0] = r0 / nn, pn[1] = r1 / nn, pn[2] = r2 / nn;
        }
    }
    unsigned long long gatedMask[MP * MP / 64];
    bool mine[MP * MP / 64];
#pragma unroll
    for (int k = 0; k < MP * MP / 64; ++k)
    {
        const int pair = k * 64 + lane, j = pair / MP, i = pair % MP;
        const double qn0 = __shfl(pn[0], j), qn1 = __shfl(pn[1], j), qn2 = __shfl(pn[2], j), qd = __shfl(pd, j);
        const double sn0 = __shfl(cn[0], i), sn1 = __shfl(cn[1], i), sn2 = __shfl(cn[2], i), sd = __shfl(cd, i);
        bool gated = false;
        if (fits && j < nPrev && i < nCur)
        {
            const double cosAngle = (sn0 * qn0 + sn1 * qn1) + sn2 * qn2;
            gated = fabs(sd - qd) < p.maxDistance && fabs(cosAngle) > p.minCosAngle;
        }
        if (live)
            out.inter_area[j][i] = gated ? nan_code(kNanPending) : -1.0;
        gatedMask[k] = __ballot(gated);
        mine[k] = gated;
    }
    // ONE atomic per workgroup on the list's counter (a counter every frame's wave bumps on its own serialises thousands of
    // atomics on one address: 50 us of the call)
    const unsigned myCount = (unsigned)(__popcll(gatedMask[0]) + __popcll(gatedMask[1]) + __popcll(gatedMask[2]) + __popcll(gatedMask[3]));
    if (lane == 0)
        s_count[wave] = live ? myCount : 0u;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        unsigned total = 0;
        for (int w = 0; w < kGateFrames; ++w)
        {
            const unsigned c = s_count[w];
            s_count[w] = total;
            total += c;
        }
        s_base = total ? atomicAdd(&p.listCounts[0], total) : 0u;
    }
    __syncthreads();
    if (!live)
        return;
    unsigned at = s_base + s_count[wave];
#pragma unroll
    for (int k = 0; k < MP * MP / 64; ++k)
    {
        const int pair = k * 64 + lane;
        if (mine[k])
            p.pairLists[at + __popcll(gatedMask[k] & ((1ull << lane) - 1ull))] = pack_pair(frame, pair / MP, pair % MP);
        at += (unsigned)__popcll(gatedMask[k]);
    }
}

// Persistent waves over the work list of tier TIER.  A pair beyond this tier's capacities moves to the next tier's list when
// that one is larger in the resource that ran out; otherwise its area stays a NaN that names the resource.
template <int TIER>
__global__ __launch_bounds__(64 * Tier<TIER>::kWavesPerGroup) void cape_polygon_inter_kernel(MatchPolygonParams p, int ldsPerWave)
{
    using T = Tier<TIER>;
    constexpr bool kHasNext = TIER + 1 < kTiers;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    constexpr bool kCoop = T::kCoop;
    // cooperative tiers: ONE carve for the workgroup's four waves, `tid` strides of 256; else a carve per (independent) wave
    const TierCtx<TIER> ctx = tier_ctx<TIER>(smem_all, ldsPerWave);
    const MpLds& L = ctx.L;
    const int lane = ctx.lane, wave = ctx.wave, tid = ctx.tid;
    constexpr int kStride = TierCtx<TIER>::kStride;
    const unsigned* list = p.pairLists + (size_t)TIER * p.pairCapacity;
    const unsigned count = p.listCounts[TIER];
    // The tiers behind the first hold few pairs of very unequal cost (an outline of 70 vertices over 145 slabs keeps a lone wave busy
    // for 0.1 ms, its neighbours on the list for a tenth of that): their waves take pairs off a TICKET counter (listCounts[4 + TIER],
    // cleared with the counts) instead of a fixed stride, so a wave that drew a long pair does not also sit on the pairs queued
    // behind it.  CAPE_MP_TICKETS: bit TIER set = that tier draws tickets (A/B builds; default: tiers 1..3).
#ifndef CAPE_MP_TICKETS
#define CAPE_MP_TICKETS 0xE
#endif
#ifndef CAPE_MP_REVERSE
#define CAPE_MP_REVERSE 0
#endif
    constexpr bool kTickets = ((CAPE_MP_TICKETS >> TIER) & 1) != 0;
    constexpr bool kReverse = ((CAPE_MP_REVERSE >> TIER) & 1) != 0;
    auto next_index = [&](unsigned prev, bool first) -> unsigned {
        if (kCoop)
        {
            // one pair per WORKGROUP: thread 0 draws (or strides), everybody reads the number
            if (threadIdx.x == 0)
                L.sh[7] = (int)(kTickets ? atomicAdd(&p.listCounts[4 + TIER], 1u) : (first ? blockIdx.x : prev + gridDim.x));
            __syncthreads();
            const unsigned t = (unsigned)L.sh[7];
            __syncthreads(); // (everybody has read it before thread 0 may write the next one)
            return t;
        }
        if (!kTickets)
            return first ? blockIdx.x * T::kWavesPerGroup + wave : prev + gridDim.x * T::kWavesPerGroup;
        unsigned t = 0;
        if (lane == 0)
            t = atomicAdd(&p.listCounts[4 + TIER], 1u);
        return (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    };
    for (unsigned t = next_index(0u, true); t < count; t = next_index(t, false))
    {
        // (tier 0's list is the gate kernel's, front only; the later tiers': front entries, then the back entries)
        const unsigned front = TIER == 0 ? count : p.listCounts[24 + TIER];
        const unsigned u = kReverse ? count - 1u - t : t;
        const unsigned pair = u < front ? list[u] : list[p.pairCapacity - 1u - (u - front)];
        const int frame = (int)(pair >> 8), j = (int)((pair >> 4) & 15u), i = (int)(pair & 15u);
        cape_frame_match_exact& out = p.matches[frame];
        const int si = out.seg_cur[i], sj = out.seg_prev[j];
        const cape_polygon& PS = p.polygons[(size_t)frame * CAPE_MAX_PLANES + si];       // detected polygon
        const cape_polygon& PQ = p.polygons[(size_t)(frame - 1) * CAPE_MAX_PLANES + sj]; // projected polygon (identity pose)
        const int na = (int)PS.vertex_count, nb = (int)PQ.vertex_count;
        double result;
        if (na > T::kRing || nb > T::kRing)
            result = nan_code(kNanRing);
        else
        {
            const double2* vertsC = p.vertices + (size_t)frame * p.boundaryCapacity + PS.vertex_offset;
            const double2* vertsP = p.vertices + (size_t)(frame - 1) * p.boundaryCapacity + PQ.vertex_offset;
            for (int v = tid; v < na; v += kStride)
                L.ringA[v] = vertsC[v];
            // the frame the previous plane's polygon lives in: its own, or -- with a pose -- the one to_camera_space gives it
            // (polygon_coordinates.cpp:135-165), its ring moved by transform_boundary (polygon.cpp:430-451) and oriented by the
            // explicit-ring constructor (polygon.cpp:236-266); then Polygon::project (polygon.cpp:338-382) into the frame of plane i,
            // the projected ring re-oriented clockwise like every polygon (OpenRing constructor)
            if (p.poses)
            {
                const double* Tm = p.poses + (size_t)frame * 16;
                const CameraFrame F = camera_frame(Tm, PQ.center, PQ.x_axis, PQ.y_axis);
                for (int v = tid; v < nb; v += kStride)
                    L.ringB[v] = to_camera_vertex(Tm, F, vertsP[v]);
                ctx.sync();
                orient_ring(L.ringB, nb, false, ctx);
                project_ring_b(ctx, L.ringB, nb, F.nc, F.nx, F.ny, PS);
            }
            else
                project_ring_b(ctx, vertsP, nb, PQ.center, PQ.x_axis, PQ.y_axis, PS);
            ctx.sync();
            orient_ring(L.ringB, nb, false, ctx);
#ifdef CAPE_MP_PROFILE
            unsigned long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const unsigned long long tStart = __builtin_amdgcn_s_memtime();
            if constexpr (kCoop)
                result = rings_inter_area_coop<T::kStack, T::kXs>(L, na, nb, tid);
            else
                result = rings_inter_area<T::kStack, T::kXs>(L, na, nb, lane, prof);
            if (!kCoop && lane == 0 && i < 8 && j < 8)
            {
                // unused slots of the area matrix carry the ticks of this pair (profiles/match_polygons_bench.py decodes them)
                out.inter_area[j + 8][i + 8] = (double)((prof[3] - tStart) >> 4) + 1e6 * na + 1e9 * nb + 1e12 * (double)prof[5];
                out.inter_area[j + 8][i] = (double)((prof[1] - prof[0]) >> 4) + 1e6 * (double)((prof[2] - prof[1]) >> 4);
                out.inter_area[j][i + 8] = (double)((prof[3] - prof[2]) >> 4) + 1e6 * (double)prof[6] + 1e12 * TIER;
            }
#else
            if constexpr (kCoop)
                result = rings_inter_area_coop<T::kStack, T::kXs>(L, na, nb, tid);
            else
                result = rings_inter_area<T::kStack, T::kXs>(L, na, nb, lane);
#endif
            ctx.sync();
        }
        if (tid == 0)
        {
            bool again = false;
            if (kHasNext)
                again = (is_nan_code(result, kNanStack) && later_stack<TIER>() > T::kStack) || (is_nan_code(result, kNanSlabs) && later_xs<TIER>() > T::kXs) ||
                        (is_nan_code(result, kNanRing) && later_ring<TIER>() > T::kRing);
            if (again)
            {
                // the next tier's list fills from both ends: pairs that left for their ring's size -- the big outlines, the long pairs --
                // at the front (their number in listCounts[24 + tier]), the others from the back; the tier works front first, so its
                // longest pairs start first.  A/B (profiles/r06_match_tickets.txt): no gain over arrival order once the waves draw tickets -- the tier ends with its longest PAIR, wherever that starts; kept as a build knob, off (0: one list in arrival order)
#ifndef CAPE_MP_HEAVY_FIRST
#define CAPE_MP_HEAVY_FIRST 0
#endif
                atomicAdd(&p.listCounts[TIER + 1], 1u);
                unsigned* nextList = p.pairLists + (size_t)(TIER + 1) * p.pairCapacity;
                if (CAPE_MP_HEAVY_FIRST == 0 || is_nan_code(result, kNanRing))
                    nextList[atomicAdd(&p.listCounts[24 + TIER + 1], 1u)] = pair;
                else
                    nextList[p.pairCapacity - 1u - atomicAdd(&p.listCounts[28 + TIER + 1], 1u)] = pair;
                // why the pair moves on (cape_debug_match_lists: words 8 + 4 * tier + reason; a handful of atomics per batch)
                atomicAdd(&p.listCounts[8 + 4 * TIER + (is_nan_code(result, kNanRing) ? 1 : (is_nan_code(result, kNanSlabs) ? 2 : 3))], 1u);
            }
            else
                out.inter_area[j][i] = result;
        }
    }
}

// One wavefront per frame: the selection loop of find_matches over the areas.
__global__ __launch_bounds__(64 * kWaves) void cape_polygon_select_kernel(MatchPolygonParams p, int nFrames)
{
    const int lane = threadIdx.x & 63;
    const int frame = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (frame >= nFrames)
        return;
    cape_frame_match_exact& out = p.matches[frame];
    uint32_t flags = out.flags;
    if (flags & CAPE_MATCH_EXACT_OVERFLOW)
        return; // more than MP kept planes: nothing was intersected
    const int nc = out.n_cur, npv = out.n_prev;
    const int segC = lane < nc ? out.seg_cur[lane] : -1;
    const int segP = lane < npv ? out.seg_prev[lane] : -1;
    const cape_polygon* polC = p.polygons + (size_t)frame * CAPE_MAX_PLANES;
    const double myArea = (lane < nc) ? polC[segC].area : 0.0;                            // detectedPolygon.get_area()
    const double myPrevArea = (lane < npv) ? (polC - CAPE_MAX_PLANES)[segP].area : 0.0; // projectedPolygon.get_area()
    bool matched = false;
    int myMatch = -1;
    for (int j = 0; j < npv; ++j)
    {
        const double projectedArea = __shfl(myPrevArea, j);
        const double ia = (lane < nc) ? out.inter_area[j][lane] : -1.0;
        if (lane < nc && ia != ia)
            flags |= CAPE_MATCH_EXACT_OVERFLOW; // a polygon pair beyond the kernel's capacities
        // interArea > greatestSimilarity (starting at 0) and interArea / newPlaneArea >= threshold; ascending scan with a strict
        // comparison = the lowest index among the largest areas
        unsigned long long key = 0;
        if (lane < nc && !matched && projectedArea > 0.0 && ia > 0.0 && ia / myArea >= p.minOverlap)
            key = (unsigned long long)__double_as_longlong(ia);
        const unsigned long long best = ~wave_min_u64(~key); // maximum of the bit patterns (positive doubles order like them)
        const unsigned mine = (key != 0 && key == best) ? (unsigned)(63 - lane) : 0u;
        const unsigned win = wave_max_u32(mine);
        int selected = best ? 63 - (int)win : -1;
        if (!(p.flags & CAPE_MATCH_ALLOW_INDEX0) && selected <= 0) // map_primitive.cpp:146
            selected = -1;
        if (selected >= 0 && lane == selected)
            matched = true;
        if (lane == j)
            myMatch = selected;
    }
    flags = wave_or_u32(flags);
    if (lane == 0)
        out.flags = flags;
    if (lane < MP)
        out.match[lane] = (lane < npv && !(flags & CAPE_MATCH_EXACT_OVERFLOW)) ? myMatch : -1;
}


template <int TIER> static hipError_t launch_polygon_tier(const MatchPolygonParams& p, int blocks, hipStream_t stream)
{
    const int lds = (int)tier_lds_bytes<TIER>();
    // (a cooperative tier's four waves share ONE carve)
    hipLaunchKernelGGL(cape_polygon_inter_kernel<TIER>, dim3(blocks), dim3(64 * Tier<TIER>::kWavesPerGroup),
                       (size_t)lds * (Tier<TIER>::kCoop ? 1 : Tier<TIER>::kWavesPerGroup), stream, p, lds);
    return hipGetLastError();
}

hipError_t launch_match_polygons(const MatchPolygonParams& p, int nFrames, hipStream_t stream)
{
    if (const hipError_t e = hipMemsetAsync(p.listCounts, 0, 32 * sizeof(unsigned), stream); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(cape_polygon_gate_kernel, dim3((nFrames + kGateFrames - 1) / kGateFrames), dim3(64 * kGateFrames), 0, stream, p, nFrames);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    // persistent grids: as many workgroups as the chip holds at once
    const int cus = p.computeUnits > 0 ? p.computeUnits : 256;
    const int maxPairs = nFrames * MP * MP;
    auto blocks_for = [&](int perCu, int pairsPerGroup) { // pairs a workgroup works on at a time: its waves, or one (cooperative tiers)
        const int need = (maxPairs + pairsPerGroup - 1) / pairsPerGroup;
        return need < cus * perCu ? need : cus * perCu;
    };
    if (const hipError_t e = launch_polygon_tier<0>(p, blocks_for(Tier<0>::kGroupsPerCu, Tier<0>::kCoop ? 1 : Tier<0>::kWavesPerGroup), stream); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_polygon_tier<1>(p, blocks_for(Tier<1>::kGroupsPerCu, Tier<1>::kCoop ? 1 : Tier<1>::kWavesPerGroup), stream); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_polygon_tier<2>(p, blocks_for(Tier<2>::kGroupsPerCu, Tier<2>::kCoop ? 1 : Tier<2>::kWavesPerGroup), stream); e != hipSuccess)
        return e;
    if (p.boundaryCapacity > Tier<2>::kRing && tier_lds_bytes<3>() <= (size_t)p.ldsLimitBytes) // (a ring is a subset of its plane's candidates)
        if (const hipError_t e = launch_polygon_tier<3>(p, blocks_for(Tier<3>::kGroupsPerCu, Tier<3>::kCoop ? 1 : Tier<3>::kWavesPerGroup), stream); e != hipSuccess)
            return e;
    hipLaunchKernelGGL(cape_polygon_select_kernel, dim3((nFrames + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, stream, p, nFrames);
    return hipGetLastError();
}

} // namespace cape

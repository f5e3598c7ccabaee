// What the pair-list kernels share around the ring intersection (cape_ring_area.h), the chain walk (cape_chain_walk.h) and the camera
// frame (cape_map_camera.h): cape_match_polygons_wide (cape_match_wide.hip), cape_match_map / _shards / _wide (cape_match_map.hip),
// cape_map_visibility / cape_map_step_visible (cape_map_visibility.hip).  In each a gate kernel reserves slots of a 64-bit work list
// (PairList, cape_internal.h) with one atomic per workgroup, persistent waves walk the list through the four capacity tiers, handing
// an entry to the next tier when a resource runs out, and a select kernel reads each frame's run of pairs.  Here, each once:
//
//   pack_pair64, kNoEntry        : an entry of the list
//   reserve_pairs, claim_frame   : a gate workgroup's reservation, and a frame's range in the list (or its empty slots)
//   TierCtx, tier_ctx            : the carve a tier's lanes share (one per workgroup, or one per wave), their stride and ordering point
//   orient_ring, project_ring_b  : a ring in LDS in the orientation the host class gives it; Polygon::project into the detected plane's frame
//   walk_tier                    : the walk of a tier's list around two callables -- an entry's area, and what to do with a final one
//   select_wide                  : the selection loop over runs of up to 128 gated pairs (two candidates per lane)
//   launch_tier                  : the persistent grid of a tier
//
// The 16-plane matcher (cape_match_polygon.hip, the one bench.py times) takes the carve and the ring placement only: its 32-bit lists,
// their front/back fill and its A/B knobs are its own, and so is its copy of the walk.
// Every file compiles its own copy (anonymous namespace; no device symbol crosses a file).
#pragma once
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_ring_area.h"
#include "cape_wave.h"

namespace cape {

namespace {

constexpr unsigned long long kNoEntry = ~0ull; // a slot of the work list reserved by a frame that did not fit

// a triple of the matchers' lists: i takes 8 bits, j the 24 above them
__device__ __forceinline__ unsigned long long pack_pair64(int frame, int j, int i)
{
    return ((unsigned long long)(unsigned)frame << 32) | ((unsigned long long)(unsigned)j << 8) | (unsigned long long)(unsigned)i;
}

// ONE atomic per workgroup on the list's counter reserves the slots of its kFrames waves (a frame each): returns the first slot of
// the calling wave's myCount entries.  EVERY wave of the workgroup must come here -- an idle one with myCount 0 -- and before any of
// them returns: there are two barriers inside.  s_count: kFrames words, s_base: one, both in LDS.
template <int kFrames> __device__ __forceinline__ unsigned long long reserve_pairs(const PairList& list, unsigned* s_count, unsigned long long& s_base, unsigned myCount)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        s_count[wave] = myCount;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        unsigned total = 0;
        for (int w = 0; w < kFrames; ++w)
        {
            const unsigned c = s_count[w];
            s_count[w] = total;
            total += c;
        }
        s_base = total ? atomicAdd(reinterpret_cast<unsigned long long*>(list.counts), (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    return s_base + s_count[wave];
}

// The frame's range in the list, by its wave: false = its myCount entries from `first` on do not fit the list; then the range is
// empty and the slots it reserved inside the list are marked empty (the walk skips them)
__device__ __forceinline__ bool claim_frame(const PairList& list, int frame, unsigned long long first, unsigned myCount)
{
    const int lane = threadIdx.x & 63;
    const bool listed = first + myCount <= list.capacity;
    if (lane == 0)
        list.frameRange[frame] = make_uint2((unsigned)(listed ? first : 0ull), listed ? myCount : 0u);
    if (!listed)
    {
        for (unsigned long long k = first + lane; k < first + myCount && k < list.capacity; k += 64)
            list.work[k] = kNoEntry;
    }
    return listed;
}

// The lanes that work on one pair in tier TIER and the carve they share: the four waves of the workgroup with ONE carve and `tid`
// strides of 256 (cooperative tiers), else a wave with a carve of its own
template <int TIER> struct TierCtx
{
    using T = Tier<TIER>;
    static constexpr bool kCoop = T::kCoop;
    static constexpr int kStride = kCoop ? 256 : 64;
    MpLds L;
    int lane, wave, tid;
    // ordering point between the lanes that share the carve: the wave (fence + wait) or the workgroup (barrier)
    __device__ __forceinline__ void sync() const
    {
        if (kCoop)
            __syncthreads();
        else
            CAPE_MP_SYNC();
    }
    // the area of the intersection of rings A and B of the carve, and the ordering point behind it
    __device__ __forceinline__ double inter_area(int na, int nb) const
    {
        double r;
        if constexpr (kCoop)
            r = rings_inter_area_coop<T::kStack, T::kXs>(L, na, nb, tid);
        else
            r = rings_inter_area<T::kStack, T::kXs>(L, na, nb, lane);
        sync();
        return r;
    }
};
template <int TIER> __device__ __forceinline__ TierCtx<TIER> tier_ctx(unsigned char* smemAll, int ldsPerWave)
{
    TierCtx<TIER> c;
    c.lane = threadIdx.x & 63, c.wave = threadIdx.x >> 6;
    c.tid = TierCtx<TIER>::kCoop ? (int)threadIdx.x : c.lane;
    c.L = mp_carve<TIER>(smemAll + (TierCtx<TIER>::kCoop ? (size_t)0 : (size_t)c.wave * ldsPerWave));
    return c;
}

// The orientation the host class gives a ring of n vertices in LDS: an outer ring clockwise (OpenRing constructor: reversed when its
// signed area is positive), a hole counter-clockwise (add_hole).  The caller's ordering point stands between the ring's stores and
// this; every lane reads the whole ring before any lane of the carve rewrites it.  Reversal in place: lane v swaps v and n - 1 - v.
template <typename Ctx> __device__ __forceinline__ void orient_ring(double2* ring, int n, bool hole, const Ctx& ctx)
{
    const double s = ring_area_signed(ring, n);
    ctx.sync();
    if (hole ? s < 0 : s > 0)
    {
        for (int v = ctx.tid; v < n / 2; v += Ctx::kStride)
        {
            const double2 a = ring[v], b = ring[n - 1 - v];
            ring[v] = b;
            ring[n - 1 - v] = a;
        }
        ctx.sync();
    }
}

// Polygon::project (polygon.cpp:338-382): every vertex of a ring in the frame (center, xAxis, yAxis) lifted to 3-D and expressed in
// the frame of the detected polygon PS, into ring B of the carve (src may be ring B itself: a lane rewrites what it read)
template <typename Ctx>
__device__ __forceinline__ void project_ring_b(const Ctx& ctx, const double2* src, int nb, const double* center, const double* xAxis, const double* yAxis,
                                               const cape_polygon& PS)
{
    for (int v = ctx.tid; v < nb; v += Ctx::kStride)
    {
        const double2 q = src[v];
        const double X = center[0] + q.x * xAxis[0] + q.y * yAxis[0];
        const double Y = center[1] + q.x * xAxis[1] + q.y * yAxis[1];
        const double Z = center[2] + q.x * xAxis[2] + q.y * yAxis[2];
        const double dx = X - PS.center[0], dy = Y - PS.center[1], dz = Z - PS.center[2];
        ctx.L.ringB[v] = make_double2((PS.x_axis[0] * dx + PS.x_axis[1] * dy) + PS.x_axis[2] * dz, (PS.y_axis[0] * dx + PS.y_axis[1] * dy) + PS.y_axis[2] * dz);
    }
}

// Persistent waves over the work list (tier 0) or a tier's list of indices into it (tiers 1..3).  Tier 0 takes a fixed stride over the
// (many, short) entries; the later tiers draw tickets (few entries of very unequal cost).  area(ctx, entry) is run by all lanes of the
// carve and returns the entry's area or a NaN that names the resource this tier lacks; such an entry moves to the next tier's list
// when that one is larger in the resource and runs on the device (lastTier; an entry visits each tier once).  Every other result is
// final: the carve's first lane calls finish(index in the list, entry, result).
template <int TIER, typename Area, typename Finish>
__device__ __forceinline__ void walk_tier(const PairList& list, int ldsPerWave, int lastTier, Area&& area, Finish&& finish)
{
    using T = Tier<TIER>;
    constexpr bool kHasNext = TIER + 1 < kTiers;
    constexpr bool kCoop = T::kCoop;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    const TierCtx<TIER> ctx = tier_ctx<TIER>(smem_all, ldsPerWave);
    const MpLds& L = ctx.L;
    const int lane = ctx.lane, wave = ctx.wave;
    const size_t cap = list.capacity;
    const unsigned long long reserved = *reinterpret_cast<const unsigned long long*>(list.counts);
    const unsigned long long count = TIER == 0 ? (reserved < cap ? reserved : cap) : (unsigned long long)list.counts[1 + TIER];
    const unsigned* indices = TIER == 0 ? nullptr : list.tierLists + (size_t)(TIER - 1) * cap;
    auto next_index = [&](unsigned long long prev, bool first) -> unsigned long long {
        if (kCoop)
        {
            // one entry per WORKGROUP: thread 0 draws (or strides), everybody reads the number
            if (threadIdx.x == 0)
                L.sh[7] = (int)(TIER > 0 ? atomicAdd(&list.counts[4 + TIER], 1u) : (unsigned)(first ? blockIdx.x : prev + gridDim.x));
            __syncthreads();
            const unsigned t = (unsigned)L.sh[7];
            __syncthreads(); // (everybody has read it before thread 0 may write the next one)
            return t;
        }
        if (TIER == 0)
            return first ? (unsigned long long)blockIdx.x * T::kWavesPerGroup + wave : prev + (unsigned long long)gridDim.x * T::kWavesPerGroup;
        unsigned t = 0;
        if (lane == 0)
            t = atomicAdd(&list.counts[4 + TIER], 1u);
        return (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    };
    for (unsigned long long t = next_index(0ull, true); t < count; t = next_index(t, false))
    {
        const size_t idx = TIER == 0 ? (size_t)t : (size_t)indices[t];
        const unsigned long long e = list.work[idx];
        if (e == kNoEntry)
            continue;
        const double result = area(ctx, e);
        if (ctx.tid == 0)
        {
            bool again = false;
            if (kHasNext && TIER + 1 <= lastTier)
                again = (is_nan_code(result, kNanStack) && later_stack<TIER>() > T::kStack) || (is_nan_code(result, kNanSlabs) && later_xs<TIER>() > T::kXs) ||
                        (is_nan_code(result, kNanRing) && later_ring<TIER>() > T::kRing);
            if (again)
                list.tierLists[(size_t)TIER * cap + atomicAdd(&list.counts[2 + TIER], 1u)] = (unsigned)idx;
            else
                finish(idx, e, result);
        }
    }
}

// One wavefront on one frame's run of the list: plane j after plane j in order, each with the contiguous run of its gated pairs (at
// most 128: two candidates per lane, at list positions at + lane and at + lane + 64); wave arg-max of the area above the overlap
// threshold, the lowest index on a tie, the `selectedIndex <= 0` quirk, a 128-bit is-matched mask.  curArea(k) / prevArea(k): the
// polygon area of detected plane k / of plane k of the other side (read with kPrevArea only: a map plane without a positive area lists
// no pair); matchRow: the frame's row of the match table; mapOfRow (kMapOf): the frame's 128 entries "plane j took detected plane i".
template <bool kPrevArea, bool kMapOf, typename Frame, typename CurArea, typename PrevArea>
__device__ __forceinline__ void select_wide(const PairList& list, int frame, Frame& out, uint32_t flags, double minOverlap, int32_t* matchRow, int32_t* mapOfRow,
                                            CurArea&& curArea, PrevArea&& prevArea)
{
    const int lane = threadIdx.x & 63;
    if (out.flags & CAPE_MATCH_EXACT_OVERFLOW)
        return; // nothing was intersected
    const int nc = out.n_cur; // (<= 128: the frame is not flagged)
    // detectedPolygon.get_area() / projectedPolygon.get_area() of my two planes of either side
    const double curArea0 = lane < nc ? curArea(lane) : 0.0;
    const double curArea1 = lane + 64 < nc ? curArea(lane + 64) : 0.0;
    double prevArea0 = 0.0, prevArea1 = 0.0;
    if constexpr (kPrevArea)
    {
        const int npv = out.n_prev;
        prevArea0 = lane < npv ? prevArea(lane) : 0.0;
        prevArea1 = lane + 64 < npv ? prevArea(lane + 64) : 0.0;
    }
    const uint2 range = list.frameRange[frame];
    const unsigned begin = range.x, end = range.x + range.y;
    // a pair beyond the intersection kernel's capacities: no match is reported for the frame
    bool nan = false;
    for (unsigned k = begin + lane; k < end; k += 64)
        nan |= list.workArea[k] != list.workArea[k];
    if (__any(nan))
    {
        if (lane == 0)
            out.flags |= CAPE_MATCH_EXACT_OVERFLOW;
        return;
    }
    unsigned long long takenLo = 0ull, takenHi = 0ull; // is-matched flags of the detected planes
    int myMapOf0 = -1, myMapOf1 = -1, nMatched = 0;
    for (unsigned at = begin; at < end;)
    {
        const unsigned k0 = at + lane, k1 = k0 + 64;
        const bool valid0 = k0 < end, valid1 = k1 < end;
        const unsigned long long e0 = valid0 ? list.work[k0] : 0ull, e1 = valid1 ? list.work[k1] : 0ull;
        const double ia0 = valid0 ? list.workArea[k0] : -1.0, ia1 = valid1 ? list.workArea[k1] : -1.0;
        const int jl0 = (int)((e0 >> 8) & 0xFFFFFFu), jl1 = (int)((e1 >> 8) & 0xFFFFFFu), i0 = (int)(e0 & 255u), i1 = (int)(e1 & 255u);
        const int j = __builtin_amdgcn_readfirstlane(jl0); // (lane 0's first candidate is the head of the run)
        const bool mine0 = valid0 && jl0 == j, mine1 = valid1 && jl1 == j;
        bool projected = true; // projectedArea > 0
        if constexpr (kPrevArea)
            projected = (j < 64 ? readlane_f64(prevArea0, j & 63) : readlane_f64(prevArea1, j & 63)) > 0.0;
        const double lo0 = __shfl(curArea0, i0 & 63), hi0 = __shfl(curArea1, i0 & 63), lo1 = __shfl(curArea0, i1 & 63), hi1 = __shfl(curArea1, i1 & 63);
        const double detArea0 = i0 < 64 ? lo0 : hi0, detArea1 = i1 < 64 ? lo1 : hi1;
        const bool taken0 = ((i0 < 64 ? takenLo >> i0 : takenHi >> (i0 - 64)) & 1ull) != 0ull;
        const bool taken1 = ((i1 < 64 ? takenLo >> i1 : takenHi >> (i1 - 64)) & 1ull) != 0ull;
        // interArea > greatestSimilarity (starting at 0) and interArea / newPlaneArea >= threshold (map_primitive.cpp:137-143); the
        // run is in ascending i and the comparison strict: the lowest index among the largest areas
        unsigned long long key0 = 0, key1 = 0;
        if (mine0 && !taken0 && projected && ia0 > 0.0 && ia0 / detArea0 >= minOverlap)
            key0 = (unsigned long long)__double_as_longlong(ia0);
        if (mine1 && !taken1 && projected && ia1 > 0.0 && ia1 / detArea1 >= minOverlap)
            key1 = (unsigned long long)__double_as_longlong(ia1);
        const unsigned long long best = ~wave_min_u64(~(key0 > key1 ? key0 : key1)); // maximum of the bit patterns (positive doubles order like them)
        // the winner's position in the run: my first candidate lies before every second one
        const unsigned pos = (key0 != 0 && key0 == best) ? (unsigned)lane : ((key1 != 0 && key1 == best) ? (unsigned)lane + 64u : 0xFFFFFFFFu);
        const unsigned win = wave_min_u32(pos);
        int selected = -1;
        if (best)
            selected = win < 64u ? __builtin_amdgcn_readlane(i0, (int)win) : __builtin_amdgcn_readlane(i1, (int)win - 64);
        if (!(flags & CAPE_MATCH_ALLOW_INDEX0) && selected <= 0) // map_primitive.cpp:146
            selected = -1;
        if (selected >= 0)
        {
            if (selected < 64)
                takenLo |= 1ull << selected;
            else
                takenHi |= 1ull << (selected - 64);
            ++nMatched;
            if (lane == selected)
                myMapOf0 = j;
            if (lane + 64 == selected)
                myMapOf1 = j;
            if (lane == 0)
                matchRow[j] = selected;
        }
        at += (unsigned)(__popcll(__ballot(mine0)) + __popcll(__ballot(mine1)));
    }
    if (lane == 0)
        out.n_matched = nMatched;
    if constexpr (kMapOf)
    {
        mapOfRow[lane] = myMapOf0;
        mapOfRow[lane + 64] = myMapOf1;
    }
}

// A tier's persistent grid: as many workgroups as the chip holds at once (the list's length is only known on the device); the LDS is
// one carve for a cooperative tier's workgroup, one per wave otherwise
template <int TIER, typename Kernel, typename Params> hipError_t launch_tier(Kernel kernel, const Params& p, hipStream_t stream)
{
    using T = Tier<TIER>;
    const int cus = p.computeUnits > 0 ? p.computeUnits : 256;
    const int lds = (int)tier_lds_bytes<TIER>();
    hipLaunchKernelGGL(kernel, dim3(cus * T::kGroupsPerCu), dim3(64 * T::kWavesPerGroup), (size_t)lds * (T::kCoop ? 1 : T::kWavesPerGroup), stream, p, lds);
    return hipGetLastError();
}

} // namespace

} // namespace cape

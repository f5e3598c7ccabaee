// Row N2 between CONSECUTIVE frames without the limits of cape_match_polygon.hip: MapPlane::find_matches (reference
// src/map_management/map_features/map_primitive.cpp:91-161, whose loop runs over every detected plane) for frames of up to
// CAPE_MATCH_WIDE_MAX_PLANES = 128 kept planes, counted in record order along the frame's whole record chain
// (cape_frame_header::next_record).  Per pair and per frame the statements are those of cape_match_polygons_pose; what differs is
// where the planes come from and how wide the tables are.
//
//   cape_wide_gate_kernel        : one wavefront per frame: both chains are walked 64 segments at a time, a ballot of the kept ones plus
//        the running count ranks them, and kept plane k's (record, segment in that record) goes into the frame's kept-plane table --
//        what the later kernels resolve a plane through (walk_chain, cape_chain_walk.h).  A lane holds planes k and k + 64 of
//        either frame; the pose goes on the previous planes; all n_prev x n_cur pairs go through the gates is_distance_similar / is_normal_similar
//        (shape_primitives.cpp:66-86) and the gated (frame, j, i) triples are appended to a 64-bit work list, per frame in (j, i)
//        order, with one atomic per workgroup on the list's counter.
//   cape_wide_inter_kernel<TIER> : persistent waves over the work list (tier 0) or a tier's list of indices into it: the previous
//        plane's polygon through the pose (to_camera_space), projected into the detected plane's frame (Polygon::project), and the
//        area of the intersection of the two rings -- the statements of cape_polygon_inter_kernel, both polygons reached through one
//        accessor (kept_polygon) that resolves (frame, kept plane) to the polygon row and vertex slab of the record the plane lives
//        in, the batch's or a spill record.  The capacity tiers and the intersection are cape_ring_area.h's.
//   cape_wide_select_kernel      : one wavefront per frame: the previous planes in order, each with the contiguous run of its gated
//        pairs (at most 128: two candidates per lane); wave arg-max of the area above the overlap threshold, the lowest index on a
//        tie, the `selectedIndex <= 0` quirk, a 128-bit is-matched mask.
//   cape_wide_carry_save_kernel  : one wavefront: the kept planes of ONE frame -- parameters, segment positions, polygons, rings back
//        to back -- into the handle's carried frame (cape_match_carry_save).  With CAPE_MATCH_CARRY the three kernels above take it
//        for the previous frame of frame 0 (prev_plane, prev_polygon): a stream cut into batches loses no frame pair at the cuts.
//
// + - x / and comparisons only, in the host class's association order (-ffp-contract=off): the areas are compared BIT FOR BIT with
// cape_match_polygons_pose where both serve a frame and with the host twin cape_host_match_planes (tests/test_gpu_match_wide.py).
#include <hip/hip_runtime.h>

#include "cape_chain_walk.h"
#include "cape_internal.h"
#include "cape_layout.h"
#include "cape_ring_area.h"
#include "cape_wave.h"

namespace cape {

namespace {

constexpr int WP = CAPE_MATCH_WIDE_MAX_PLANES;
static_assert(WP == 2 * 64, "a lane holds kept planes k and k + 64");
constexpr int kWideGateFrames = 4;   // frames (waves) of a gate workgroup
constexpr int kWideSelectFrames = 4; // frames (waves) of a select workgroup
constexpr unsigned long long kNoEntry = ~0ull; // a slot of the work list reserved by a frame that did not fit

__device__ __forceinline__ unsigned long long pack_wide_pair(int frame, int j, int i)
{
    return ((unsigned long long)(unsigned)frame << 32) | ((unsigned long long)(unsigned)j << 8) | (unsigned long long)(unsigned)i;
}

// ---- the LDS carve of a gate workgroup, in byte offsets: the reservation's hand-over words, then per wave the kept-plane tables of
// the frame and of its predecessor (location and position in the segment list) and the gate masks of every previous plane
struct WideGateLayout
{
    size_t base, count, kept, seg, mask, bytes;
};
__host__ __device__ constexpr WideGateLayout wide_gate_layout()
{
    Layout l;
    WideGateLayout o{};
    o.base = l.take<unsigned long long>(1);
    o.count = l.take<unsigned>(kWideGateFrames);
    o.kept = l.take<uint2>((size_t)kWideGateFrames * 2 * WP, 16);
    o.seg = l.take<int>((size_t)kWideGateFrames * 2 * WP, 16);
    o.mask = l.take<unsigned long long>((size_t)kWideGateFrames * 2 * WP, 16);
    o.bytes = l.end(16);
    return o;
}

// Kept plane k of a frame as the intersection and selection kernels see it: its polygon record and the vertex array its
// vertex_offset counts in, those of the record the plane lives in (the kept-plane table of the gate kernel)
struct KeptPolygon
{
    const cape_polygon* polygon;
    const double2* vertices;
    __device__ __forceinline__ const double2* ring() const { return vertices + polygon->vertex_offset; }
};
__device__ __forceinline__ KeptPolygon kept_polygon(const MatchWideParams& p, int frame, int k)
{
    const uint2 at = p.kept[(size_t)frame * WP + k]; // (record, segment in that record)
    return {p.polygons + (size_t)at.x * CAPE_MAX_PLANES + at.y, p.vertices + (size_t)at.x * p.boundaryCapacity};
}

// ---- the PREVIOUS frame of `frame`: frame - 1 of the batch, or -- for frame 0 of a call with CAPE_MATCH_CARRY -- the handle's carried
// frame (cape_wide_carry_save_kernel).  One accessor for the polygon and one for the plane's parameters; `frame` is uniform over the
// wave in every caller, so the choice is a scalar branch.
__device__ __forceinline__ bool prev_is_carried(const MatchWideParams& p, int frame) { return frame == 0 && p.carry.info != nullptr; }
__device__ __forceinline__ KeptPolygon prev_polygon(const MatchWideParams& p, int frame, int j)
{
    if (prev_is_carried(p, frame))
        return {p.carry.polygons + j, p.carry.vertices};
    return kept_polygon(p, frame - 1, j);
}
struct PlaneParams
{
    double n0, n1, n2, d; // out_normal, d
};
// keptP: the previous frame's kept-plane table of the gate kernel (not read for a carried frame)
__device__ __forceinline__ PlaneParams prev_plane(const MatchWideParams& p, int frame, int k, const uint2* keptP)
{
    if (prev_is_carried(p, frame))
    {
        const double* q = p.carry.planes + 4 * (size_t)k;
        return {q[0], q[1], q[2], q[3]};
    }
    const uint2 at = keptP[k];
    const cape_plane_segment& Q = p.records[at.x].segments[at.y];
    return {Q.out_normal[0], Q.out_normal[1], Q.out_normal[2], Q.d};
}
// the carried frame as walk_chain describes a frame of the batch: its segment positions into `segs`, its true count, its flag
__device__ __forceinline__ int load_carry(const MatchCarry& c, int lane, int* segs, bool& hostOnly)
{
    const int kept = c.info->n_kept;
    hostOnly = (c.info->flags & CAPE_MATCH_EXACT_OVERFLOW) != 0u;
    for (int k = lane; k < kept && k < WP; k += 64)
        segs[k] = c.segs[k];
    return kept;
}

// ---- the LDS carve of the save kernel's one wave: the frame's kept-plane table (walk_chain), then per kept plane the first vertex
// of its ring in the source slab array and in the carry, whose last entry + 1 is the total
struct CarrySaveLayout
{
    size_t kept, seg, src, dst, bytes;
};
__host__ __device__ constexpr CarrySaveLayout carry_save_layout()
{
    Layout l;
    CarrySaveLayout o{};
    o.kept = l.take<uint2>(WP, 16);
    o.seg = l.take<int>(WP, 16);
    o.src = l.take<unsigned long long>(WP, 16);
    o.dst = l.take<int>(WP + 1, 16);
    o.bytes = l.end(16);
    return o;
}

} // namespace

// cape_match_carry_save: ONE wavefront.  The chain walk and the ranks are the gate kernel's; a lane copies the parameters and the
// polygon of kept planes k and k + 64, a wave prefix sum of the vertex counts places the rings back to back, and the whole wave copies
// them, one vertex per lane and step over ALL rings (the plane of a vertex is found in the prefix sums).  Loads, stores and integer
// arithmetic only: nothing here can differ from the host class.  A flagged frame keeps its count and its first WP segment positions.
__global__ __launch_bounds__(64) void cape_wide_carry_save_kernel(CarrySaveParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr CarrySaveLayout lay = carry_save_layout();
    const int lane = threadIdx.x;
    uint2* kept = carve_at<uint2>(smem, lay.kept);
    int* segs = carve_at<int>(smem, lay.seg);
    unsigned long long* src = carve_at<unsigned long long>(smem, lay.src);
    int* dst = carve_at<int>(smem, lay.dst);
    const MatchCarry& c = p.carry;
    bool hostOnly = false;
    const RecordChains chains{p.records, p.polygons, p.maxBatch, p.nRecords};
    const int nAll = walk_chain(chains, p.frame, lane, kept, segs, hostOnly);
    CAPE_MP_SYNC(); // (the tables are read by other lanes of the wave than wrote them)
    const int n = nAll < WP ? nAll : WP;
    bool flagged = nAll > WP || hostOnly;
    int count[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s)
    {
        const int k = lane + 64 * s;
        if (k < n)
        {
            c.segs[k] = segs[k];
            const uint2 at = kept[k];
            count[s] = (int)p.polygons[(size_t)at.x * CAPE_MAX_PLANES + at.y].vertex_count;
        }
    }
    // a ring beyond the bound the store is sized by cannot come out of the polygon kernels; if one ever did, the frame is carried as
    // flagged rather than written past the store
    flagged = flagged || __any((unsigned)count[0] > (unsigned)c.ringCapacity || (unsigned)count[1] > (unsigned)c.ringCapacity);
    if (flagged)
        count[0] = count[1] = 0;
    const int scan0 = wave_scan_i32(count[0]), scan1 = wave_scan_i32(count[1]);
    const int total0 = __builtin_amdgcn_readlane(scan0, 63), total = total0 + __builtin_amdgcn_readlane(scan1, 63);
    const int first[2] = {scan0 - count[0], total0 + scan1 - count[1]};
#pragma unroll
    for (int s = 0; s < 2; ++s)
    {
        const int k = lane + 64 * s;
        dst[k] = k < n ? first[s] : total;
        if (k < n && !flagged)
        {
            const uint2 at = kept[k];
            const cape_plane_segment& S = p.records[at.x].segments[at.y];
            double* q = c.planes + 4 * (size_t)k;
            q[0] = S.out_normal[0], q[1] = S.out_normal[1], q[2] = S.out_normal[2], q[3] = S.d;
            cape_polygon pol = p.polygons[(size_t)at.x * CAPE_MAX_PLANES + at.y];
            src[k] = (unsigned long long)at.x * (unsigned long long)p.boundaryCapacity + pol.vertex_offset;
            pol.vertex_offset = (uint32_t)first[s];
            c.polygons[k] = pol;
        }
    }
    if (lane == 0)
    {
        dst[WP] = total;
        c.info->valid = 1;
        c.info->n_kept = nAll;
        c.info->flags = flagged ? (uint32_t)CAPE_MATCH_EXACT_OVERFLOW : 0u;
        c.info->n_vertices = total;
    }
    CAPE_MP_SYNC();
    // (total <= n x ringCapacity, the size of the store: every count passed the check above)
    for (int v = lane; v < total; v += 64)
    {
        // the kept plane whose ring holds v: the last one whose first vertex is not beyond it (a kept plane has >= 3 vertices)
        int lo = 0, hi = n - 1;
        while (lo < hi)
        {
            const int mid = (lo + hi + 1) >> 1;
            if (dst[mid] <= v)
                lo = mid;
            else
                hi = mid - 1;
        }
        c.vertices[v] = p.vertices[src[lo] + (unsigned long long)(v - dst[lo])];
    }
}


__global__ __launch_bounds__(64 * kWideGateFrames) void cape_wide_gate_kernel(MatchWideParams p, int nFrames)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr WideGateLayout lay = wide_gate_layout();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long& s_base = *carve_at<unsigned long long>(smem, lay.base);
    unsigned* s_count = carve_at<unsigned>(smem, lay.count);
    uint2* keptC = carve_at<uint2>(smem, lay.kept) + (size_t)wave * 2 * WP;
    uint2* keptP = keptC + WP;
    int* segsC = carve_at<int>(smem, lay.seg) + (size_t)wave * 2 * WP;
    int* segsP = segsC + WP;
    unsigned long long* masks = carve_at<unsigned long long>(smem, lay.mask) + (size_t)wave * 2 * WP; // [j][half of the detected planes]
    const int frameRaw = blockIdx.x * kWideGateFrames + wave;
    const bool live = frameRaw < nFrames;
    const int frame = live ? frameRaw : nFrames - 1; // (idle waves of the last workgroup shadow a real frame and store nothing)
    bool hostOnlyC = false, hostOnlyP = false;
    const RecordChains chains{p.records, p.polygons, p.maxBatch, p.nRecords};
    const int nCurAll = walk_chain(chains, frame, lane, keptC, segsC, hostOnlyC);
    int nPrevAll = 0;
    if (frame > 0)
        nPrevAll = walk_chain(chains, frame - 1, lane, keptP, segsP, hostOnlyP);
    else if (prev_is_carried(p, frame))
        nPrevAll = load_carry(p.carry, lane, segsP, hostOnlyP);
    CAPE_MP_SYNC(); // (the tables are read by other lanes of the wave than wrote them)
    const bool fits = nCurAll <= WP && nPrevAll <= WP && !hostOnlyC && !hostOnlyP;
    const int nCur = nCurAll < WP ? nCurAll : WP, nPrev = nPrevAll < WP ? nPrevAll : WP;
    // my planes' parametrisations, read once (lane k: planes k and k + 64 of either frame)
    double cn[2][3] = {{0, 0, 0}, {0, 0, 0}}, cd[2] = {0, 0}, pn[2][3] = {{0, 0, 0}, {0, 0, 0}}, pd[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s)
    {
        const int k = lane + 64 * s;
        if (live)
        {
            const size_t at = (size_t)frame * WP + k;
            p.kept[at] = k < nCur ? keptC[k] : make_uint2((unsigned)frame, 0u);
            p.match[at] = -1;
            p.segCur[at] = k < nCur ? segsC[k] : -1;
            p.segPrev[at] = k < nPrev ? segsP[k] : -1;
        }
        if (k < nCur)
        {
            const uint2 at = keptC[k];
            const cape_plane_segment& S = p.records[at.x].segments[at.y];
            cn[s][0] = S.out_normal[0], cn[s][1] = S.out_normal[1], cn[s][2] = S.out_normal[2], cd[s] = S.d;
        }
        if (k < nPrev) // (the parameters of a flagged carry are stale; its frame gates nothing: nGate below)
        {
            const PlaneParams Q = prev_plane(p, frame, k, keptP);
            pn[s][0] = Q.n0, pn[s][1] = Q.n1, pn[s][2] = Q.n2, pd[s] = Q.d;
            if (p.poses)
            {
                // the map plane seen from this frame's camera: PlaneWorldCoordinates::to_camera_coordinates (plane_coordinates.cpp:20-24)
                // with the plane matrix of camera_transformation.cpp:53-71, [R 0; -t^T R 1]; the PlaneCameraCoordinates constructor
                // normalises the rotated normal (host: utils::plane_to_camera) -- the statements of cape_polygon_gate_kernel
                const double* T = p.poses + (size_t)frame * 16;
                const double r0 = (T[0] * pn[s][0] + T[1] * pn[s][1]) + T[2] * pn[s][2], r1 = (T[4] * pn[s][0] + T[5] * pn[s][1]) + T[6] * pn[s][2],
                             r2 = (T[8] * pn[s][0] + T[9] * pn[s][1]) + T[10] * pn[s][2];
                const double t0 = T[3], t1 = T[7], t2 = T[11];
                const double m0 = -((t0 * T[0] + t1 * T[4]) + t2 * T[8]), m1 = -((t0 * T[1] + t1 * T[5]) + t2 * T[9]),
                             m2 = -((t0 * T[2] + t1 * T[6]) + t2 * T[10]);
                pd[s] = ((m0 * pn[s][0] + m1 * pn[s][1]) + m2 * pn[s][2]) + pd[s];
                const double nn = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
                pn[s][0] = r0, pn[s][1] = r1, pn[s][2] = r2;
                if (nn > 0)
                    pn[s][0] = r0 / nn, pn[s][1] = r1 / nn, pn[s][2] = r2 / nn;
            }
        }
    }
    // pass 1: the gates of every pair -- previous plane j is broadcast, a lane tests its two detected planes -- as two masks over
    // i per previous plane, kept in LDS, and their count
    const int nGate = fits ? nPrev : 0;
    unsigned myCount = 0;
    for (int j = 0; j < nGate; ++j)
    {
        const int jl = j & 63;
        double qn0, qn1, qn2, qd;
        if (j < 64)
            qn0 = readlane_f64(pn[0][0], jl), qn1 = readlane_f64(pn[0][1], jl), qn2 = readlane_f64(pn[0][2], jl), qd = readlane_f64(pd[0], jl);
        else
            qn0 = readlane_f64(pn[1][0], jl), qn1 = readlane_f64(pn[1][1], jl), qn2 = readlane_f64(pn[1][2], jl), qd = readlane_f64(pd[1], jl);
        unsigned long long m[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
        {
            const double cosAngle = (cn[s][0] * qn0 + cn[s][1] * qn1) + cn[s][2] * qn2;
            m[s] = __ballot(lane + 64 * s < nCur && fabs(cd[s] - qd) < p.maxDistance && fabs(cosAngle) > p.minCosAngle);
        }
        if (lane == 0)
            masks[2 * j] = m[0], masks[2 * j + 1] = m[1];
        myCount += (unsigned)(__popcll(m[0]) + __popcll(m[1]));
    }
    // ONE atomic per workgroup on the list's counter reserves the slots of its frames
    if (lane == 0)
        s_count[wave] = live ? myCount : 0u;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        unsigned total = 0;
        for (int w = 0; w < kWideGateFrames; ++w)
        {
            const unsigned c = s_count[w];
            s_count[w] = total;
            total += c;
        }
        s_base = total ? atomicAdd(reinterpret_cast<unsigned long long*>(p.counts), (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    if (!live)
        return;
    const unsigned long long first = s_base + s_count[wave];
    const bool listed = first + myCount <= p.workCapacity;
    if (lane == 0)
    {
        cape_frame_match_wide& out = p.frames[frame];
        out.n_prev = nPrevAll;
        out.n_cur = nCurAll;
        out.flags = (fits && listed) ? 0u : (uint32_t)CAPE_MATCH_EXACT_OVERFLOW;
        out.n_matched = 0;
        p.frameRange[frame] = make_uint2((unsigned)(listed ? first : 0ull), listed ? myCount : 0u);
    }
    if (!listed)
    {
        // the slots the frame reserved inside the list are marked empty: the intersection kernel skips them
        for (unsigned long long k = first + lane; k < first + myCount && k < p.workCapacity; k += 64)
            p.work[k] = kNoEntry;
    }
    // pass 2: the triples in (j, i) order
    const unsigned long long below = (1ull << lane) - 1ull;
    if (listed)
    {
        unsigned long long at = first;
        for (int j = 0; j < nGate; ++j)
        {
            const unsigned long long m0 = masks[2 * j], m1 = masks[2 * j + 1];
            if ((m0 >> lane) & 1ull)
            {
                const unsigned long long w = at + (unsigned)__popcll(m0 & below);
                p.work[w] = pack_wide_pair(frame, j, lane);
                p.workArea[w] = nan_code(kNanPending);
            }
            if ((m1 >> lane) & 1ull)
            {
                const unsigned long long w = at + (unsigned)(__popcll(m0) + __popcll(m1 & below));
                p.work[w] = pack_wide_pair(frame, j, lane + 64);
                p.workArea[w] = nan_code(kNanPending);
            }
            at += (unsigned)(__popcll(m0) + __popcll(m1));
        }
    }
    if (p.areas)
    {
        // the dense table: -1 where the pair is not gated (the intersection kernel overwrites the gated ones; a pair that is never
        // intersected -- a frame beyond the list -- keeps the NaN)
        for (int j = 0; j < WP; ++j)
        {
            const unsigned long long m0 = j < nGate ? masks[2 * j] : 0ull, m1 = j < nGate ? masks[2 * j + 1] : 0ull;
            double* row = p.areas + ((size_t)frame * WP + j) * WP;
            row[lane] = ((m0 >> lane) & 1ull) ? nan_code(kNanPending) : -1.0;
            row[lane + 64] = ((m1 >> lane) & 1ull) ? nan_code(kNanPending) : -1.0;
        }
    }
}

// Persistent waves over the work list (tier 0) or a tier's list of indices into it (tiers 1..3).  A triple beyond this tier's
// capacities moves to the next tier's list when that one is larger in the resource that ran out; otherwise its area stays a NaN
// that names the resource.  The list walk is cape_map_inter_kernel's, the pair's arithmetic cape_polygon_inter_kernel's.
template <int TIER>
__global__ __launch_bounds__(64 * Tier<TIER>::kWavesPerGroup) void cape_wide_inter_kernel(MatchWideParams p, int ldsPerWave)
{
    using T = Tier<TIER>;
    constexpr bool kHasNext = TIER + 1 < kTiers;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr bool kCoop = T::kCoop;
    // cooperative tiers: ONE carve for the workgroup's four waves, `tid` strides of 256; else a carve per (independent) wave
    const int tid = kCoop ? (int)threadIdx.x : lane;
    constexpr int kStride = kCoop ? 256 : 64;
    unsigned char* smem = smem_all + (kCoop ? (size_t)0 : (size_t)wave * ldsPerWave);
    const MpLds L = mp_carve<TIER>(smem);
    const size_t cap = p.workCapacity;
    const unsigned long long reserved = *reinterpret_cast<const unsigned long long*>(p.counts);
    const unsigned long long count = TIER == 0 ? (reserved < cap ? reserved : cap) : (unsigned long long)p.counts[1 + TIER];
    const unsigned* list = TIER == 0 ? nullptr : p.tierLists + (size_t)(TIER - 1) * cap;
    // tier 0: a fixed stride over the (many, short) triples; the later tiers draw tickets (few triples of very unequal cost)
    auto next_index = [&](unsigned long long prev, bool first) -> unsigned long long {
        if (kCoop)
        {
            if (threadIdx.x == 0)
                L.sh[7] = (int)(TIER > 0 ? atomicAdd(&p.counts[4 + TIER], 1u) : (unsigned)(first ? blockIdx.x : prev + gridDim.x));
            __syncthreads();
            const unsigned t = (unsigned)L.sh[7];
            __syncthreads(); // (everybody has read it before thread 0 may write the next one)
            return t;
        }
        if (TIER == 0)
            return first ? (unsigned long long)blockIdx.x * T::kWavesPerGroup + wave : prev + (unsigned long long)gridDim.x * T::kWavesPerGroup;
        unsigned t = 0;
        if (lane == 0)
            t = atomicAdd(&p.counts[4 + TIER], 1u);
        return (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    };
    // ordering point between the lanes that share a carve: the wave (fence + wait) or the workgroup (barrier)
    auto sync = [&]() {
        if (kCoop)
            __syncthreads();
        else
            CAPE_MP_SYNC();
    };
    for (unsigned long long t = next_index(0ull, true); t < count; t = next_index(t, false))
    {
        const size_t idx = TIER == 0 ? (size_t)t : (size_t)list[t];
        const unsigned long long e = p.work[idx];
        if (e == kNoEntry)
            continue;
        const int frame = (int)(e >> 32), j = (int)((e >> 8) & 0xFFFFFFu), i = (int)(e & 255u);
        const KeptPolygon D = kept_polygon(p, frame, i), Q = prev_polygon(p, frame, j);
        const cape_polygon& PS = *D.polygon; // detected polygon
        const cape_polygon& PQ = *Q.polygon; // projected polygon
        const int na = (int)PS.vertex_count, nb = (int)PQ.vertex_count;
        double result;
        if (na > T::kRing || nb > T::kRing)
            result = nan_code(kNanRing);
        else
        {
            const double2* vertsC = D.ring();
            const double2* vertsP = Q.ring();
            for (int v = tid; v < na; v += kStride)
                L.ringA[v] = vertsC[v];
            // Polygon::project (polygon.cpp:338-382): every vertex of the previous plane's ring lifted to 3-D and expressed in
            // the frame of plane i; the projected ring is re-oriented clockwise like every polygon (OpenRing constructor)
            // the frame the previous plane's polygon lives in: its own, or -- with a pose -- the one to_camera_space gives it
            // (polygon_coordinates.cpp:135-165: centre through the transform, axes through its rotation and re-normalised)
            double qc[3] = {PQ.center[0], PQ.center[1], PQ.center[2]}, qx[3] = {PQ.x_axis[0], PQ.x_axis[1], PQ.x_axis[2]},
                   qy[3] = {PQ.y_axis[0], PQ.y_axis[1], PQ.y_axis[2]};
            if (p.poses)
            {
                const double* T = p.poses + (size_t)frame * 16;
                double nc[3], nx[3], ny[3];
#pragma unroll
                for (int r = 0; r < 3; ++r)
                {
                    nc[r] = ((T[4 * r] * qc[0] + T[4 * r + 1] * qc[1]) + T[4 * r + 2] * qc[2]) + T[4 * r + 3];
                    nx[r] = (T[4 * r] * qx[0] + T[4 * r + 1] * qx[1]) + T[4 * r + 2] * qx[2];
                    ny[r] = (T[4 * r] * qy[0] + T[4 * r + 1] * qy[1]) + T[4 * r + 2] * qy[2];
                }
                const double lx = sqrt((nx[0] * nx[0] + nx[1] * nx[1]) + nx[2] * nx[2]), ly = sqrt((ny[0] * ny[0] + ny[1] * ny[1]) + ny[2] * ny[2]);
                if (lx > 0)
                    nx[0] /= lx, nx[1] /= lx, nx[2] /= lx;
                if (ly > 0)
                    ny[0] /= ly, ny[1] /= ly, ny[2] /= ly;
                // transform_boundary (polygon.cpp:430-451): every vertex lifted to 3-D, moved, re-expressed in the new frame; then the
                // explicit-ring constructor's orientation fix (polygon.cpp:236-266)
                for (int v = tid; v < nb; v += kStride)
                {
                    const double2 q = vertsP[v];
                    const double X = qc[0] + q.x * qx[0] + q.y * qy[0], Y = qc[1] + q.x * qx[1] + q.y * qy[1], Z = qc[2] + q.x * qx[2] + q.y * qy[2];
                    const double mx = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3], my = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7],
                                 mz = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
                    const double dx = mx - nc[0], dy = my - nc[1], dz = mz - nc[2];
                    L.ringB[v] = make_double2((nx[0] * dx + nx[1] * dy) + nx[2] * dz, (ny[0] * dx + ny[1] * dy) + ny[2] * dz);
                }
                sync();
                const bool flip = ring_area_signed(L.ringB, nb) > 0;
                sync(); // (every lane has read the ring before any lane of the carve rewrites it)
                if (flip)
                {
                    for (int v = tid; v < nb / 2; v += kStride)
                    {
                        const double2 a = L.ringB[v], b = L.ringB[nb - 1 - v];
                        L.ringB[v] = b;
                        L.ringB[nb - 1 - v] = a;
                    }
                    sync();
                }
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    qc[r] = nc[r], qx[r] = nx[r], qy[r] = ny[r];
            }
            for (int v = tid; v < nb; v += kStride)
            {
                const double2 q = p.poses ? L.ringB[v] : vertsP[v];
                const double X = qc[0] + q.x * qx[0] + q.y * qy[0];
                const double Y = qc[1] + q.x * qx[1] + q.y * qy[1];
                const double Z = qc[2] + q.x * qx[2] + q.y * qy[2];
                const double dx = X - PS.center[0], dy = Y - PS.center[1], dz = Z - PS.center[2];
                L.ringB[v] = make_double2((PS.x_axis[0] * dx + PS.x_axis[1] * dy) + PS.x_axis[2] * dz,
                                          (PS.y_axis[0] * dx + PS.y_axis[1] * dy) + PS.y_axis[2] * dz);
            }
            sync();
            const bool flip = ring_area_signed(L.ringB, nb) > 0;
            sync(); // (every lane has read the ring before any lane of the carve rewrites it)
            if (flip)
            {
                // reverse in place: lane v swaps v and nb - 1 - v
                for (int v = tid; v < nb / 2; v += kStride)
                {
                    const double2 a = L.ringB[v], b = L.ringB[nb - 1 - v];
                    L.ringB[v] = b;
                    L.ringB[nb - 1 - v] = a;
                }
                sync();
            }
            if constexpr (kCoop)
                result = rings_inter_area_coop<T::kStack, T::kXs>(L, na, nb, tid);
            else
                result = rings_inter_area<T::kStack, T::kXs>(L, na, nb, lane);
            sync();
        }
        if (tid == 0)
        {
            bool again = false;
            if (kHasNext)
                again = (is_nan_code(result, kNanStack) && later_stack<TIER>() > T::kStack) || (is_nan_code(result, kNanSlabs) && later_xs<TIER>() > T::kXs) ||
                        (is_nan_code(result, kNanRing) && later_ring<TIER>() > T::kRing);
            if (again)
                p.tierLists[(size_t)TIER * cap + atomicAdd(&p.counts[2 + TIER], 1u)] = (unsigned)idx; // (an entry visits each tier once)
            else
            {
                p.workArea[idx] = result;
                if (p.areas)
                    p.areas[((size_t)frame * WP + j) * WP + i] = result;
            }
        }
    }
}

// One wavefront per frame: the previous planes in order, each with the contiguous run of its gated pairs (at most WP of them:
// two candidates per lane, at list positions at + lane and at + lane + 64).
__global__ __launch_bounds__(64 * kWideSelectFrames) void cape_wide_select_kernel(MatchWideParams p, int nFrames)
{
    const int lane = threadIdx.x & 63;
    const int frame = blockIdx.x * kWideSelectFrames + (threadIdx.x >> 6);
    if (frame >= nFrames)
        return;
    cape_frame_match_wide& out = p.frames[frame];
    if (out.flags & CAPE_MATCH_EXACT_OVERFLOW)
        return; // nothing was intersected
    const int nc = out.n_cur, npv = out.n_prev; // (both <= WP: the frame is not flagged)
    // detectedPolygon.get_area() / projectedPolygon.get_area() of my two planes of either frame
    const double curArea0 = lane < nc ? kept_polygon(p, frame, lane).polygon->area : 0.0;
    const double curArea1 = lane + 64 < nc ? kept_polygon(p, frame, lane + 64).polygon->area : 0.0;
    const double prevArea0 = lane < npv ? prev_polygon(p, frame, lane).polygon->area : 0.0;
    const double prevArea1 = lane + 64 < npv ? prev_polygon(p, frame, lane + 64).polygon->area : 0.0;
    const uint2 range = p.frameRange[frame];
    const unsigned begin = range.x, end = range.x + range.y;
    // a pair beyond the intersection kernel's capacities: no match is reported for the frame
    bool nan = false;
    for (unsigned k = begin + lane; k < end; k += 64)
        nan |= p.workArea[k] != p.workArea[k];
    if (__any(nan))
    {
        if (lane == 0)
            out.flags |= CAPE_MATCH_EXACT_OVERFLOW;
        return;
    }
    unsigned long long takenLo = 0ull, takenHi = 0ull; // is-matched flags of the detected planes
    int nMatched = 0;
    for (unsigned at = begin; at < end;)
    {
        const unsigned k0 = at + lane, k1 = k0 + 64;
        const bool valid0 = k0 < end, valid1 = k1 < end;
        const unsigned long long e0 = valid0 ? p.work[k0] : 0ull, e1 = valid1 ? p.work[k1] : 0ull;
        const double ia0 = valid0 ? p.workArea[k0] : -1.0, ia1 = valid1 ? p.workArea[k1] : -1.0;
        const int jl0 = (int)(((unsigned)e0) >> 8), jl1 = (int)(((unsigned)e1) >> 8), i0 = (int)(e0 & 255u), i1 = (int)(e1 & 255u);
        const int j = __builtin_amdgcn_readfirstlane(jl0); // (lane 0's first candidate is the head of the run)
        const bool mine0 = valid0 && jl0 == j, mine1 = valid1 && jl1 == j;
        const double projectedArea = j < 64 ? readlane_f64(prevArea0, j & 63) : readlane_f64(prevArea1, j & 63);
        const double lo0 = __shfl(curArea0, i0 & 63), hi0 = __shfl(curArea1, i0 & 63), lo1 = __shfl(curArea0, i1 & 63), hi1 = __shfl(curArea1, i1 & 63);
        const double detArea0 = i0 < 64 ? lo0 : hi0, detArea1 = i1 < 64 ? lo1 : hi1;
        const bool taken0 = ((i0 < 64 ? takenLo >> i0 : takenHi >> (i0 - 64)) & 1ull) != 0ull;
        const bool taken1 = ((i1 < 64 ? takenLo >> i1 : takenHi >> (i1 - 64)) & 1ull) != 0ull;
        // interArea > greatestSimilarity (starting at 0) and interArea / newPlaneArea >= threshold (map_primitive.cpp:137-143); the
        // run is in ascending i and the comparison strict: the lowest index among the largest areas
        unsigned long long key0 = 0, key1 = 0;
        if (mine0 && !taken0 && projectedArea > 0.0 && ia0 > 0.0 && ia0 / detArea0 >= p.minOverlap)
            key0 = (unsigned long long)__double_as_longlong(ia0);
        if (mine1 && !taken1 && projectedArea > 0.0 && ia1 > 0.0 && ia1 / detArea1 >= p.minOverlap)
            key1 = (unsigned long long)__double_as_longlong(ia1);
        const unsigned long long best = ~wave_min_u64(~(key0 > key1 ? key0 : key1)); // maximum of the bit patterns (positive doubles order like them)
        // the winner's position in the run: my first candidate lies before every second one
        const unsigned pos = (key0 != 0 && key0 == best) ? (unsigned)lane : ((key1 != 0 && key1 == best) ? (unsigned)lane + 64u : 0xFFFFFFFFu);
        const unsigned win = wave_min_u32(pos);
        int selected = -1;
        if (best)
            selected = win < 64u ? __builtin_amdgcn_readlane(i0, (int)win) : __builtin_amdgcn_readlane(i1, (int)win - 64);
        if (!(p.flags & CAPE_MATCH_ALLOW_INDEX0) && selected <= 0) // map_primitive.cpp:146
            selected = -1;
        if (selected >= 0)
        {
            if (selected < 64)
                takenLo |= 1ull << selected;
            else
                takenHi |= 1ull << (selected - 64);
            ++nMatched;
            if (lane == 0)
                p.match[(size_t)frame * WP + j] = selected;
        }
        at += (unsigned)(__popcll(__ballot(mine0)) + __popcll(__ballot(mine1)));
    }
    if (lane == 0)
        out.n_matched = nMatched;
}

hipError_t launch_carry_save(const CarrySaveParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_wide_carry_save_kernel, dim3(1), dim3(64), carry_save_layout().bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_match_wide(const MatchWideParams& p, int nFrames, hipStream_t stream)
{
    if (const hipError_t e = hipMemsetAsync(p.counts, 0, 16 * sizeof(unsigned), stream); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(cape_wide_gate_kernel, dim3((nFrames + kWideGateFrames - 1) / kWideGateFrames), dim3(64 * kWideGateFrames),
                       wide_gate_layout().bytes, stream, p, nFrames);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    // persistent grids: as many workgroups as the chip holds at once (the list's length is only known on the device)
    const int cus = p.computeUnits > 0 ? p.computeUnits : 256;
    auto launch = [&](auto kernel, int lds, int wavesPerGroup, bool coop, int groupsPerCu) {
        hipLaunchKernelGGL(kernel, dim3(cus * groupsPerCu), dim3(64 * wavesPerGroup), (size_t)lds * (coop ? 1 : wavesPerGroup), stream, p, lds);
        return hipGetLastError();
    };
    if (const hipError_t e = launch(cape_wide_inter_kernel<0>, (int)tier_lds_bytes<0>(), Tier<0>::kWavesPerGroup, Tier<0>::kCoop, Tier<0>::kGroupsPerCu); e != hipSuccess)
        return e;
    if (const hipError_t e = launch(cape_wide_inter_kernel<1>, (int)tier_lds_bytes<1>(), Tier<1>::kWavesPerGroup, Tier<1>::kCoop, Tier<1>::kGroupsPerCu); e != hipSuccess)
        return e;
    if (const hipError_t e = launch(cape_wide_inter_kernel<2>, (int)tier_lds_bytes<2>(), Tier<2>::kWavesPerGroup, Tier<2>::kCoop, Tier<2>::kGroupsPerCu); e != hipSuccess)
        return e;
    // (a ring is a subset of its plane's candidates; a device without the LDS for the largest tier leaves its triples NaN: their
    // frames are flagged)
    if (p.boundaryCapacity > Tier<2>::kRing && tier_lds_bytes<3>() <= (size_t)p.ldsLimitBytes)
        if (const hipError_t e = launch(cape_wide_inter_kernel<3>, (int)tier_lds_bytes<3>(), Tier<3>::kWavesPerGroup, Tier<3>::kCoop, Tier<3>::kGroupsPerCu); e != hipSuccess)
            return e;
    hipLaunchKernelGGL(cape_wide_select_kernel, dim3((nFrames + kWideSelectFrames - 1) / kWideSelectFrames), dim3(64 * kWideSelectFrames), 0, stream, p,
                       nFrames);
    return hipGetLastError();
}

} // namespace cape

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
//        order (reserve_pairs, cape_pair_list.h).
//   cape_wide_inter_kernel<TIER> : the walk of the list through the capacity tiers (walk_tier, cape_pair_list.h) around one pair's
//        area: the previous plane's polygon through the pose (to_camera_space: camera_frame / to_camera_vertex, cape_map_camera.h),
//        projected into the detected plane's frame (project_ring_b) and oriented (orient_ring), and the area of the intersection of
//        the two rings (cape_ring_area.h); both polygons reached through one accessor (kept_polygon) that resolves (frame, kept
//        plane) to the polygon row and vertex slab of the record the plane lives in, the batch's or a spill record.
//   cape_wide_select_kernel      : one wavefront per frame: the previous planes in order, each with the contiguous run of its gated
//        pairs (select_wide, cape_pair_list.h).
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
#include "cape_map_camera.h"
#include "cape_pair_list.h"
#include "cape_ring_area.h"
#include "cape_wave.h"

namespace cape {

namespace {

constexpr int WP = CAPE_MATCH_WIDE_MAX_PLANES;
static_assert(WP == 2 * 64, "a lane holds kept planes k and k + 64");
constexpr int kWideGateFrames = 4;   // frames (waves) of a gate workgroup
constexpr int kWideSelectFrames = 4; // frames (waves) of a select workgroup

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
    const unsigned long long first = reserve_pairs<kWideGateFrames>(p.list, s_count, s_base, live ? myCount : 0u);
    if (!live)
        return;
    const bool listed = claim_frame(p.list, frame, first, myCount);
    if (lane == 0)
    {
        cape_frame_match_wide& out = p.frames[frame];
        out.n_prev = nPrevAll;
        out.n_cur = nCurAll;
        out.flags = (fits && listed) ? 0u : (uint32_t)CAPE_MATCH_EXACT_OVERFLOW;
        out.n_matched = 0;
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
                p.list.work[w] = pack_pair64(frame, j, lane);
                p.list.workArea[w] = nan_code(kNanPending);
            }
            if ((m1 >> lane) & 1ull)
            {
                const unsigned long long w = at + (unsigned)(__popcll(m0) + __popcll(m1 & below));
                p.list.work[w] = pack_pair64(frame, j, lane + 64);
                p.list.workArea[w] = nan_code(kNanPending);
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

// One tier of the list's walk (walk_tier, cape_pair_list.h).  A triple beyond every tier's capacities keeps a NaN that names the
// resource: its frame is flagged by the select kernel.
template <int TIER>
__global__ __launch_bounds__(64 * Tier<TIER>::kWavesPerGroup) void cape_wide_inter_kernel(MatchWideParams p, int ldsPerWave)
{
    using T = Tier<TIER>;
    walk_tier<TIER>(
        p.list, ldsPerWave, kTiers - 1,
        [&](const TierCtx<TIER>& ctx, unsigned long long e) -> double {
            const MpLds& L = ctx.L;
            const int frame = (int)(e >> 32), j = (int)((e >> 8) & 0xFFFFFFu), i = (int)(e & 255u);
            const KeptPolygon D = kept_polygon(p, frame, i), Q = prev_polygon(p, frame, j);
            const cape_polygon& PS = *D.polygon; // detected polygon
            const cape_polygon& PQ = *Q.polygon; // projected polygon
            const int na = (int)PS.vertex_count, nb = (int)PQ.vertex_count;
            if (na > T::kRing || nb > T::kRing)
                return nan_code(kNanRing);
            const double2* vertsC = D.ring();
            const double2* vertsP = Q.ring();
            for (int v = ctx.tid; v < na; v += ctx.kStride)
                L.ringA[v] = vertsC[v];
            // the frame the previous plane's polygon lives in: its own, or -- with a pose -- the one to_camera_space gives it
            // (polygon_coordinates.cpp:135-165), its ring moved by transform_boundary (polygon.cpp:430-451) and oriented by the
            // explicit-ring constructor (polygon.cpp:236-266); then Polygon::project into the frame of plane i, the projected ring
            // re-oriented clockwise like every polygon (OpenRing constructor)
            if (p.poses)
            {
                const double* Tm = p.poses + (size_t)frame * 16;
                const CameraFrame F = camera_frame(Tm, PQ.center, PQ.x_axis, PQ.y_axis);
                for (int v = ctx.tid; v < nb; v += ctx.kStride)
                    L.ringB[v] = to_camera_vertex(Tm, F, vertsP[v]);
                ctx.sync();
                orient_ring(L.ringB, nb, false, ctx);
                project_ring_b(ctx, L.ringB, nb, F.nc, F.nx, F.ny, PS);
            }
            else
                project_ring_b(ctx, vertsP, nb, PQ.center, PQ.x_axis, PQ.y_axis, PS);
            ctx.sync();
            orient_ring(L.ringB, nb, false, ctx);
            return ctx.inter_area(na, nb);
        },
        [&](size_t idx, unsigned long long e, double result) {
            const int frame = (int)(e >> 32), j = (int)((e >> 8) & 0xFFFFFFu), i = (int)(e & 255u);
            p.list.workArea[idx] = result;
            if (p.areas)
                p.areas[((size_t)frame * WP + j) * WP + i] = result;
        });
}

// One wavefront per frame (select_wide, cape_pair_list.h): the previous planes in order; a previous plane without a positive area
// matches nothing.
__global__ __launch_bounds__(64 * kWideSelectFrames) void cape_wide_select_kernel(MatchWideParams p, int nFrames)
{
    const int frame = blockIdx.x * kWideSelectFrames + (threadIdx.x >> 6);
    if (frame >= nFrames)
        return;
    select_wide<true, false>(
        p.list, frame, p.frames[frame], p.flags, p.minOverlap, p.match + (size_t)frame * WP, nullptr,
        [&](int k) { return kept_polygon(p, frame, k).polygon->area; }, [&](int k) { return prev_polygon(p, frame, k).polygon->area; });
}

hipError_t launch_carry_save(const CarrySaveParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_wide_carry_save_kernel, dim3(1), dim3(64), carry_save_layout().bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_match_wide(const MatchWideParams& p, int nFrames, hipStream_t stream)
{
    if (const hipError_t e = hipMemsetAsync(p.list.counts, 0, 16 * sizeof(unsigned), stream); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(cape_wide_gate_kernel, dim3((nFrames + kWideGateFrames - 1) / kWideGateFrames), dim3(64 * kWideGateFrames),
                       wide_gate_layout().bytes, stream, p, nFrames);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_tier<0>(cape_wide_inter_kernel<0>, p, stream); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_tier<1>(cape_wide_inter_kernel<1>, p, stream); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_tier<2>(cape_wide_inter_kernel<2>, p, stream); e != hipSuccess)
        return e;
    // (a ring is a subset of its plane's candidates; a device without the LDS for the largest tier leaves its triples NaN: their
    // frames are flagged)
    if (p.boundaryCapacity > Tier<2>::kRing && tier_lds_bytes<3>() <= (size_t)p.ldsLimitBytes)
        if (const hipError_t e = launch_tier<3>(cape_wide_inter_kernel<3>, p, stream); e != hipSuccess)
            return e;
    hipLaunchKernelGGL(cape_wide_select_kernel, dim3((nFrames + kWideSelectFrames - 1) / kWideSelectFrames), dim3(64 * kWideSelectFrames), 0, stream, p,
                       nFrames);
    return hipGetLastError();
}

} // namespace cape

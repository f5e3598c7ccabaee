// Row N2 against a persistent MAP: Feature_Map::get_matches (reference src/map_management/feature_map.hpp:638-697) -- every map
// plane in turn runs MapPlane::find_matches (map_primitive.cpp:91-161) against the detected planes of a frame, seen through the
// frame's worldToCamera, a detected plane taken by an earlier map plane being skipped by the later ones.  The map planes live
// in world coordinates and their polygons (grown by merge_union) may have holes; they stay on the device between batches
// (cape_map_upload).
//
//   cape_map_gate_kernel /
//   cape_map_gate_shards_kernel  : one wavefront per frame, lanes over map planes: plane_to_camera of map plane j
//        (plane_coordinates.cpp:20-24), the gates is_distance_similar / is_normal_similar (shape_primitives.cpp:66-86) against
//        every kept plane i of the frame; for a map plane with a gated pair, the area of its polygon seen from the camera
//        (to_camera_space, polygon_coordinates.cpp:135-165, holes included) -- <= 0: it matches nothing and lists no pair --
//        and the work list of the gated (frame, j, i) triples, per frame in (j, i) order (reserve_pairs, cape_pair_list.h).
//   cape_map_inter_kernel<TIER>  : the walk of the list through the capacity tiers (walk_tier, cape_pair_list.h) around one triple's
//        area: every ring of the map polygon goes through to_camera_space (cape_map_camera.h) and is projected into the detected
//        plane's frame (project_ring_b) and oriented (orient_ring), and
//        inter = I(detected, outer) - I(detected, hole_k) in order, clamped at 0 -- Polygon::inter_area of the host class
//        (host/boundary_polygon.cpp: polygons_inter_area).  The capacity tiers and the intersection are cape_ring_area.h's.
//   cape_map_select_kernel       : one wavefront per frame: map plane after map plane in order, lanes over the gated pairs of
//        the plane; wave arg-max of the area above the overlap threshold (lowest index on a tie), the `selectedIndex <= 0`
//        quirk, the is-matched mask.
//
// The detected planes come from one of three SOURCES, a template parameter of the kernels (detected_polygon): the records and polygon
// rows of the handle's last batch (cape_match_map), gathered shards in device memory (cape_match_map_shards: the packed lists of
// cape_gather.hip with CAPE_GATHER_POLYGONS, a "frame" being a slot shard x frames_capacity + k), or the frame's whole record CHAIN
// (cape_match_map_wide: up to 128 kept planes in record order, those of spill records included).  The shard source has a gate
// kernel of its own, cape_map_gate_shards_kernel, which finds the kept planes among the frame's packed polygons and checks every
// index it reads from the shard -- the bytes come from another process -- before the shared part of the gate kernels
// (gate_kept_planes) takes over.  The chain source has a gate and a select kernel of its own, twice as wide:
//
//   cape_map_gate_wide_kernel    : one wavefront per frame: the chain is walked into the frame's kept-plane table (walk_chain,
//        cape_chain_walk.h), a lane holds kept planes k and k + 64; lanes over the map planes, 64 at a time, both gates on all
//        n_map x n_cur pairs as a 128-bit mask per map plane, the projected polygon measured once per map plane with a gated pair,
//        the triples appended in (j, i) order with one atomic per workgroup.
//   cape_map_select_wide_kernel  : cape_map_select_kernel with runs of up to 128 gated pairs (select_wide, cape_pair_list.h).
//
// The intersection kernel is the same for the three: only the accessor differs.
//
// + - x / and comparisons only, in the host class's association order (-ffp-contract=off): the areas are compared BIT FOR BIT
// with the host twin cape_host_match_map (tests/test_gpu_map_match.py).
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

constexpr int kMapGateFrames = 4;   // frames (waves) of a gate workgroup
constexpr int kMapSelectFrames = 4; // frames (waves) of a select workgroup
constexpr int WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
static_assert(WP == 2 * 64, "a lane holds kept planes k and k + 64");
// a triple is (frame << 32) | (j << 8) | i: i takes 8 bits, j the 24 above them
static_assert(WP - 1 <= 0xFF && CAPE_MAX_PLANES - 1 <= 0xFF && CAPE_MAP_MAX_PLANES - 1 <= 0xFFFFFF, "the triple packing holds every (j, i)");

// where the detected planes of a call come from
enum MapSource
{
    kFromRecords, // the first record of each frame of the handle's batch (cape_match_map)
    kFromShards,  // gathered shards (cape_match_map_shards)
    kFromChain    // the frame's whole record chain (cape_match_map_wide)
};
// kept planes a frame of the source holds at most = entries per map plane of the dense area table
template <MapSource kSource> constexpr int kSourcePlanes = kSource == kFromChain ? WP : CAPE_MAX_PLANES;

// map plane j seen from the frame's camera (plane_to_camera of cape_map_camera.h)
__device__ __forceinline__ void plane_to_camera(const double* T, const cape_map_plane& M, double pn[3], double& pd)
{
    plane_to_camera(T, M.normal, M.d, pn, pd);
}

// Polygon::area of the map polygon seen from the camera > 0 (one lane, sequentially): the outer ring's |signed area| minus the
// holes', each ring measured in the orientation the host class gives it (OpenRing constructor / add_hole reverse a ring, and the
// area of the reversed ring is summed in the reversed order)
__device__ inline bool projected_area_positive(const double* Tm, const MatchMapParams& p, int j)
{
    const cape_map_plane& M = p.mapPlanes[j];
    const CameraFrame F = camera_frame(Tm, M);
    double area = 0.0;
    for (int k = 0; k < (int)M.ring_count; ++k)
    {
        const cape_map_ring R = p.mapRings[M.ring_first + k];
        const double2* src = p.mapVertices + R.vertex_offset;
        const int n = (int)R.vertex_count;
        double s = 0;
        double2 prev = to_camera_vertex(Tm, F, src[n - 1]);
        for (int i = 0; i < n; ++i)
        {
            const double2 cur = to_camera_vertex(Tm, F, src[i]);
            s += (prev.x * cur.y - cur.x * prev.y);
            prev = cur;
        }
        double sa = 0.5 * s;
        if (k == 0 ? sa > 0 : sa < 0)
        {
            s = 0;
            prev = to_camera_vertex(Tm, F, src[0]); // (the reversed ring's last vertex)
            for (int i = 0; i < n; ++i)
            {
                const double2 cur = to_camera_vertex(Tm, F, src[n - 1 - i]);
                s += (prev.x * cur.y - cur.x * prev.y);
                prev = cur;
            }
            sa = 0.5 * s;
        }
        area = k == 0 ? fabs(sa) : area - fabs(sa);
    }
    return area > 0.0;
}

// Kept plane i of a frame as the intersection and selection kernels see it: its polygon record and the vertex array its
// vertex_offset counts in.  kFromRecords: the polygon row and vertex slab of the frame's record; kFromShards: the polygon and vertex
// sections of the slot's shard, through the kept-plane table the shard gate kernel filled (and checked); kFromChain: the polygon row
// and vertex slab of the record the plane lives in, the batch's or a spill record, through the kept-plane table of the wide gate kernel.
struct DetectedPolygon
{
    const cape_polygon* polygon;
    const double2* vertices;
    __device__ __forceinline__ const double2* ring() const { return vertices + polygon->vertex_offset; }
};
template <MapSource kSource> __device__ __forceinline__ DetectedPolygon detected_polygon(const MatchMapParams& p, int frame, int i)
{
    if constexpr (kSource == kFromChain)
    {
        const uint2 at = p.keptIndex[(size_t)frame * WP + i]; // (record, segment in that record)
        return {p.polygons + (size_t)at.x * CAPE_MAX_PLANES + at.y, p.vertices + (size_t)at.x * p.boundaryCapacity};
    }
    else if constexpr (kSource == kFromShards)
    {
        const uint2 at = p.keptIndex[(size_t)frame * CAPE_MAX_PLANES + i]; // (packed index, shard)
        const unsigned char* shard = p.shards + (size_t)at.y * p.shardBytes;
        return {reinterpret_cast<const cape_polygon*>(shard + p.polygonsOffset) + at.x, reinterpret_cast<const double2*>(shard + p.verticesOffset)};
    }
    else
    {
        const int si = p.frames[frame].seg_cur[i];
        return {p.polygons + (size_t)frame * CAPE_MAX_PLANES + si, p.vertices + (size_t)frame * p.boundaryCapacity};
    }
}

// The part the gate kernels share, one wavefront per frame with lane i holding kept plane i (its segment index, normal and d; nCur
// of them), lanes over the map planes (64 at a time): the detected planes are broadcast; bit i of a lane's mask = pair (j, i) passes
// the gates.  Pass 1 counts the pairs (one atomic per workgroup reserves the frame's slots) and keeps the masks, pass 2 writes the
// triples in (j, i) order.  A frame that does not fit (`fits` false) gates nothing and is flagged `flagged | CAPE_MATCH_EXACT_OVERFLOW`.
__device__ __forceinline__ void gate_kept_planes(const MatchMapParams& p, int frame, bool live, int nCur, bool fits, uint32_t flagged, int seg,
                                                 double cn0, double cn1, double cn2, double cd, unsigned* s_count, unsigned long long& s_base)
{
    const int lane = threadIdx.x & 63;
    cape_frame_map_match& out = p.frames[frame];
    const double* T = p.poses + (size_t)frame * 16;
    const uint32_t* skip = p.skip ? p.skip + (size_t)frame * p.skipWords : nullptr;
    // the gated detected planes of map plane j (lane's), as a mask over i
    auto gate = [&](int j) -> unsigned long long {
        if (!fits || j >= p.nMap || (skip && ((skip[j >> 5] >> (j & 31)) & 1u)))
            return 0ull;
        double qn[3], qd;
        plane_to_camera(T, p.mapPlanes[j], qn, qd);
        unsigned long long m = 0ull;
        for (int i = 0; i < nCur; ++i)
        {
            const double sn0 = readlane_f64(cn0, i), sn1 = readlane_f64(cn1, i), sn2 = readlane_f64(cn2, i), sd = readlane_f64(cd, i);
            const double cosAngle = (sn0 * qn[0] + sn1 * qn[1]) + sn2 * qn[2];
            if (fabs(sd - qd) < p.maxDistance && fabs(cosAngle) > p.minCosAngle)
                m |= 1ull << i;
        }
        // a map plane whose projected polygon has no positive area matches nothing (map_primitive.cpp:105-106): its pairs are not
        // listed (their areas stay -1)
        if (m && !projected_area_positive(T, p, j))
            m = 0ull;
        return m;
    };
    unsigned long long* masks = p.gateMasks + (size_t)frame * p.nMap;
    unsigned myCount = 0;
    for (int jb = 0; jb < p.nMap; jb += 64)
    {
        const int j = jb + lane;
        const unsigned long long m = gate(j);
        if (live && j < p.nMap)
            masks[j] = m;
        myCount += (unsigned)wave_sum_i32(__popcll(m));
    }
    const unsigned long long first = reserve_pairs<kMapGateFrames>(p.list, s_count, s_base, live ? myCount : 0u);
    if (!live)
        return;
    const bool listed = claim_frame(p.list, frame, first, myCount);
    if (lane == 0)
    {
        out.n_map = p.nMap;
        out.n_cur = nCur;
        out.flags = (fits && listed) ? 0u : flagged | (uint32_t)CAPE_MATCH_EXACT_OVERFLOW;
        out.n_matched = 0;
    }
    out.seg_cur[lane] = lane < nCur ? seg : -1;
    out.map_of[lane] = -1;
    unsigned long long at = first;
    for (int jb = 0; jb < p.nMap; jb += 64)
    {
        const int j = jb + lane;
        const unsigned long long m = j < p.nMap ? masks[j] : 0ull;
        if (j < p.nMap)
            p.match[(size_t)frame * p.nMap + j] = -1;
        const int c = __popcll(m);
        const int incl = wave_scan_i32(c);
        if (listed)
        {
            unsigned long long w = at + (unsigned)(incl - c);
            for (unsigned long long mm = m; mm; mm &= mm - 1, ++w)
            {
                p.list.work[w] = pack_pair64(frame, j, __ffsll((long long)mm) - 1);
                p.list.workArea[w] = nan_code(kNanPending);
            }
        }
        at += (unsigned)__builtin_amdgcn_readlane(incl, 63);
        if (p.areas)
        {
            // the dense table: -1 where the pair is not gated (the intersection kernel overwrites the gated ones; a pair that is
            // never intersected -- a frame beyond the list -- keeps the NaN)
            const int rows = p.nMap - jb < 64 ? p.nMap - jb : 64;
            for (int l = 0; l < rows; ++l)
            {
                const unsigned long long ml = readlane_u64(m, l);
                p.areas[((size_t)frame * p.nMap + jb + l) * CAPE_MAX_PLANES + lane] = ((ml >> lane) & 1ull) ? nan_code(kNanPending) : -1.0;
            }
        }
    }
}

} // namespace

// The gate kernel of the record source: the kept planes of the frame's first record (valid_planes), normal and d out of its segments.
__global__ __launch_bounds__(64 * kMapGateFrames) void cape_map_gate_kernel(MatchMapParams p, int nFrames)
{
    __shared__ unsigned s_count[kMapGateFrames];
    __shared__ unsigned long long s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frameRaw = blockIdx.x * kMapGateFrames + wave;
    const bool live = frameRaw < nFrames;
    const int frame = live ? frameRaw : nFrames - 1; // (idle waves of the last workgroup shadow a real frame and store nothing)
    const cape_frame_record& rec = p.records[frame];
    const cape_polygon* pol = p.polygons + (size_t)frame * CAPE_MAX_PLANES;
    int seg = -1;
    bool hostOnly = false;
    const int nCur = valid_planes(rec, pol, lane, seg, hostOnly);
    double cn0 = 0, cn1 = 0, cn2 = 0, cd = 0;
    if (seg >= 0)
    {
        const cape_plane_segment& S = rec.segments[seg];
        cn0 = S.out_normal[0], cn1 = S.out_normal[1], cn2 = S.out_normal[2], cd = S.d;
    }
    gate_kept_planes(p, frame, live, nCur, !hostOnly, 0u, seg, cn0, cn1, cn2, cd, s_count, s_base);
}

// The gate kernel of the shard source, one wavefront per slot (shard x framesCapacity + k).  The shard's bytes were written by
// another process: the header is compared with the layout the caller gave (a mismatch flags every slot of the shard
// CAPE_MATCH_EXACT_BAD_SHARD and nothing else of it is read), and every index read from the shard -- the frame's run of planes, the
// end of each ring -- is checked against its section before it is used; what the intersection and selection kernels dereference later
// (keptIndex, the rings of the kept polygons) has passed here.  The frame's packed polygons are walked 64 at a time: a ballot of
// the kept ones (CAPE_POLY_VALID, >= 3 vertices) plus the running count ranks them, kept plane i's packed index goes to lane i
// through LDS, and lane i reads its normal, d and segment out of the plane section.
__global__ __launch_bounds__(64 * kMapGateFrames) void cape_map_gate_shards_kernel(MatchMapParams p, int nSlots)
{
    __shared__ unsigned s_count[kMapGateFrames];
    __shared__ unsigned long long s_base;
    __shared__ int s_kept[kMapGateFrames][CAPE_MAX_PLANES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slotRaw = blockIdx.x * kMapGateFrames + wave;
    const bool live = slotRaw < nSlots;
    const int slot = live ? slotRaw : nSlots - 1; // (idle waves of the last workgroup shadow a real slot and store nothing)
    const int shardIndex = slot / p.framesCapacity, k = slot - shardIndex * p.framesCapacity;
    const unsigned char* shard = p.shards + (size_t)shardIndex * p.shardBytes;
    const cape_packed_header hd = *reinterpret_cast<const cape_packed_header*>(shard);
    bool bad = hd.magic != CAPE_PACKED_MAGIC || !(hd.flags & CAPE_GATHER_POLYGONS) || hd.frames_capacity != p.framesCapacity ||
               hd.planes_capacity != p.planesCapacity || hd.cells != p.cells || hd.n_frames < 0 || hd.n_frames > p.framesCapacity;
    if (!bad)
        bad = reinterpret_cast<const cape_packed_polygon_header*>(shard + p.polygonHeaderOffset)->vertices_capacity != p.verticesCapacity;
    // (every condition below is uniform over the wave: header and frame entry are, the per-polygon ones go through a ballot)
    bool overflow = false; // the frame is left to the host: more than 64 kept planes, a polygon the host class builds, dropped planes / rings
    int kept = 0;
    s_kept[wave][lane] = -1;
    if (!bad && k < hd.n_frames)
    {
        const cape_packed_frame fr = reinterpret_cast<const cape_packed_frame*>(shard + p.framesOffset)[k];
        // planes beyond the section: the shard dropped them when its header says so, otherwise the entry is not a frame of this shard
        const bool dropped = (long long)fr.plane_offset + fr.n_planes > (long long)p.planesCapacity;
        if (fr.plane_offset < 0 || fr.n_planes < 0 || (dropped && !(hd.overflow & CAPE_PACKED_PLANES_DROPPED)))
            bad = true;
        else
        {
            overflow = dropped;
            const int first = fr.plane_offset;
            const int listed = !dropped ? fr.n_planes : (first < p.planesCapacity ? p.planesCapacity - first : 0);
            const cape_polygon* polygons = reinterpret_cast<const cape_polygon*>(shard + p.polygonsOffset);
            for (int b = 0; b < listed; b += 64)
            {
                const bool has = b + lane < listed;
                uint32_t flags = 0u, count = 0u, offset = 0u;
                if (has)
                {
                    const cape_polygon& g = polygons[first + b + lane];
                    flags = g.flags, count = g.vertex_count, offset = g.vertex_offset;
                }
                const bool away = offset == UINT32_MAX; // the ring did not travel (CAPE_PACKED_VERTICES_DROPPED): kept or not cannot be told
                const bool outside = !away && count > 0u && (unsigned long long)offset + count > (unsigned long long)p.verticesCapacity;
                const bool ok = (flags & CAPE_POLY_VALID) != 0u && count >= 3u;
                bad = bad || __any(outside);
                overflow = overflow || __any(away || (flags & CAPE_POLY_OVERFLOW) != 0u);
                const unsigned long long m = __ballot(ok);
                const int rank = kept + __popcll(m & ((1ull << lane) - 1ull));
                if (ok && rank < CAPE_MAX_PLANES)
                    s_kept[wave][rank] = first + b + lane;
                kept += __popcll(m);
            }
            overflow = overflow || kept > CAPE_MAX_PLANES;
        }
    }
    CAPE_MP_SYNC(); // (the table is read by other lanes of the wave than wrote it)
    const int nCur = bad ? 0 : (kept < CAPE_MAX_PLANES ? kept : CAPE_MAX_PLANES);
    const int mine = lane < nCur ? s_kept[wave][lane] : -1;
    if (live)
        p.keptIndex[(size_t)slot * CAPE_MAX_PLANES + lane] = make_uint2((unsigned)mine, (unsigned)shardIndex);
    int seg = -1;
    double cn0 = 0, cn1 = 0, cn2 = 0, cd = 0;
    if (mine >= 0)
    {
        const cape_packed_plane& P = reinterpret_cast<const cape_packed_plane*>(shard + p.planesOffset)[mine];
        cn0 = P.normal[0], cn1 = P.normal[1], cn2 = P.normal[2], cd = P.d;
        seg = (int)P.segment;
    }
    gate_kept_planes(p, slot, live, nCur, !bad && !overflow, bad ? (uint32_t)CAPE_MATCH_EXACT_BAD_SHARD : 0u, seg, cn0, cn1, cn2, cd, s_count, s_base);
}

// ---- the LDS carve of a wide gate workgroup, in byte offsets: the reservation's hand-over words, then per wave the frame's
// kept-plane table (location and position in the segment list)
struct MapGateWideLayout
{
    size_t base, count, kept, seg, bytes;
};
__host__ __device__ constexpr MapGateWideLayout map_gate_wide_layout()
{
    Layout l;
    MapGateWideLayout o{};
    o.base = l.take<unsigned long long>(1);
    o.count = l.take<unsigned>(kMapGateFrames);
    o.kept = l.take<uint2>((size_t)kMapGateFrames * WP, 16);
    o.seg = l.take<int>((size_t)kMapGateFrames * WP, 16);
    o.bytes = l.end(16);
    return o;
}

// The gate kernel of the chain source, one wavefront per frame: the chain is walked into the frame's kept-plane table, lane k reads
// the normal and d of kept planes k and k + 64 out of the segments of the records they live in; then lanes over the map planes (64
// at a time) as in gate_kept_planes, the detected planes broadcast out of either half: bit i of a lane's mask pair = pair (j, i)
// passes the gates.  Pass 1 counts the pairs (one atomic per workgroup reserves the frame's slots) and keeps the masks, pass 2
// writes the triples in (j, i) order.  A frame that keeps more than WP planes, or one with a plane left to the host class, gates
// nothing and is flagged with its true count.
__global__ __launch_bounds__(64 * kMapGateFrames) void cape_map_gate_wide_kernel(MatchMapParams p, int nFrames)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr MapGateWideLayout lay = map_gate_wide_layout();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long& s_base = *carve_at<unsigned long long>(smem, lay.base);
    unsigned* s_count = carve_at<unsigned>(smem, lay.count);
    uint2* kept = carve_at<uint2>(smem, lay.kept) + (size_t)wave * WP;
    int* segs = carve_at<int>(smem, lay.seg) + (size_t)wave * WP;
    const int frameRaw = blockIdx.x * kMapGateFrames + wave;
    const bool live = frameRaw < nFrames;
    const int frame = live ? frameRaw : nFrames - 1; // (idle waves of the last workgroup shadow a real frame and store nothing)
    bool hostOnly = false;
    const RecordChains chains{p.records, p.polygons, p.maxBatch, p.nRecords};
    const int head = p.chainBase + frame; // the frame's own record, where its chain starts
    const int nCurAll = walk_chain(chains, head, lane, kept, segs, hostOnly);
    CAPE_MP_SYNC(); // (the table is read by other lanes of the wave than wrote it)
    const bool fits = nCurAll <= WP && !hostOnly;
    const int nCur = nCurAll < WP ? nCurAll : WP;
    // my planes' parametrisations, read once (lane k: kept planes k and k + 64)
    double cn[2][3] = {{0, 0, 0}, {0, 0, 0}}, cd[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 2; ++s)
    {
        const int k = lane + 64 * s;
        if (live)
        {
            const size_t at = (size_t)frame * WP + k;
            p.keptIndex[at] = k < nCur ? kept[k] : make_uint2((unsigned)head, 0u);
            p.segCur[at] = k < nCur ? segs[k] : -1;
            p.mapOf[at] = -1;
        }
        if (k < nCur)
        {
            const uint2 at = kept[k];
            const cape_plane_segment& S = p.records[at.x].segments[at.y];
            cn[s][0] = S.out_normal[0], cn[s][1] = S.out_normal[1], cn[s][2] = S.out_normal[2], cd[s] = S.d;
        }
    }
    const double* T = p.poses + (size_t)frame * 16;
    const uint32_t* skip = p.skip ? p.skip + (size_t)frame * p.skipWords : nullptr;
    const int nLo = nCur < 64 ? nCur : 64;
    // the gated detected planes of map plane j (lane's), as two masks over i: planes 0..63 and 64..127
    auto gate = [&](int j, unsigned long long& m0, unsigned long long& m1) {
        m0 = m1 = 0ull;
        if (!fits || j >= p.nMap || (skip && ((skip[j >> 5] >> (j & 31)) & 1u)))
            return;
        double qn[3], qd;
        plane_to_camera(T, p.mapPlanes[j], qn, qd);
        for (int i = 0; i < nLo; ++i)
        {
            const double sn0 = readlane_f64(cn[0][0], i), sn1 = readlane_f64(cn[0][1], i), sn2 = readlane_f64(cn[0][2], i), sd = readlane_f64(cd[0], i);
            const double cosAngle = (sn0 * qn[0] + sn1 * qn[1]) + sn2 * qn[2];
            if (fabs(sd - qd) < p.maxDistance && fabs(cosAngle) > p.minCosAngle)
                m0 |= 1ull << i;
        }
        for (int i = 64; i < nCur; ++i)
        {
            const double sn0 = readlane_f64(cn[1][0], i - 64), sn1 = readlane_f64(cn[1][1], i - 64), sn2 = readlane_f64(cn[1][2], i - 64),
                         sd = readlane_f64(cd[1], i - 64);
            const double cosAngle = (sn0 * qn[0] + sn1 * qn[1]) + sn2 * qn[2];
            if (fabs(sd - qd) < p.maxDistance && fabs(cosAngle) > p.minCosAngle)
                m1 |= 1ull << (i - 64);
        }
        // a map plane whose projected polygon has no positive area matches nothing (map_primitive.cpp:105-106): its pairs are not
        // listed (their areas stay -1)
        if ((m0 | m1) && !projected_area_positive(T, p, j))
            m0 = m1 = 0ull;
    };
    unsigned long long* masks = p.gateMasks + (size_t)frame * p.nMap * 2; // [j][half of the detected planes]
    unsigned myCount = 0;
    for (int jb = 0; jb < p.nMap; jb += 64)
    {
        const int j = jb + lane;
        unsigned long long m0, m1;
        gate(j, m0, m1);
        if (live && j < p.nMap)
            masks[2 * j] = m0, masks[2 * j + 1] = m1;
        myCount += (unsigned)wave_sum_i32(__popcll(m0) + __popcll(m1));
    }
    // ONE atomic per workgroup on the list's counter reserves the slots of its frames
    const unsigned long long first = reserve_pairs<kMapGateFrames>(p.list, s_count, s_base, live ? myCount : 0u);
    if (!live)
        return;
    const bool listed = claim_frame(p.list, frame, first, myCount);
    if (lane == 0)
    {
        cape_frame_map_match_wide& out = p.framesWide[frame];
        out.n_map = p.nMap;
        out.n_cur = nCurAll;
        out.flags = (fits && listed) ? 0u : (uint32_t)CAPE_MATCH_EXACT_OVERFLOW;
        out.n_matched = 0;
    }
    unsigned long long at = first;
    for (int jb = 0; jb < p.nMap; jb += 64)
    {
        const int j = jb + lane;
        const unsigned long long m0 = j < p.nMap ? masks[2 * j] : 0ull, m1 = j < p.nMap ? masks[2 * j + 1] : 0ull;
        if (j < p.nMap)
            p.match[(size_t)frame * p.nMap + j] = -1;
        const int c = __popcll(m0) + __popcll(m1);
        const int incl = wave_scan_i32(c);
        if (listed)
        {
            unsigned long long w = at + (unsigned)(incl - c);
            for (unsigned long long mm = m0; mm; mm &= mm - 1, ++w)
            {
                p.list.work[w] = pack_pair64(frame, j, __ffsll((long long)mm) - 1);
                p.list.workArea[w] = nan_code(kNanPending);
            }
            for (unsigned long long mm = m1; mm; mm &= mm - 1, ++w)
            {
                p.list.work[w] = pack_pair64(frame, j, 64 + __ffsll((long long)mm) - 1);
                p.list.workArea[w] = nan_code(kNanPending);
            }
        }
        at += (unsigned)__builtin_amdgcn_readlane(incl, 63);
        if (p.areas)
        {
            // the dense table: -1 where the pair is not gated (the intersection kernel overwrites the gated ones; a pair that is
            // never intersected -- a frame beyond the list -- keeps the NaN)
            const int rows = p.nMap - jb < 64 ? p.nMap - jb : 64;
            for (int l = 0; l < rows; ++l)
            {
                const unsigned long long l0 = readlane_u64(m0, l), l1 = readlane_u64(m1, l);
                double* row = p.areas + ((size_t)frame * p.nMap + jb + l) * WP;
                row[lane] = ((l0 >> lane) & 1ull) ? nan_code(kNanPending) : -1.0;
                row[lane + 64] = ((l1 >> lane) & 1ull) ? nan_code(kNanPending) : -1.0;
            }
        }
    }
}

// One tier of the list's walk (walk_tier, cape_pair_list.h).  A triple beyond every tier's capacities keeps a NaN that names the
// resource: its frame is flagged by the select kernel.
template <int TIER, MapSource kSource>
__global__ __launch_bounds__(64 * Tier<TIER>::kWavesPerGroup) void cape_map_inter_kernel(MatchMapParams p, int ldsPerWave)
{
    using T = Tier<TIER>;
    walk_tier<TIER>(
        p.list, ldsPerWave, kTiers - 1,
        [&](const TierCtx<TIER>& ctx, unsigned long long e) -> double {
            const MpLds& L = ctx.L;
            const int frame = (int)(e >> 32), j = (int)((e >> 8) & 0xFFFFFFu), i = (int)(e & 255u);
            const DetectedPolygon D = detected_polygon<kSource>(p, frame, i);
            const cape_polygon& PS = *D.polygon; // detected polygon
            const cape_map_plane& M = p.mapPlanes[j];
            const int na = (int)PS.vertex_count, nRings = (int)M.ring_count;
            int nbMax = 0;
            for (int k = 0; k < nRings; ++k)
            {
                const int nb = (int)p.mapRings[M.ring_first + k].vertex_count;
                nbMax = nb > nbMax ? nb : nbMax;
            }
            if (na > T::kRing || nbMax > T::kRing)
                return nan_code(kNanRing);
            const double2* vertsC = D.ring();
            for (int v = ctx.tid; v < na; v += ctx.kStride)
                L.ringA[v] = vertsC[v];
            const double* Tm = p.poses + (size_t)frame * 16;
            const CameraFrame F = camera_frame(Tm, M); // to_camera_space (polygon_coordinates.cpp:135-165)
            // (the projected polygon's area was found positive by the gate kernel: only such map planes list pairs)
            double acc = 0.0, result = 0.0;
            for (int k = 0; k < nRings; ++k)
            {
                // ring k of the map polygon into ring B, seen from the camera (transform_boundary, polygon.cpp:430-451), in the
                // orientation the host class gives it: the outer one clockwise (OpenRing constructor), holes counter-clockwise (add_hole)
                const cape_map_ring R = p.mapRings[M.ring_first + k];
                const double2* src = p.mapVertices + R.vertex_offset;
                const int nb = (int)R.vertex_count;
                for (int v = ctx.tid; v < nb; v += ctx.kStride)
                    L.ringB[v] = to_camera_vertex(Tm, F, src[v]);
                ctx.sync();
                orient_ring(L.ringB, nb, k > 0, ctx);
                // ... projected into the detected plane's frame (Polygon::project, polygon.cpp:338-382), oriented again
                project_ring_b(ctx, L.ringB, nb, F.nc, F.nx, F.ny, PS);
                ctx.sync();
                orient_ring(L.ringB, nb, k > 0, ctx);
                const double r = ctx.inter_area(na, nb);
                if (r != r)
                    return r;
                acc = k == 0 ? r : acc - r; // polygons_inter_area: I(A, B) - I(A, hole_k) in order
                result = acc < 0 ? 0.0 : acc;
            }
            return result;
        },
        [&](size_t idx, unsigned long long e, double result) {
            const int frame = (int)(e >> 32), j = (int)((e >> 8) & 0xFFFFFFu), i = (int)(e & 255u);
            p.list.workArea[idx] = result;
            if (p.areas)
                p.areas[((size_t)frame * p.nMap + j) * kSourcePlanes<kSource> + i] = result;
        });
}

// One wavefront per frame: the map planes in order, each with the contiguous run of its gated pairs (one run fits the wave: at
// most 64 kept planes), lanes over the run.
template <MapSource kSource> __global__ __launch_bounds__(64 * kMapSelectFrames) void cape_map_select_kernel(MatchMapParams p, int nFrames)
{
    const int lane = threadIdx.x & 63;
    const int frame = blockIdx.x * kMapSelectFrames + (threadIdx.x >> 6);
    if (frame >= nFrames)
        return;
    cape_frame_map_match& out = p.frames[frame];
    if (out.flags & CAPE_MATCH_EXACT_OVERFLOW)
        return; // nothing was intersected
    const int nc = out.n_cur;
    const double myArea = lane < nc ? detected_polygon<kSource>(p, frame, lane).polygon->area : 0.0; // detectedPolygon.get_area()
    const uint2 range = p.list.frameRange[frame];
    const unsigned begin = range.x, end = range.x + range.y;
    // a pair beyond the intersection kernel's capacities: no match is reported for the frame
    bool nan = false;
    for (unsigned k = begin + lane; k < end; k += 64)
        nan |= p.list.workArea[k] != p.list.workArea[k];
    if (__any(nan))
    {
        if (lane == 0)
            out.flags |= CAPE_MATCH_EXACT_OVERFLOW;
        return;
    }
    unsigned long long taken = 0ull; // is-matched flags of the detected planes
    int myMapOf = -1, nMatched = 0;
    for (unsigned at = begin; at < end;)
    {
        const unsigned k = at + lane;
        const bool valid = k < end;
        const unsigned long long e = valid ? p.list.work[k] : 0ull;
        const double ia = valid ? p.list.workArea[k] : -1.0;
        const int jl = (int)((e >> 8) & 0xFFFFFFu), i = (int)(e & 255u);
        const int j = __builtin_amdgcn_readfirstlane(jl);
        const bool mine = valid && jl == j;
        const double detArea = __shfl(myArea, i);
        // interArea > greatestSimilarity (starting at 0) and interArea / newPlaneArea >= threshold (map_primitive.cpp:137-143); the
        // run is in ascending i and the comparison strict: the lowest index among the largest areas
        unsigned long long key = 0;
        if (mine && !((taken >> i) & 1ull) && ia > 0.0 && ia / detArea >= p.minOverlap)
            key = (unsigned long long)__double_as_longlong(ia);
        const unsigned long long best = ~wave_min_u64(~key);
        const unsigned long long winners = __ballot(key != 0 && key == best);
        int selected = winners ? __shfl(i, __ffsll((long long)winners) - 1) : -1;
        if (!(p.flags & CAPE_MATCH_ALLOW_INDEX0) && selected <= 0) // map_primitive.cpp:146
            selected = -1;
        if (selected >= 0)
        {
            taken |= 1ull << selected;
            ++nMatched;
            if (lane == selected)
                myMapOf = j;
            if (lane == 0)
                p.match[(size_t)frame * p.nMap + j] = selected;
        }
        at += (unsigned)__popcll(__ballot(mine));
    }
    if (lane == 0)
        out.n_matched = nMatched;
    out.map_of[lane] = myMapOf;
}

// The select kernel of the chain source, one wavefront per frame (select_wide, cape_pair_list.h): the map planes in order; which
// map plane took a kept plane goes to the frame's row of mapOf.
__global__ __launch_bounds__(64 * kMapSelectFrames) void cape_map_select_wide_kernel(MatchMapParams p, int nFrames)
{
    const int frame = blockIdx.x * kMapSelectFrames + (threadIdx.x >> 6);
    if (frame >= nFrames)
        return;
    select_wide<false, true>(
        p.list, frame, p.framesWide[frame], p.flags, p.minOverlap, p.match + (size_t)frame * p.nMap, p.mapOf + (size_t)frame * WP,
        [&](int k) { return detected_polygon<kFromChain>(p, frame, k).polygon->area; }, [](int) { return 0.0; });
}

namespace {

template <MapSource kSource> hipError_t launch_match_map_from(const MatchMapParams& p, int nFrames, hipStream_t stream)
{
    if (const hipError_t e = hipMemsetAsync(p.list.counts, 0, 16 * sizeof(unsigned), stream); e != hipSuccess)
        return e;
    const dim3 gateGrid((nFrames + kMapGateFrames - 1) / kMapGateFrames), gateGroup(64 * kMapGateFrames);
    if constexpr (kSource == kFromChain)
        hipLaunchKernelGGL(cape_map_gate_wide_kernel, gateGrid, gateGroup, map_gate_wide_layout().bytes, stream, p, nFrames);
    else
        hipLaunchKernelGGL(kSource == kFromShards ? cape_map_gate_shards_kernel : cape_map_gate_kernel, gateGrid, gateGroup, 0, stream, p, nFrames);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_tier<0>(cape_map_inter_kernel<0, kSource>, p, stream); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_tier<1>(cape_map_inter_kernel<1, kSource>, p, stream); e != hipSuccess)
        return e;
    if (const hipError_t e = launch_tier<2>(cape_map_inter_kernel<2, kSource>, p, stream); e != hipSuccess)
        return e;
    // (a device without the LDS for the largest tier leaves its triples NaN: their frames are flagged)
    if (tier_lds_bytes<3>() <= (size_t)p.ldsLimitBytes)
        if (const hipError_t e = launch_tier<3>(cape_map_inter_kernel<3, kSource>, p, stream); e != hipSuccess)
            return e;
    const dim3 selectGrid((nFrames + kMapSelectFrames - 1) / kMapSelectFrames), selectGroup(64 * kMapSelectFrames);
    if constexpr (kSource == kFromChain)
        hipLaunchKernelGGL(cape_map_select_wide_kernel, selectGrid, selectGroup, 0, stream, p, nFrames);
    else
        hipLaunchKernelGGL(cape_map_select_kernel<kSource>, selectGrid, selectGroup, 0, stream, p, nFrames);
    return hipGetLastError();
}

} // namespace

// nFrames: frames of the handle's batch, or slots when p.shards is set (cape_match_map_shards)
hipError_t launch_match_map(const MatchMapParams& p, int nFrames, hipStream_t stream)
{
    return p.shards ? launch_match_map_from<kFromShards>(p, nFrames, stream) : launch_match_map_from<kFromRecords>(p, nFrames, stream);
}

// cape_match_map_wide: nFrames frames of the handle's batch, each over its whole record chain
hipError_t launch_match_map_wide(const MatchMapParams& p, int nFrames, hipStream_t stream)
{
    return launch_match_map_from<kFromChain>(p, nFrames, stream);
}

} // namespace cape

// The state half of the map update (Feature_Map::update_map, host twin cape_host_map_kalman in host/polygon_capi.cpp) up to, but not
// including, the polygon union: what MapPlane::update_with_match does with a matched detection's measurement -- the Kalman step, the
// triple normalisation of the new normal, the frame update_boundary_polygon projects into -- and the update_matched /
// update_unmatched counters with the promote / drop / lost decisions.  It reads the uploaded map and tracks, the match of the last
// cape_match_map_wide and the rows of the last cape_map_measure, and writes only its own result buffers: every frame sees the same map
// and the same tracks, so every (frame, map plane) is independent.
//
//   cape_map_kalman_kernel : one wavefront per frame, four per workgroup, no block barrier.
//        Pass 1, lanes over the kept planes (i and i + 64): the lane reads map_of[f][i] and, if a map plane j took the plane (and
//        match[f][j] says so too), the plane and track of j and kept plane i's measurement row -- found through the kept-plane
//        table of the wide match, (record, segment), both checked against the row buffer -- runs the steps and writes its own fusion
//        row: one writer per row.  The pair's result bits go to the wave's 128-entry LDS array, tagged with j.
//        Pass 2, after a wave-level sync, lanes over the map planes 64 at a time: match[f][j], the pair's bits out of LDS (if the
//        tag is j), the counters and decisions, one 16-byte store per map plane.
//   A frame the wide match flagged CAPE_MATCH_EXACT_OVERFLOW reports nothing: its rows and track results are zeros.
//
// Everything is + - x / sqrt in the order of the host twin (-ffp-contract=off) and equals it bit for bit.
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_layout.h"
#include "cape_map_tracking.h"
#include "cape_ring_area.h"
#include "cape_wave.h"

namespace cape {

namespace {

constexpr int kKalmanFrames = 4; // frames (waves) of a workgroup
constexpr int kKalmanPlanes = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
static_assert(kKalmanPlanes == 128, "a lane serves kept planes i and i + 64");
static_assert(sizeof(cape_map_track_result) == 16 && sizeof(cape_plane_fusion) % 16 == 0, "16-byte stores");

// the wave's result words: bits [0, 16) the pair's CAPE_MAP_RESULT_* bits, bits [16, 32) the map plane + 1 (0: unmatched)
struct MapKalmanLayout
{
    size_t bits, bytes;
};
__host__ __device__ constexpr MapKalmanLayout map_kalman_layout()
{
    Layout l;
    MapKalmanLayout o{};
    o.bits = l.take<unsigned>((size_t)kKalmanFrames * kKalmanPlanes, 16);
    o.bytes = l.end(16);
    return o;
}
static_assert(CAPE_MAP_MAX_PLANES < (1 << 16), "the map plane fits the tag");

constexpr uint32_t kMeasureNoDetection = CAPE_MEASURE_FAIL_PLANE_COV | CAPE_MEASURE_FAIL_WORLD_COV | CAPE_MEASURE_BAD_POSE_COV;

// One matched pair, one lane: M, K the map plane and its track, m the detection's measurement row (null: the kept-plane table points
// outside the row buffer).  Fills the row's state and frame as far as the steps get and returns the pair's result bits.
__device__ __forceinline__ uint32_t fuse_pair(const cape_map_plane& M, const MapTrackState& K, const cape_plane_measurement* m, cape_plane_fusion& row)
{
    uint32_t result = CAPE_MAP_RESULT_MATCHED;
    const uint32_t mflags = m ? m->flags : 0u;
    if (!(mflags & CAPE_MEASURE_KEPT) || (mflags & kMeasureNoDetection))
        return result | CAPE_MAP_RESULT_FAIL_DETECTION;
    double P[16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        P[k] = K.covariance[k];
    if (!is_covariance_valid<4>(P))
        return result | CAPE_MAP_RESULT_FAIL_STATE;
    double R[16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        R[k] = m->covariance[k];
    const double x[4] = {M.normal[0], M.normal[1], M.normal[2], M.d}, z[4] = {m->normal[0], m->normal[1], m->normal[2], m->d};
    double xn[4], Pn[16];
    const int st = kalman_update(x, P, z, R, xn, Pn);
    if (st == kKalmanSingular)
        return result | CAPE_MAP_RESULT_FAIL_SINGULAR;
    if (st != kKalmanOk)
        return result | CAPE_MAP_RESULT_FAIL_KALMAN;
    // PlaneWorldCoordinates(vector4), its copy and the assignment each normalise the normal (plane_coordinates.hpp:19-32)
    double n[3] = {xn[0], xn[1], xn[2]};
    normalize3(n);
    normalize3(n);
    normalize3(n);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        row.normal[k] = n[k];
    row.d = xn[3];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        row.covariance[k] = Pn[k];
    row.flags |= CAPE_FUSION_STATE;
    // Plane::update_boundary_polygon (plane_with_tracking.cpp:63-82): Polygon::project's unit check, the target frame
    bool ok = fabs(norm3(n) - 1.0) <= kDblEpsilon;
    if (ok)
    {
        double ax[3], ay[3];
        ok = plane_coordinate_system(n, ax, ay);
        if (ok)
        {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                row.x_axis[k] = ax[k], row.y_axis[k] = ay[k], row.center[k] = n[k] * -xn[3];
            row.flags |= CAPE_FUSION_FRAME;
        }
    }
    ok = ok && !(mflags & CAPE_MEASURE_FAIL_POLYGON);
    return result | (ok ? CAPE_MAP_RESULT_UPDATED : CAPE_MAP_RESULT_FAIL_POLYGON);
}

} // namespace

__global__ __launch_bounds__(64 * kKalmanFrames) void cape_map_kalman_kernel(MapKalmanParams p, int nFrames)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr MapKalmanLayout lay = map_kalman_layout();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* bits = carve_at<unsigned>(smem, lay.bits) + (size_t)wave * kKalmanPlanes;
    const int frame = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kKalmanFrames + wave));
    if (frame >= nFrames) // (idle waves of the last workgroup; the kernel has no barrier)
        return;
    const cape_frame_map_match_wide hd = p.matchFrames[frame];
    const int nMap = p.nMap;
    const bool reports = !(hd.flags & CAPE_MATCH_EXACT_OVERFLOW);
    const int nCur = !reports ? 0 : (hd.n_cur < 0 ? 0 : (hd.n_cur > kKalmanPlanes ? kKalmanPlanes : hd.n_cur));
    cape_plane_fusion* rows = p.rows + (size_t)frame * kKalmanPlanes;
    const int32_t* match = p.match + (size_t)frame * nMap;
    // ---- pass 1: the kept planes
    bool badPose = false;
#pragma unroll 1
    for (int s = 0; s < 2; ++s)
    {
        const int i = lane + 64 * s;
        cape_plane_fusion row{};
        unsigned word = 0u;
        bool myBadPose = false;
        if (i < nCur)
        {
            row.map_plane = -1;
            // kept plane i's measurement row, through the wide match's table: (record, segment in that record)
            const uint2 at = p.kept[(size_t)frame * kKalmanPlanes + i];
            const cape_plane_measurement* m =
                (at.x < (unsigned)p.nRecords && at.y < (unsigned)CAPE_MAX_PLANES) ? p.measurements + (size_t)at.x * CAPE_MAX_PLANES + at.y : nullptr;
            myBadPose = m && (m->flags & CAPE_MEASURE_BAD_POSE_COV) != 0;
            const int j = p.mapOf[(size_t)frame * kKalmanPlanes + i];
            if (j >= 0 && j < nMap && match[j] == i)
            {
                row.map_plane = j;
                const uint32_t result = fuse_pair(p.mapPlanes[j], p.tracks[j], m, row);
                if ((result & CAPE_MAP_RESULT_UPDATED) || (p.tracks[j].flags & CAPE_MAP_TRACK_STAGED))
                    row.flags |= CAPE_FUSION_USED;
                word = result | ((unsigned)(j + 1) << 16);
            }
        }
        rows[i] = row;
        bits[i] = word;
        badPose = badPose || __any(myBadPose) != 0; // (wave-uniform)
    }
    CAPE_MP_SYNC(); // (the words are read by other lanes of the wave than wrote them)
    // ---- pass 2: the map planes
    int nUpdated = 0;
    cape_map_track_result* out = p.trackResults + (size_t)frame * nMap;
    for (int jb = 0; jb < nMap; jb += 64)
    {
        const int j = jb + lane;
        bool updated = false;
        if (j < nMap)
        {
            cape_map_track_result r{};
            if (reports)
            {
                const int i = match[j];
                const unsigned word = (i >= 0 && i < nCur) ? bits[i] : 0u;
                const bool mine = (word >> 16) == (unsigned)(j + 1);
                const MapTrackState& K = p.tracks[j];
                uint32_t result = mine ? (word & 0xFFFFu) : 0u;
                int32_t successive = K.successiveMatched;
                uint32_t failed = K.failedTracking;
                const bool staged = (K.flags & CAPE_MAP_TRACK_STAGED) != 0;
                updated = (result & CAPE_MAP_RESULT_UPDATED) != 0;
                if (updated)
                {
                    failed = 0;
                    successive = (int32_t)((uint32_t)successive + 1u);
                }
                else
                {
                    ++failed;
                    successive = (int32_t)((uint32_t)successive - 1u);
                }
                if (staged && successive >= 4)
                    result |= CAPE_MAP_RESULT_PROMOTE;
                else if (staged && failed >= 2)
                    result |= CAPE_MAP_RESULT_DROP;
                else if (!staged && failed >= 10)
                    result |= CAPE_MAP_RESULT_LOST;
                r.result = result;
                r.successive_matched = successive;
                r.failed_tracking = failed;
                r.kept_plane = mine ? i : -1;
            }
            *reinterpret_cast<uint4*>(out + j) = make_uint4(r.result, (unsigned)r.successive_matched, r.failed_tracking, (unsigned)r.kept_plane);
        }
        nUpdated += __popcll(__ballot(updated));
    }
    if (lane == 0)
    {
        cape_frame_map_kalman f;
        f.n_map = nMap;
        f.n_cur = hd.n_cur;
        f.flags = (hd.flags & CAPE_MATCH_EXACT_OVERFLOW) | (reports && badPose ? (uint32_t)CAPE_KALMAN_BAD_POSE_COV : 0u);
        f.n_updated = nUpdated;
        p.frames[frame] = f;
    }
}

hipError_t launch_map_kalman(const MapKalmanParams& p, int nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_map_kalman_kernel, dim3((nFrames + kKalmanFrames - 1) / kKalmanFrames), dim3(64 * kKalmanFrames), map_kalman_layout().bytes, stream, p,
                       nFrames);
    return hipGetLastError();
}

} // namespace cape

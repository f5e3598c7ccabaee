// The measurement half of the map update (Feature_Map::update_map, host twin cape_host_map_update in host/polygon_capi.cpp): what
// MapPlane::update_with_match computes of a detection before the Kalman step and what the StagedMapPlane constructor computes of an
// unmatched one -- the detection's plane covariance, the plane in world coordinates, the world plane covariance, the polygon in world
// space.  It reads neither the map nor a match, so every plane of every frame is independent.
//
//   cape_map_measure_kernel : one wavefront per frame, four per workgroup.  The wave follows the frame's record chain with the hop
//        bound of walk_chain (cape_chain_walk.h); in each record lane s owns segment s, kept by walk_chain's rule (output plane,
//        CAPE_POLY_VALID, >= 3 vertices) -- no limit on the planes of a frame, a CAPE_POLY_OVERFLOW plane is simply not kept.  The
//        lane of a kept plane runs the algebra of cape_map_tracking.h and writes the plane's row; every other lane writes a row of
//        zeros.  Then the whole wave walks the rings of the record's kept planes, one after the other, 64 vertices at a time: the
//        ring goes to the wave's LDS ring, is oriented like the host class orients the detection's ring (reversed when its signed
//        area, the ordered sum, is positive), goes through to_camera_vertex with the camera-to-world matrix, is oriented again like
//        the constructor of the transformed polygon does, and lands in the record's world-vertex slab at the polygon's offset (the
//        ring of a kept plane that failed a step is zeroed).  Every lane recomputes the plane's world frame from the polygon row for
//        that (the statements of the owning lane on the same operands: the same bits) instead of 18 cross-lane reads.
//
// The world plane, the polygon frame and the ring are + - x / sqrt in the order of the host twin (-ffp-contract=off) and equal it bit
// for bit; the covariances go through pow and are compared with a tolerance (tests/test_gpu_map_measure.py).
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_map_camera.h"
#include "cape_map_tracking.h"
#include "cape_ring_area.h"

namespace cape {

namespace {

constexpr int kMeasureFrames = 4; // frames (waves) of a workgroup

// One kept plane, one lane.  T, S: the frame's camera-to-world matrix and pose covariance; poseOk: is_covariance_valid(S, 3), decided
// once per frame; inSlab: the wave can serve the ring; ringOk: the polygon step passed, the wave writes the world ring.
__device__ __forceinline__ cape_plane_measurement measure_plane(const cape_plane_segment& seg, const cape_polygon& g, const double* T,
                                                                const double* S, bool poseOk, bool inSlab, bool& ringOk)
{
    cape_plane_measurement m{};
    m.flags = CAPE_MEASURE_KEPT;
    ringOk = false;
    if (!poseOk)
    {
        m.flags |= CAPE_MEASURE_BAD_POSE_COV;
        return m;
    }
    double n[3], cov[9];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        n[k] = seg.out_normal[k];
#pragma unroll
    for (int k = 0; k < 9; ++k)
        cov[k] = seg.cov[k];
    const double d = seg.d;
    double planeCov[16], worldCov[16];
    if (!plane_covariance(n, d, cov, planeCov))
    {
        m.flags |= CAPE_MEASURE_FAIL_PLANE_COV;
        return m;
    }
    if (!world_plane_covariance(n, d, T, planeCov, S, worldCov))
    {
        m.flags |= CAPE_MEASURE_FAIL_WORLD_COV;
        return m;
    }
    // the Kalman measurement of update_with_match; the staged plane's normal is normalised once more (the assignment to
    // _parametrization in the StagedMapPlane constructor)
    double nw[3], dw;
    plane_to_world(n, d, T, nw, dw);
    double sn[3] = {nw[0], nw[1], nw[2]};
    normalize3(sn);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        m.normal[k] = nw[k], m.staged_normal[k] = sn[k];
    m.d = dw;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        m.covariance[k] = worldCov[k];
    // CameraPolygon::to_world_space (polygon_coordinates.cpp:48-75): the transformed axes re-normalised (camera_frame's statements),
    // both unit within DBL_EPSILON and orthogonal within .01; then the staged plane's own unit check
    const CameraFrame F = camera_frame(T, g.center, g.x_axis, g.y_axis);
    if (!(fabs(norm3(F.nx) - 1.0) <= kDblEpsilon) || !(fabs(norm3(F.ny) - 1.0) <= kDblEpsilon) ||
        fabs((F.ny[0] * F.nx[0] + F.ny[1] * F.nx[1]) + F.ny[2] * F.nx[2]) > .01 || !(fabs(norm3(sn) - 1.0) <= kDblEpsilon) || !inSlab)
    {
        m.flags |= CAPE_MEASURE_FAIL_POLYGON;
        return m;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        m.x_axis[k] = F.nx[k], m.y_axis[k] = F.ny[k], m.center[k] = F.nc[k];
    m.vertex_offset = g.vertex_offset;
    m.vertex_count = g.vertex_count;
    ringOk = true;
    m.flags |= g.vertex_count > CAPE_MAP_MAX_RING ? CAPE_MEASURE_RING_TOO_LONG : CAPE_MEASURE_STAGEABLE;
    return m;
}

// the orientation the host class gives an outer ring (both ring constructors): reversed when its signed area is positive.  One
// wavefront on a ring in LDS: every lane reads the whole ring (ring_area_signed: the ordered sum) before any lane rewrites it
__device__ __forceinline__ void orient(double2* ring, int n, int lane)
{
    const double s = ring_area_signed(ring, n);
    CAPE_MP_SYNC();
    if (s > 0)
    {
        for (int v = lane; v < n / 2; v += 64)
        {
            const double2 a = ring[v], b = ring[n - 1 - v];
            ring[v] = b;
            ring[n - 1 - v] = a;
        }
        CAPE_MP_SYNC();
    }
}

} // namespace

__global__ __launch_bounds__(64 * kMeasureFrames) void cape_map_measure_kernel(MapMeasureParams p, int nFrames)
{
    __shared__ double2 s_ring[kMeasureFrames][kPolyMaxPoints]; // a wave's ring on its way to the world
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double2* ring = s_ring[wave];
    const int frame = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kMeasureFrames + wave)); // (wave-uniform: scalar loads below)
    if (frame >= nFrames) // (idle waves of the last workgroup; the kernel has no barrier)
        return;
    double T[16], S[9];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        T[k] = p.poses[(size_t)frame * 16 + k];
#pragma unroll
    for (int k = 0; k < 9; ++k)
        S[k] = p.poseCov[(size_t)frame * 9 + k];
    const bool poseOk = is_covariance_valid<3>(S);
    const unsigned cap = (unsigned)p.boundaryCapacity;
    int rec = frame;
    // the chain is followed through at most as many links as the pool has records, and a link outside the pool ends it (walk_chain)
    for (int hop = 0; hop <= p.nRecords - p.maxBatch; ++hop)
    {
        const cape_frame_record& R = p.records[rec];
        const cape_polygon* pol = p.polygons + (size_t)rec * CAPE_MAX_PLANES;
        int nSeg = R.header.n_plane_segments;
        nSeg = nSeg < 0 ? 0 : (nSeg > CAPE_MAX_PLANES ? CAPE_MAX_PLANES : nSeg);
        const bool isOut = lane < nSeg && R.segments[lane].is_output != 0;
        const unsigned flags = isOut ? pol[lane].flags : 0u;
        const bool kept = isOut && (flags & CAPE_POLY_VALID) != 0 && pol[lane].vertex_count >= 3;
        // a ring the wave can serve lies inside the record's slab and fits the wave's LDS ring (a longer one is CAPE_POLY_OVERFLOW)
        const bool inSlab = kept && pol[lane].vertex_count <= (unsigned)kPolyMaxPoints && pol[lane].vertex_offset <= cap &&
                            pol[lane].vertex_count <= cap - pol[lane].vertex_offset;
        cape_plane_measurement m{};
        bool ringOk = false;
        if (kept)
            m = measure_plane(R.segments[lane], pol[lane], T, S, poseOk, inSlab, ringOk);
        p.rows[(size_t)rec * CAPE_MAX_PLANES + lane] = m;
        // the rings, by the whole wave
        unsigned long long todo = __ballot(inSlab);
        const unsigned long long good = __ballot(ringOk);
        const double2* src = p.vertices + (size_t)rec * cap;
        double2* dst = p.worldVertices + (size_t)rec * cap;
        while (todo)
        {
            const int i = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const cape_polygon& g = pol[i];
            const int off = (int)g.vertex_offset, n = (int)g.vertex_count;
            if ((good >> i) & 1ull)
            {
                // the detection as the host class holds it (the explicit-ring constructor orients the ring), through
                // to_camera_space with T (transform_boundary, then the OpenRing constructor orients the result)
                const CameraFrame F = camera_frame(T, g.center, g.x_axis, g.y_axis);
                for (int v = lane; v < n; v += 64)
                    ring[v] = src[off + v];
                CAPE_MP_SYNC();
                orient(ring, n, lane);
                for (int v = lane; v < n; v += 64)
                    ring[v] = to_camera_vertex(T, F, ring[v]);
                CAPE_MP_SYNC();
                orient(ring, n, lane);
                for (int v = lane; v < n; v += 64)
                    dst[off + v] = ring[v];
                CAPE_MP_SYNC(); // (the next plane rewrites the ring)
            }
            else
                for (int v = lane; v < n; v += 64)
                    dst[off + v] = make_double2(0.0, 0.0);
        }
        const int next = __builtin_amdgcn_readfirstlane(R.header.next_record);
        if (next < p.maxBatch || next >= p.nRecords)
            break;
        rec = next;
    }
}

hipError_t launch_map_measure(const MapMeasureParams& p, int nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_map_measure_kernel, dim3((nFrames + kMeasureFrames - 1) / kMeasureFrames), dim3(64 * kMeasureFrames), 0, stream, p, nFrames);
    return hipGetLastError();
}

} // namespace cape

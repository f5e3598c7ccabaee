// The polygon half of the map update (host twin cape_host_map_union in host/polygon_capi.cpp): for every pair cape_map_kalman reports
// as UPDATED, the map plane's new boundary polygon -- Polygon::project, merge_union and simplify of host/boundary_polygon.cpp, restated
// for one wavefront in cape_map_union.h -- for a map plane without holes whose union with the detection creates no hole.  Everything
// else is reported as the host's, per pair.  It reads the uploaded map, the match of the last cape_match_map_wide, the rows and world
// rings of the last cape_map_measure and the fusion rows of the last cape_map_kalman, and writes only its own result buffers: every
// frame sees the same map, so every (frame, pair) is independent.
//
//   cape_map_union_kernel : one wavefront per frame, one per workgroup, no block barrier.
//        Pass 1, lanes over the kept planes (i and i + 64): which kept planes have a pair; the rows of the others are written here
//        (map_plane = -1 below n_cur, zeros beyond), so that every row has one writer.
//        Pass 2, the wave walks the frame's pairs in kept-plane order: both rings into LDS, union_pair, the row, and a served ring
//        appended to the frame's slab -- the offsets are deterministic and there is no allocator.  A ring that does not fit the rest
//        of the slab is CAPE_UNION_HOST_CAPACITY.
//   cape_ring_union_kernel : the same per-pair function on one pair given by its rings and frames (cape_debug_ring_union).
//   A frame the wide match flagged CAPE_MATCH_EXACT_OVERFLOW reports nothing: its rows are zeros.
//   cape_map_union_rings_kernel<Cuts>, cape_polygon_union_kernel<Cuts> : the same two for the modes with rings, one template each
//        over union_pair_rings<Cuts>.  <false> is the holes mode (a map plane with interior rings, a union that encloses faces):
//        the same rows and slab, where a served polygon's rings lie back to back, plus a row of ring lengths per kept plane; a
//        larger carve (union_holes_layout).  <true> is the cut mode (a hole of the map plane that the detection covers in part is
//        cut into its pieces by a second arrangement inside the pair): the rows, slab, rings rows and carve size of the holes
//        mode, and the second arrangement's sorted cuts (union_cut_carve).  The <false> instantiations are the instructions the
//        holes kernels were before they were templates, and the cut call's median lies inside its former spread
//        (profiles/map_union_one_pair.txt).  All modes share the loading of a pair (load_map_pair, load_debug_pair).  Pass 1
//        stands twice, in cape_map_union_kernel and in union_find_pairs for the kernels with rings: called from both, it moved the
//        plain kernel's register allocation, and a call's median left the spread of the restated build
//        (profiles/map_union_shared_steps.txt).
//
// Every count read from the map, a row or a table is checked against its buffer before it indexes anything; every loop of union_pair
// is bounded by a capacity of the carve.
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_map_union.h"

namespace cape {

namespace {

constexpr int kUnionPlanes = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
static_assert(kUnionPlanes == 128, "a lane serves kept planes i and i + 64");

__device__ __forceinline__ void load_frame(UnionFrame& f, const double* x, const double* y, const double* c)
{
#pragma unroll
    for (int k = 0; k < 3; ++k)
        f.x[k] = x[k], f.y[k] = y[k], f.c[k] = c[k];
}

// a frame's pair into the carve (both frame kernels): the map plane's outer ring, the detection's world ring, and the frames of the
// map plane, the measurement and the fusion row.  The caller has checked the counts against the carve and the buffers.
__device__ __forceinline__ void load_map_pair(const UnionLds& L, const double2* srcA, unsigned nA, const double2* srcB, unsigned nB, const cape_map_plane& M,
                                              const cape_plane_measurement& m, const cape_plane_fusion& fu, UnionFrame& fa, UnionFrame& fb,
                                              UnionFrame& target, int lane)
{
    for (unsigned v = lane; v < nA; v += 64)
        L.ringA[v] = srcA[v];
    for (unsigned v = lane; v < nB; v += 64)
        L.ringB[v] = srcB[v];
    CAPE_MP_SYNC();
    load_frame(fa, M.x_axis, M.y_axis, M.center);
    load_frame(fb, m.x_axis, m.y_axis, m.center);
    load_frame(target, fu.x_axis, fu.y_axis, fu.center);
}

// ... and the pair of a debug kernel: two rings and 27 doubles, the frames of ring a, ring b and the target (x, y, centre each)
__device__ __forceinline__ void load_debug_pair(const UnionLds& L, const double2* ringA, int nA, const double2* ringB, int nB, const double* frames27,
                                                UnionFrame& fa, UnionFrame& fb, UnionFrame& target, int lane)
{
    for (int v = lane; v < nA; v += 64)
        L.ringA[v] = ringA[v];
    for (int v = lane; v < nB; v += 64)
        L.ringB[v] = ringB[v];
    CAPE_MP_SYNC();
    load_frame(fa, frames27, frames27 + 3, frames27 + 6);
    load_frame(fb, frames27 + 9, frames27 + 12, frames27 + 15);
    load_frame(target, frames27 + 18, frames27 + 21, frames27 + 24);
}

// the row of a pair from union_pair's result; a served ring goes to slab[used, used + n) if it fits `capacity`.  Returns the new `used`.
__device__ __forceinline__ unsigned put_pair(const UnionResult& res, const UnionFrame& frame, int mapPlane, cape_plane_union* row, double2* slab,
                                             unsigned used, unsigned capacity, int lane)
{
    cape_plane_union r{};
    r.map_plane = mapPlane;
    r.flags = res.flags;
    const bool served = (res.flags & CAPE_UNION_SERVED) != 0;
    const bool fits = served && res.n >= 0 && (unsigned)res.n <= capacity - used;
    if (served && !fits)
        r.flags = CAPE_UNION_HOST_CAPACITY;
    if (fits)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            r.x_axis[k] = frame.x[k], r.y_axis[k] = frame.y[k], r.center[k] = frame.c[k];
        r.area = res.area;
        r.vertex_offset = used;
        r.vertex_count = (uint32_t)res.n;
        r.n_nodes = (uint32_t)res.nNodes;
        for (int v = lane; v < res.n; v += 64)
            slab[used + v] = res.ring[v];
        used += (unsigned)res.n;
    }
    if (lane == 0)
        *row = r;
    return used;
}

// pass 1 of cape_map_union_kernel for the kernels with rings (a copy, kept for the measured reason at the head of this file), lanes over the kept planes (i and i + 64): which kept planes have a pair; the rows of the others
// are written here
__device__ __forceinline__ void union_find_pairs(const MapUnionParams& p, int frame, int nCur, cape_plane_union* rows, const cape_plane_fusion* fusion,
                                                 int lane, unsigned long long (&pairs)[2])
{
    const int nMap = p.nMap;
#pragma unroll 1
    for (int s = 0; s < 2; ++s)
    {
        const int i = lane + 64 * s;
        bool pair = false;
        if (i < nCur)
        {
            const int j = fusion[i].map_plane;
            const uint2 at = p.kept[(size_t)frame * kUnionPlanes + i];
            if (j >= 0 && j < nMap && (fusion[i].flags & CAPE_FUSION_FRAME) && at.x < (unsigned)p.nRecords && at.y < (unsigned)CAPE_MAX_PLANES)
            {
                const uint32_t mflags = p.measurements[(size_t)at.x * CAPE_MAX_PLANES + at.y].flags;
                pair = (mflags & CAPE_MEASURE_KEPT) && !(mflags & CAPE_MEASURE_FAIL_POLYGON) && p.match[(size_t)frame * nMap + j] == i;
            }
        }
        if (!pair)
        {
            cape_plane_union row{};
            row.map_plane = i < nCur ? -1 : 0;
            rows[i] = row;
        }
        pairs[s] = __ballot(pair);
    }
}

// the rows of a pair of the modes with rings: the outer ring and the interior rings go to slab[used, ...) back to back if the whole polygon
// fits `capacity`.  Returns the new `used`.
__device__ __forceinline__ unsigned put_pair_holes(const UnionResult& res, const UnionHoleResult& hr, const UnionHolesLds& H, const UnionFrame& frame, int mapPlane,
                                                   cape_plane_union* row, cape_plane_union_rings* ringRow, double2* slab, unsigned used,
                                                   unsigned capacity, int lane)
{
    cape_plane_union r{};
    cape_plane_union_rings q{};
    r.map_plane = mapPlane;
    r.flags = res.flags;
    const bool served = (res.flags & CAPE_UNION_SERVED) != 0;
    const int nHoles = served && hr.nHoles > 0 && hr.nHoles <= kUnionHoles ? hr.nHoles : 0;
    unsigned total = served && res.n >= 0 ? (unsigned)res.n : 0u;
    for (int k = 0; k < nHoles; ++k)
        total += (unsigned)uni(H.holeLen[k]);
    const bool fits = served && res.n >= 0 && total <= capacity - used;
    if (served && !fits)
        r.flags = CAPE_UNION_HOST_CAPACITY;
    if (fits)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            r.x_axis[k] = frame.x[k], r.y_axis[k] = frame.y[k], r.center[k] = frame.c[k];
        r.area = res.area;
        r.vertex_offset = used;
        r.vertex_count = (uint32_t)res.n;
        r.n_nodes = (uint32_t)res.nNodes;
        q.ring_count = 1u + (uint32_t)nHoles;
        q.vertex_count[0] = (uint32_t)res.n;
        q.holes_new = hr.holesNew;
        q.holes_kept = hr.holesKept;
        q.holes_covered = hr.holesCovered;
        for (int v = lane; v < res.n; v += 64)
            slab[used + v] = res.ring[v];
        const unsigned holesAt = used + (unsigned)res.n;
#pragma unroll
        for (int k = 0; k < kUnionHoles; ++k)
            q.vertex_count[1 + k] = k < nHoles ? (uint32_t)uni(H.holeLen[k]) : 0u;
        for (unsigned v = lane; v < total - (unsigned)res.n; v += 64)
            slab[holesAt + v] = H.holes[v];
        used += total;
    }
    if (lane == 0)
    {
        *row = r;
        *ringRow = q;
    }
    return used;
}

} // namespace

__global__ __launch_bounds__(64) void cape_map_union_kernel(MapUnionParams p, int nFrames)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const UnionLds L = union_carve(smem);
    const int lane = threadIdx.x & 63;
    const int frame = (int)blockIdx.x;
    if (frame >= nFrames)
        return;
    const cape_frame_map_match_wide hd = p.matchFrames[frame];
    const int nMap = p.nMap;
    const bool reports = !(hd.flags & CAPE_MATCH_EXACT_OVERFLOW);
    const int nCur = !reports ? 0 : (hd.n_cur < 0 ? 0 : (hd.n_cur > kUnionPlanes ? kUnionPlanes : hd.n_cur));
    cape_plane_union* rows = p.rows + (size_t)frame * kUnionPlanes;
    const cape_plane_fusion* fusion = p.fusion + (size_t)frame * kUnionPlanes;
    double2* slab = p.vertices + (size_t)frame * CAPE_MAP_UNION_FRAME_VERTICES;
    // ---- pass 1: which kept planes have a pair
    unsigned long long pairs[2];
#pragma unroll 1
    for (int s = 0; s < 2; ++s)
    {
        const int i = lane + 64 * s;
        bool pair = false;
        if (i < nCur)
        {
            const int j = fusion[i].map_plane;
            const uint2 at = p.kept[(size_t)frame * kUnionPlanes + i];
            if (j >= 0 && j < nMap && (fusion[i].flags & CAPE_FUSION_FRAME) && at.x < (unsigned)p.nRecords && at.y < (unsigned)CAPE_MAX_PLANES)
            {
                const uint32_t mflags = p.measurements[(size_t)at.x * CAPE_MAX_PLANES + at.y].flags;
                pair = (mflags & CAPE_MEASURE_KEPT) && !(mflags & CAPE_MEASURE_FAIL_POLYGON) && p.match[(size_t)frame * nMap + j] == i;
            }
        }
        if (!pair)
        {
            cape_plane_union row{};
            row.map_plane = i < nCur ? -1 : 0;
            rows[i] = row;
        }
        pairs[s] = __ballot(pair);
    }
    // ---- pass 2: the pairs in kept-plane order
    unsigned used = 0;
#pragma unroll 1
    for (int s = 0; s < 2; ++s)
    {
        unsigned long long todo = pairs[s];
        while (todo)
        {
            const int i = 64 * s + __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int j = uni(fusion[i].map_plane);
            const uint2 at = p.kept[(size_t)frame * kUnionPlanes + i];
            const int rec = uni((int)at.x);
            const cape_plane_measurement& m = p.measurements[(size_t)rec * CAPE_MAX_PLANES + uni((int)at.y)];
            const cape_map_plane& M = p.mapPlanes[j];
            UnionResult res{};
            UnionFrame frameOut{};
            const unsigned ringFirst = (unsigned)uni((int)M.ring_first), ringCount = (unsigned)uni((int)M.ring_count);
            if (ringCount > 1u)
                res.flags = CAPE_UNION_HOST_MAP_HOLES; // (decided before any geometry)
            else if (ringCount == 0u || ringFirst >= p.nMapRings)
                res.flags = CAPE_UNION_HOST_CAPACITY;
            else
            {
                const cape_map_ring R = p.mapRings[ringFirst];
                const unsigned nA = (unsigned)uni((int)R.vertex_count), offA = (unsigned)uni((int)R.vertex_offset);
                const unsigned nB = (unsigned)uni((int)m.vertex_count), offB = (unsigned)uni((int)m.vertex_offset);
                const unsigned cap = (unsigned)p.boundaryCapacity;
                if (nA > (unsigned)kUnionRing || nB > (unsigned)kUnionRing || nA < 3u || nB < 3u || (unsigned long long)offA + nA > p.nMapVertices ||
                    offB > cap || nB > cap - offB)
                    res.flags = CAPE_UNION_HOST_CAPACITY;
                else
                {
                    const double2* srcA = p.mapVertices + offA;
                    const double2* srcB = p.worldVertices + (size_t)rec * cap + offB;
                    UnionFrame fa, fb, target;
                    load_map_pair(L, srcA, nA, srcB, nB, M, m, fusion[i], fa, fb, target, lane);
                    res = union_pair(L, (int)nA, (int)nB, fa, fb, target, frameOut, lane);
                }
            }
            used = put_pair(res, frameOut, j, rows + i, slab, used, CAPE_MAP_UNION_FRAME_VERTICES, lane);
            CAPE_MP_SYNC(); // (the next pair rewrites the carve)
        }
    }
}

__global__ __launch_bounds__(64) void cape_ring_union_kernel(RingUnionParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const UnionLds L = union_carve(smem);
    const int lane = threadIdx.x & 63;
    UnionResult res{};
    UnionFrame frameOut{};
    if (p.nA > kUnionRing || p.nB > kUnionRing || p.nA < 3 || p.nB < 3)
        res.flags = CAPE_UNION_HOST_CAPACITY;
    else
    {
        UnionFrame fa, fb, target;
        load_debug_pair(L, p.ringA, p.nA, p.ringB, p.nB, p.frames27, fa, fb, target, lane);
        res = union_pair(L, p.nA, p.nB, fa, fb, target, frameOut, lane);
    }
    (void)put_pair(res, frameOut, 0, p.row, p.vertices, 0u, CAPE_MAP_MAX_RING, lane);
}

// The frame kernel of the modes with rings (Cuts = false: the holes mode, true: the cut mode): the walk above, with the map plane's
// interior rings described to union_pair_rings (every count and offset checked here) and the rings rows written beside the rows.
template <bool Cuts>
__global__ __launch_bounds__(64) void cape_map_union_rings_kernel(MapUnionParams p, cape_plane_union_rings* ringRowsAll, int nFrames)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const UnionLds L = union_carve(smem);
    UnionHolesLds H = union_holes_carve(smem, L);
    UnionCutLds C{}; // (the second arrangement's sorted cuts: the cut mode's alone)
    if constexpr (Cuts)
        C = union_cut_carve(smem);
    const int lane = threadIdx.x & 63;
    const int frame = (int)blockIdx.x;
    if (frame >= nFrames)
        return;
    const cape_frame_map_match_wide hd = p.matchFrames[frame];
    const bool reports = !(hd.flags & CAPE_MATCH_EXACT_OVERFLOW);
    const int nCur = !reports ? 0 : (hd.n_cur < 0 ? 0 : (hd.n_cur > kUnionPlanes ? kUnionPlanes : hd.n_cur));
    cape_plane_union* rows = p.rows + (size_t)frame * kUnionPlanes;
    cape_plane_union_rings* ringRows = ringRowsAll + (size_t)frame * kUnionPlanes;
    const cape_plane_fusion* fusion = p.fusion + (size_t)frame * kUnionPlanes;
    double2* slab = p.vertices + (size_t)frame * CAPE_MAP_UNION_FRAME_VERTICES;
    // ---- pass 1: which kept planes have a pair (the rings rows of the others: zeros)
    unsigned long long pairs[2];
    union_find_pairs(p, frame, nCur, rows, fusion, lane, pairs);
#pragma unroll 1
    for (int s = 0; s < 2; ++s)
        if (!((pairs[s] >> lane) & 1ull))
            ringRows[lane + 64 * s] = cape_plane_union_rings{};
    H.src = p.mapVertices;
    // ---- pass 2: the pairs in kept-plane order
    unsigned used = 0;
#pragma unroll 1
    for (int s = 0; s < 2; ++s)
    {
        unsigned long long todo = pairs[s];
        while (todo)
        {
            const int i = 64 * s + __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int j = uni(fusion[i].map_plane);
            const uint2 at = p.kept[(size_t)frame * kUnionPlanes + i];
            const int rec = uni((int)at.x);
            const cape_plane_measurement& m = p.measurements[(size_t)rec * CAPE_MAX_PLANES + uni((int)at.y)];
            const cape_map_plane& M = p.mapPlanes[j];
            UnionResult res{};
            UnionHoleResult holes{};
            UnionFrame frameOut{};
            const unsigned ringFirst = (unsigned)uni((int)M.ring_first), ringCount = (unsigned)uni((int)M.ring_count);
            const unsigned nB = (unsigned)uni((int)m.vertex_count), offB = (unsigned)uni((int)m.vertex_offset);
            const unsigned cap = (unsigned)p.boundaryCapacity;
            // every ring of the map plane: in its table, inside the vertex buffer, of 3 .. kUnionRing vertices
            bool fits = ringCount >= 1u && ringCount <= 1u + (unsigned)kUnionHoles && ringFirst < p.nMapRings && ringCount <= p.nMapRings - ringFirst &&
                        nB >= 3u && nB <= (unsigned)kUnionRing && offB <= cap && nB <= cap - offB;
            for (unsigned k = 0; fits && k < ringCount; ++k)
            {
                const cape_map_ring R = p.mapRings[ringFirst + k];
                const unsigned n = (unsigned)uni((int)R.vertex_count), off = (unsigned)uni((int)R.vertex_offset);
                fits = n >= 3u && n <= (unsigned)kUnionRing && (unsigned long long)off + n <= p.nMapVertices;
                if (fits && k > 0u && lane == 0)
                {
                    H.srcOff[k - 1u] = off;
                    H.srcLen[k - 1u] = (unsigned short)n;
                }
            }
            CAPE_MP_SYNC();
            if (!fits)
                res.flags = CAPE_UNION_HOST_CAPACITY;
            else
            {
                const cape_map_ring R = p.mapRings[ringFirst];
                const unsigned nA = (unsigned)uni((int)R.vertex_count), offA = (unsigned)uni((int)R.vertex_offset);
                const double2* srcA = p.mapVertices + offA;
                const double2* srcB = p.worldVertices + (size_t)rec * cap + offB;
                H.nSrc = (int)ringCount - 1;
                UnionFrame fa, fb, target;
                load_map_pair(L, srcA, nA, srcB, nB, M, m, fusion[i], fa, fb, target, lane);
                res = union_pair_rings<Cuts>(L, H, C, (int)nA, (int)nB, fa, fb, target, frameOut, holes, lane);
            }
            used = put_pair_holes(res, holes, H, frameOut, j, rows + i, ringRows + i, slab, used, CAPE_MAP_UNION_FRAME_VERTICES, lane);
            CAPE_MP_SYNC(); // (the next pair rewrites the carve)
        }
    }
}

// The same per-pair function on one pair given by ring a's rings (back to back, counts[nRingsA]), ring b and the frames
// (cape_debug_polygon_union, and cape_debug_polygon_union_cut with Cuts).  1 <= nRingsA <= 1 + kUnionHoles: the entry point has
// checked it.
template <bool Cuts>
__global__ __launch_bounds__(64) void cape_polygon_union_kernel(PolygonUnionParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const UnionLds L = union_carve(smem);
    UnionHolesLds H = union_holes_carve(smem, L);
    UnionCutLds C{};
    if constexpr (Cuts)
        C = union_cut_carve(smem);
    const int lane = threadIdx.x & 63;
    UnionResult res{};
    UnionHoleResult holes{};
    UnionFrame frameOut{};
    bool fits = p.nRingsA >= 1 && p.nRingsA <= 1 + kUnionHoles && p.nB >= 3 && p.nB <= kUnionRing;
    unsigned at = 0;
    for (int k = 0; fits && k < p.nRingsA; ++k)
    {
        const int n = uni(p.countsA[k]);
        fits = n >= 3 && n <= kUnionRing;
        if (fits && k > 0 && lane == 0)
        {
            H.srcOff[k - 1] = at;
            H.srcLen[k - 1] = (unsigned short)n;
        }
        at += fits ? (unsigned)n : 0u;
    }
    CAPE_MP_SYNC();
    if (!fits)
        res.flags = CAPE_UNION_HOST_CAPACITY;
    else
    {
        const int nA = uni(p.countsA[0]);
        H.src = p.ringsA;
        H.nSrc = p.nRingsA - 1;
        UnionFrame fa, fb, target;
        load_debug_pair(L, p.ringsA, nA, p.ringB, p.nB, p.frames27, fa, fb, target, lane);
        res = union_pair_rings<Cuts>(L, H, C, nA, p.nB, fa, fb, target, frameOut, holes, lane);
    }
    (void)put_pair_holes(res, holes, H, frameOut, 0, p.row, p.ringRow, p.vertices, 0u, CAPE_MAP_UNION_FRAME_VERTICES, lane);
}

hipError_t launch_map_union_cut(const MapUnionParams& p, cape_plane_union_rings* ringRows, int nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_map_union_rings_kernel<true>, dim3(nFrames), dim3(64), union_cut_layout().bytes, stream, p, ringRows, nFrames);
    return hipGetLastError();
}

hipError_t launch_polygon_union_cut(const PolygonUnionParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_polygon_union_kernel<true>, dim3(1), dim3(64), union_cut_layout().bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_map_union_holes(const MapUnionParams& p, cape_plane_union_rings* ringRows, int nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_map_union_rings_kernel<false>, dim3(nFrames), dim3(64), union_holes_layout().bytes, stream, p, ringRows, nFrames);
    return hipGetLastError();
}

hipError_t launch_polygon_union(const PolygonUnionParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_polygon_union_kernel<false>, dim3(1), dim3(64), union_holes_layout().bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_map_union(const MapUnionParams& p, int nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_map_union_kernel, dim3(nFrames), dim3(64), union_layout().bytes, stream, p, nFrames);
    return hipGetLastError();
}

hipError_t launch_ring_union(const RingUnionParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_ring_union_kernel, dim3(1), dim3(64), union_layout().bytes, stream, p);
    return hipGetLastError();
}

} // namespace cape

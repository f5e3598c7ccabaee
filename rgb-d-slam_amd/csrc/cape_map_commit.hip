// cape_map_commit: a frame's map update written into the device map (host twin cape_host_map_commit in host/polygon_capi.cpp; the
// rules are the plain functions of cape_map_commit.h).  It reads the uploaded map and tracks and the result buffers of
// cape_map_kalman, cape_map_measure and cape_map_union[_holes|_cut] and writes the BACK buffers of the map, the tracks and their
// ids; the host swaps front and back once the header says DONE.  No floating-point statement: every double is copied.
//
//   cape_map_commit_plan_kernel : ONE workgroup of 256 lanes.  Lane t decides map planes 4 t .. 4 t + 3 (1024 at the most) with
//        commit_map_plane -- the source (old map or union slab), the ring and vertex counts, the refusal causes -- and lanes 0 .. 127
//        decide kept planes t with commit_appends.  Four exclusive scans (rings and vertices of the map planes; planes and vertices
//        of the appended ones) run as a wave scan on the DPP path (cape_wave.h) and a step across the four waves through LDS; the
//        refusal bits and the counts are reduced the same way.  Lane 0 writes the result header with the capacity check
//        (commit_result) and, if it says DONE, every lane the plan rows of its planes.
//   cape_map_commit_copy_kernel : one workgroup per output plane, 256 lanes.  It leaves at once unless the header says DONE.  Lane 0
//        writes the plane record, the track, the id / result and the ring records; all lanes copy the vertices, a 16-byte load and
//        store per vertex.
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_layout.h"
#include "cape_map_commit.h"
#include "cape_wave.h"

namespace cape {

namespace {

constexpr int kCommitLanes = 256, kCommitWaves = kCommitLanes / 64, kCommitPerLane = 4;
static_assert(kCommitLanes * kCommitPerLane == CAPE_MAP_MAX_PLANES, "four map planes per lane");
static_assert(kCommitMaxAppended <= kCommitLanes, "one kept plane per lane");
static_assert(sizeof(double2) == 16 && sizeof(cape_map_ring) == 8, "16-byte vertex copies");

// per wave, the totals the other waves need: of the map planes, then of the appended ones
enum { kSumRings, kSumVertices, kSumRefusal, kSumUpdated, kSumHostPairs, kSumFailPolygon, kSumAppended, kSumAppendedVertices, kSumWords };
struct MapCommitLayout
{
    size_t sums, bytes;
};
__host__ __device__ constexpr MapCommitLayout map_commit_layout()
{
    Layout l;
    MapCommitLayout o{};
    o.sums = l.take<int>((size_t)kCommitWaves * kSumWords, 16);
    o.bytes = l.end(16);
    return o;
}

// kept plane i's measurement row through the wide match's table, or -1: (record, segment) outside the row buffer
__device__ __forceinline__ long long measurement_row(const MapCommitParams& p, int i)
{
    const uint2 at = p.kept[i];
    return (at.x < (unsigned)p.nRecords && at.y < (unsigned)CAPE_MAX_PLANES) ? (long long)at.x * CAPE_MAX_PLANES + at.y : -1ll;
}

} // namespace

__global__ __launch_bounds__(kCommitLanes) void cape_map_commit_plan_kernel(MapCommitParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr MapCommitLayout lay = map_commit_layout();
    int* sums = carve_at<int>(smem, lay.sums);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const cape_frame_map_kalman hd = *p.kalmanFrame;
    const int nCur = commit_kept_planes(hd);
    const int nMap = p.nMap < 0 ? 0 : (p.nMap > CAPE_MAP_MAX_PLANES ? CAPE_MAP_MAX_PLANES : p.nMap);

    // ---- the map planes: four per lane, in order
    CommitItem items[kCommitPerLane];
    CommitTotals mine{};
    int myRings = 0, myVertices = 0;
#pragma unroll
    for (int k = 0; k < kCommitPerLane; ++k)
    {
        const int j = kCommitPerLane * tid + k;
        items[k] = CommitItem{};
        if (j < nMap)
        {
            items[k] = commit_map_plane(j, p.mapPlanes[j], p.mapRings, (uint64_t)(p.nMapRings < 0 ? 0 : p.nMapRings),
                                        (uint64_t)(p.nMapVertices < 0 ? 0 : p.nMapVertices), p.trackResults[j], nCur, p.fusion, p.unionRows, p.ringRows);
            commit_count(mine, items[k]);
            myRings += (int)items[k].rings;
            myVertices += (int)items[k].vertices; // (at most 1024 x 9 x 512: an int holds the map's)
        }
    }
    // ---- the appended planes: one per lane
    bool appends = false;
    long long mrow = -1;
    unsigned appendVertices = 0, appendOffset = 0;
    if ((p.flags & CAPE_COMMIT_ADD_STAGED) && tid < nCur)
    {
        mrow = measurement_row(p, tid);
        const cape_plane_measurement* m = mrow >= 0 ? p.measurements + mrow : nullptr;
        appends = commit_appends(p.fusion[tid], m, (uint64_t)(p.boundaryCapacity < 0 ? 0 : p.boundaryCapacity));
        if (appends)
        {
            appendVertices = m->vertex_count;
            appendOffset = m->vertex_offset;
        }
    }
    // ---- the scans: inside the wave, then across the waves
    const int ringsIncl = wave_scan_i32(myRings), verticesIncl = wave_scan_i32(myVertices);
    const int appendedIncl = wave_scan_i32(appends ? 1 : 0), appendVerticesIncl = wave_scan_i32((int)appendVertices);
    const unsigned refusal = wave_or_u32(mine.refusal);
    const int updated = wave_sum_i32(mine.updated), hostPairs = wave_sum_i32(mine.hostPairs), failPolygon = wave_sum_i32(mine.failPolygon);
    if (lane == 63)
    {
        int* s = sums + wave * kSumWords;
        s[kSumRings] = ringsIncl;
        s[kSumVertices] = verticesIncl;
        s[kSumRefusal] = (int)refusal;
        s[kSumUpdated] = updated;
        s[kSumHostPairs] = hostPairs;
        s[kSumFailPolygon] = failPolygon;
        s[kSumAppended] = appendedIncl;
        s[kSumAppendedVertices] = appendVerticesIncl;
    }
    __syncthreads();
    int before[kSumWords], total[kSumWords];
#pragma unroll
    for (int w = 0; w < kSumWords; ++w)
        before[w] = total[w] = 0;
#pragma unroll
    for (int v = 0; v < kCommitWaves; ++v)
#pragma unroll
        for (int w = 0; w < kSumWords; ++w)
        {
            const int s = sums[v * kSumWords + w];
            if (w == kSumRefusal)
                total[w] |= s;
            else
            {
                total[w] += s;
                before[w] += v < wave ? s : 0;
            }
        }
    // ---- the header, with the capacity check; the plan rows only if it says DONE (the copy kernel reads them only then)
    CommitTotals t{};
    t.refusal = (unsigned)total[kSumRefusal] | commit_frame_refusal(hd);
    t.planes = nMap + total[kSumAppended];
    t.rings = total[kSumRings] + total[kSumAppended];
    t.vertices = (long long)total[kSumVertices] + total[kSumAppendedVertices];
    t.updated = total[kSumUpdated];
    t.appended = total[kSumAppended];
    t.hostPairs = total[kSumHostPairs];
    t.failPolygon = total[kSumFailPolygon];
    const cape_map_commit_result result = commit_result(t, p.frame, p.nMap, p.nMapRings, p.nMapVertices, p.planesCapacity, p.ringsCapacity,
                                                        p.verticesCapacity, p.nextId);
    if (tid == 0)
        *p.header = result;
    if (!(result.flags & CAPE_COMMIT_DONE)) // (uniform: every lane holds the same totals)
        return;
    unsigned ring = (unsigned)(before[kSumRings] + ringsIncl - myRings), vertex = (unsigned)(before[kSumVertices] + verticesIncl - myVertices);
#pragma unroll
    for (int k = 0; k < kCommitPerLane; ++k)
    {
        const int j = kCommitPerLane * tid + k;
        if (j < nMap)
        {
            const CommitItem& it = items[k];
            CommitPlanRow row{};
            row.source = it.source;
            row.index = it.index;
            row.ringFirst = ring;
            row.ringCount = it.rings;
            row.vertexFirst = vertex;
            row.vertexCount = it.vertices;
            row.srcVertex = it.srcVertex; // (in p.slab, the frame's own)
            p.plan[j] = row;
            ring += it.rings;
            vertex += it.vertices;
        }
    }
    if (appends)
    {
        const unsigned nth = (unsigned)(before[kSumAppended] + appendedIncl - 1);
        CommitPlanRow row{};
        row.source = kCommitFromMeasure;
        row.index = (unsigned)tid;
        row.ringFirst = (unsigned)total[kSumRings] + nth;
        row.ringCount = 1u;
        row.vertexFirst = (unsigned)total[kSumVertices] + (unsigned)(before[kSumAppendedVertices] + appendVerticesIncl) - appendVertices;
        row.vertexCount = appendVertices;
        row.srcRow = (unsigned)mrow;
        row.srcVertex = (uint64_t)(mrow / CAPE_MAX_PLANES) * (uint64_t)p.boundaryCapacity + appendOffset;
        p.plan[nMap + nth] = row; // (nMap + appended <= CAPE_MAP_MAX_PLANES: DONE)
    }
}

__global__ __launch_bounds__(kCommitLanes) void cape_map_commit_copy_kernel(MapCommitParams p)
{
    const cape_map_commit_result hd = *p.header;
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (!(hd.flags & CAPE_COMMIT_DONE) || b >= hd.n_planes)
        return;
    const CommitPlanRow row = p.plan[b];
    const double2* src = nullptr;
    if (row.source == kCommitFromUnion)
        src = reinterpret_cast<const double2*>(p.slab) + row.srcVertex;
    else if (row.source == kCommitFromMeasure)
        src = reinterpret_cast<const double2*>(p.worldVertices) + row.srcVertex;
    double2* dst = reinterpret_cast<double2*>(p.outVertices) + row.vertexFirst;
    if (row.source == kCommitFromMap)
    {
        // ring by ring: each lies where its own record says
        const cape_map_plane& M = p.mapPlanes[row.index];
        unsigned at = 0;
        for (unsigned k = 0; k < row.ringCount; ++k)
        {
            const cape_map_ring r = p.mapRings[M.ring_first + k];
            const double2* from = reinterpret_cast<const double2*>(p.mapVertices) + r.vertex_offset;
            for (unsigned v = (unsigned)tid; v < r.vertex_count; v += kCommitLanes)
                dst[at + v] = from[v];
            if (tid == 0)
                p.outRings[row.ringFirst + k] = cape_map_ring {row.vertexFirst + at, r.vertex_count};
            at += r.vertex_count;
        }
    }
    else
    {
        for (unsigned v = (unsigned)tid; v < row.vertexCount; v += kCommitLanes)
            dst[v] = src[v];
    }
    if (tid != 0)
        return;
    cape_map_plane P{};
    MapTrackState T{};
    MapTrackTag G{};
    if (row.source == kCommitFromMeasure)
    {
        const cape_plane_measurement& m = p.measurements[row.srcRow];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            P.normal[k] = m.staged_normal[k], P.x_axis[k] = m.x_axis[k], P.y_axis[k] = m.y_axis[k], P.center[k] = m.center[k];
        P.d = m.d;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            T.covariance[k] = m.covariance[k];
        T.flags = CAPE_MAP_TRACK_STAGED;
        G.id = p.nextId + (unsigned long long)(b - p.nMap);
        G.result = CAPE_MAP_RESULT_APPENDED;
        p.outRings[row.ringFirst] = cape_map_ring {row.vertexFirst, row.vertexCount};
    }
    else
    {
        const int j = row.source == kCommitFromUnion ? p.unionRows[row.index].map_plane : (int)row.index;
        P = p.mapPlanes[j];
        T = p.tracks[j];
        if (row.source == kCommitFromUnion)
        {
            const cape_plane_fusion& F = p.fusion[row.index];
            const cape_plane_union& U = p.unionRows[row.index];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                P.normal[k] = F.normal[k], P.x_axis[k] = U.x_axis[k], P.y_axis[k] = U.y_axis[k], P.center[k] = U.center[k];
            P.d = F.d;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                T.covariance[k] = F.covariance[k];
            unsigned at = 0;
            for (unsigned k = 0; k < row.ringCount; ++k)
            {
                const unsigned n = p.ringRows ? p.ringRows[row.index].vertex_count[k] : U.vertex_count;
                p.outRings[row.ringFirst + k] = cape_map_ring {row.vertexFirst + at, n};
                at += n;
            }
        }
        const cape_map_track_result tr = p.trackResults[j];
        T.successiveMatched = tr.successive_matched;
        T.failedTracking = tr.failed_tracking;
        G.id = p.tags[j].id;
        G.result = tr.result;
    }
    P.ring_first = row.ringFirst;
    P.ring_count = row.ringCount;
    p.outPlanes[b] = P;
    p.outTracks[b] = T;
    p.outTags[b] = G;
}

hipError_t launch_map_commit(const MapCommitParams& p, int outPlanesBound, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_map_commit_plan_kernel, dim3(1), dim3(kCommitLanes), map_commit_layout().bytes, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(cape_map_commit_copy_kernel, dim3(outPlanesBound < 1 ? 1 : outPlanesBound), dim3(kCommitLanes), 0, stream, p);
    return hipGetLastError();
}

} // namespace cape

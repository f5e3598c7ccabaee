// cape_map_maintain: PROMOTE, DROP and LOST executed on the device map, with the retired log (host twin cape_host_map_maintain in
// host/polygon_capi.cpp; the rules are the plain functions of cape_map_maintain.h).  It reads the map and tracks as they stand and
// writes the BACK buffers of the map, the tracks and their ids -- the same set cape_map_commit writes -- and the tail of the retired
// log; the host swaps front and back once the header says DONE.
//
//   cape_map_maintain_plan_kernel : ONE workgroup of 256 lanes.  Lane t decides map planes 4 t .. 4 t + 3 (1024 at the most) with
//        maintain_plane; for a promote candidate it runs is_covariance_valid<4> (cape_map_tracking.h) on the track's covariance and the
//        unit check of the normal -- the only arithmetic of the call.  Three output sequences (local-out, staged-out, log) need
//        exclusive scans of planes, rings and vertices each: nine wave scans on the DPP path (cape_wave.h) and a step across the four
//        waves through LDS; the staged sequence starts at the local one's totals, the log sequence at what the log holds.  Lane 0
//        writes the result header (maintain_result) and, if it says DONE, every lane the plan rows of its planes.
//   cape_map_maintain_copy_kernel : one workgroup per INPUT plane, 256 lanes.  It leaves at once unless the header says DONE.  Lane 0
//        writes the plane record, the track, the id / result and the re-based ring records -- into the back set for a map
//        destination, as a whole cape_map_track into the log for a log destination; all lanes copy the vertices, a 16-byte load and
//        store per vertex.
//   cape_map_step_plan_kernel, cape_map_step_copy_kernel : the same two behind a commit on the same stream (cape_map_step).  They read
//        the commit's header in device memory: unless it says DONE they leave at once (the plan kernel writes the all-zero header);
//        else the map's sizes, the capacities and the log's bounds are derived from it (step_map_after, cape_map_step.h) where
//        cape_map_maintain's host side passes them as arguments, and the work is that of the two kernels above, one copy of it.
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_layout.h"
#include "cape_map_commit.h"
#include "cape_map_maintain.h"
#include "cape_map_step.h"
#include "cape_map_tracking.h"
#include "cape_wave.h"

namespace cape {

namespace {

constexpr int kMaintainLanes = 256, kMaintainWaves = kMaintainLanes / 64, kMaintainPerLane = 4;
static_assert(kMaintainLanes * kMaintainPerLane == CAPE_MAP_MAX_PLANES, "four map planes per lane");
static_assert(sizeof(double2) == 16 && sizeof(cape_map_ring) == 8, "16-byte vertex copies");

// per wave, the totals the other waves need: planes, rings and vertices of the three sequences, then the counts
enum
{
    kSumSeq = 0,                                // 3 x (planes, rings, vertices)
    kSumPromoted = 3 * (int)kMaintainSequences,
    kSumPromoteRefused,
    kSumDropped,
    kSumOutside,
    kSumWords
};
struct MapMaintainLayout
{
    size_t sums, bytes;
};
__host__ __device__ constexpr MapMaintainLayout map_maintain_layout()
{
    Layout l;
    MapMaintainLayout o{};
    o.sums = l.take<int>((size_t)kMaintainWaves * kSumWords, 16);
    o.bytes = l.end(16);
    return o;
}

// the plan kernel's work, for a map whose sizes the caller has put into p (cape_map_maintain: the host; cape_map_step: the kernel)
__device__ __forceinline__ void map_maintain_plan(const MapMaintainParams& p, unsigned char* smem)
{
    constexpr MapMaintainLayout lay = map_maintain_layout();
    int* sums = carve_at<int>(smem, lay.sums);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nMap = p.nMap < 0 ? 0 : (p.nMap > CAPE_MAP_MAX_PLANES ? CAPE_MAP_MAX_PLANES : p.nMap);

    // ---- the promote candidates' check, one plane after the other (one copy of the LDLT in the kernel, not four)
    unsigned promotable = 0;
#pragma unroll 1
    for (int k = 0; k < kMaintainPerLane; ++k)
    {
        const int j = kMaintainPerLane * tid + k;
        if (j < nMap && maintain_promote_candidate(p.tracks[j].flags, p.tracks[j].successiveMatched))
        {
            double C[16];
#pragma unroll
            for (int e = 0; e < 16; ++e)
                C[e] = p.tracks[j].covariance[e];
            const bool ok = is_covariance_valid<4>(C) && double_equal(norm3(p.mapPlanes[j].normal), 1.0);
            promotable |= (ok ? 1u : 0u) << k;
        }
    }
    // ---- the classes and sizes: four planes per lane, in order
    MaintainItem items[kMaintainPerLane];
    MaintainTotals mine{};
#pragma unroll
    for (int k = 0; k < kMaintainPerLane; ++k)
    {
        const int j = kMaintainPerLane * tid + k;
        items[k] = MaintainItem {kMaintainDropped, 0u, 0u, 0u}; // (beyond the map: no sequence, and not counted)
        if (j < nMap)
        {
            const MapTrackState& T = p.tracks[j];
            items[k] = maintain_plane(p.mapPlanes[j], p.mapRings, (uint64_t)(p.nMapRings < 0 ? 0 : p.nMapRings),
                                      (uint64_t)(p.nMapVertices < 0 ? 0 : p.nMapVertices), T.flags, T.successiveMatched, T.failedTracking,
                                      ((promotable >> k) & 1u) != 0);
            maintain_count(mine, items[k]);
        }
    }
    // ---- the scans: inside the wave, then across the waves
    int my[kSumWords], incl[kSumWords];
#pragma unroll
    for (int s = 0; s < (int)kMaintainSequences; ++s)
    {
        my[3 * s] = mine.seq[s].planes;
        my[3 * s + 1] = mine.seq[s].rings;
        my[3 * s + 2] = (int)mine.seq[s].vertices; // (at most 1024 x 9 x 512: an int holds the map's)
    }
    my[kSumPromoted] = mine.promoted;
    my[kSumPromoteRefused] = mine.promoteRefused;
    my[kSumDropped] = mine.dropped;
    my[kSumOutside] = mine.outside;
#pragma unroll
    for (int w = 0; w < kSumWords; ++w)
        incl[w] = w < kSumPromoted ? wave_scan_i32(my[w]) : wave_sum_i32(my[w]);
    if (lane == 63)
    {
#pragma unroll
        for (int w = 0; w < kSumWords; ++w)
            sums[wave * kSumWords + w] = incl[w];
    }
    __syncthreads();
    int before[kSumWords], total[kSumWords];
#pragma unroll
    for (int w = 0; w < kSumWords; ++w)
        before[w] = total[w] = 0;
#pragma unroll
    for (int v = 0; v < kMaintainWaves; ++v)
#pragma unroll
        for (int w = 0; w < kSumWords; ++w)
        {
            const int s = sums[v * kSumWords + w];
            total[w] += s;
            before[w] += v < wave ? s : 0;
        }
    // ---- the header; the plan rows only if it says DONE (the copy kernel reads them only then)
    MaintainTotals t{};
#pragma unroll
    for (int s = 0; s < (int)kMaintainSequences; ++s)
        t.seq[s] = MaintainCursor {total[3 * s], total[3 * s + 1], (int64_t)total[3 * s + 2]};
    t.promoted = total[kSumPromoted];
    t.promoteRefused = total[kSumPromoteRefused];
    t.dropped = total[kSumDropped];
    t.outside = total[kSumOutside];
    const cape_map_maintain_result result =
        maintain_result(t, p.nMap, p.nMapRings, p.nMapVertices, p.planesCapacity, p.ringsCapacity, p.verticesCapacity, p.log);
    if (tid == 0)
        *p.header = result;
    if (!(result.flags & CAPE_MAINTAIN_DONE)) // (uniform: every lane holds the same totals)
        return;
    // where this lane's first plane of each sequence goes: the sequence's start, the waves before, the lanes before
    const MaintainCursor start[kMaintainSequences] = {MaintainCursor {0, 0, 0}, t.seq[kMaintainSeqLocal], p.log.held};
    MaintainCursor at[kMaintainSequences];
#pragma unroll
    for (int s = 0; s < (int)kMaintainSequences; ++s)
    {
        at[s].planes = start[s].planes + before[3 * s] + incl[3 * s] - my[3 * s];
        at[s].rings = start[s].rings + before[3 * s + 1] + incl[3 * s + 1] - my[3 * s + 1];
        at[s].vertices = start[s].vertices + (int64_t)(before[3 * s + 2] + incl[3 * s + 2] - my[3 * s + 2]);
    }
#pragma unroll
    for (int k = 0; k < kMaintainPerLane; ++k)
    {
        const int j = kMaintainPerLane * tid + k;
        if (j < nMap)
        {
            const MaintainItem& it = items[k];
            const uint32_t seq = maintain_sequence(it.cls);
            MaintainPlanRow row = maintain_row(it, MaintainCursor {0, 0, 0});
#pragma unroll
            for (int s = 0; s < (int)kMaintainSequences; ++s) // (compare and select: no array indexed by the sequence)
                if (seq == (uint32_t)s)
                {
                    row = maintain_row(it, at[s]);
                    at[s].planes += 1;
                    at[s].rings += (int32_t)it.rings;
                    at[s].vertices += (int64_t)it.vertices;
                }
            p.plan[j] = row;
        }
    }
}

// the copy kernel's work, likewise
__device__ __forceinline__ void map_maintain_copy(const MapMaintainParams& p)
{
    const cape_map_maintain_result hd = *p.header;
    const int j = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (!(hd.flags & CAPE_MAINTAIN_DONE) || j >= p.nMap || j >= CAPE_MAP_MAX_PLANES)
        return;
    const MaintainPlanRow row = p.plan[j];
    if (row.dest == kMaintainToNone)
        return;
    const bool toLog = row.dest == kMaintainToLog;
    // (the plan checked the destination against its buffers -- a DONE header -- and the plane's rings against the map's)
    double2* dst = reinterpret_cast<double2*>(toLog ? p.logVertices : p.outVertices) + row.vertexFirst;
    cape_map_ring* dstRings = (toLog ? p.logRings : p.outRings) + row.ringFirst;
    const cape_map_plane M = p.mapPlanes[j];
    unsigned at = 0;
    for (unsigned k = 0; k < row.ringCount; ++k)
    {
        // ring by ring: each lies where its own record says
        const cape_map_ring r = p.mapRings[M.ring_first + k];
        const double2* from = reinterpret_cast<const double2*>(p.mapVertices) + r.vertex_offset;
        for (unsigned v = (unsigned)tid; v < r.vertex_count; v += kMaintainLanes)
            dst[at + v] = from[v];
        if (tid == 0)
            dstRings[k] = cape_map_ring {row.vertexFirst + at, r.vertex_count};
        at += r.vertex_count;
    }
    if (tid != 0)
        return;
    // (records are written in place and then amended: no copy of a whole record is held in registers)
    MapTrackState T = p.tracks[j];
    const MapTrackTag G = p.tags[j];
    if (row.edit == kMaintainEditPromote)
    {
        T.flags &= ~(uint32_t)CAPE_MAP_TRACK_STAGED;
        T.failedTracking = 0u;
    }
    cape_map_plane* P = (toLog ? p.logPlanes : p.outPlanes) + row.plane;
    *P = p.mapPlanes[j];
    P->ring_first = row.ringFirst;
    P->ring_count = row.ringCount;
    if (toLog)
    {
        cape_map_track* out = p.logTracks + row.plane;
#pragma unroll
        for (int e = 0; e < 16; ++e)
            out->covariance[e] = T.covariance[e];
        out->successive_matched = T.successiveMatched;
        out->failed_tracking = T.failedTracking;
        out->flags = T.flags;
        out->result = G.result;
        out->id = G.id;
    }
    else
    {
        p.outTracks[row.plane] = T;
        p.outTags[row.plane] = G;
    }
}

// cape_map_step: whether the maintenance runs, and on which map.  The state after the commit alone (step_map_after with the maintain
// header all zero) is the source: nothing to do unless that is the commit's BACK set, the set s.maintain's source pointers name.
// Its counts are the map's sizes, the capacities and the log's bounds what cape_map_maintain's host side derives from those sizes.
__device__ __forceinline__ bool map_step_source(MapMaintainParams& p, const cape_map_commit_result& commit)
{
    const StepMapState from = step_map_after(commit, cape_map_maintain_result{});
    if (from.set != kStepSetBack)
        return false;
    p.nMap = from.planes;
    p.nMapRings = from.rings;
    p.nMapVertices = from.vertices;
    p.planesCapacity = (unsigned long long)from.planes;
    p.ringsCapacity = (unsigned long long)from.rings;
    p.verticesCapacity = (unsigned long long)from.vertices;
    p.log = maintain_log_bounds(p.log.held, (uint64_t)from.planes, (uint64_t)from.rings, (uint64_t)from.vertices);
    return true;
}

} // namespace

__global__ __launch_bounds__(kMaintainLanes) void cape_map_maintain_plan_kernel(MapMaintainParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    map_maintain_plan(p, smem);
}

__global__ __launch_bounds__(kMaintainLanes) void cape_map_maintain_copy_kernel(MapMaintainParams p)
{
    map_maintain_copy(p);
}

// The step's plan kernel: ONE workgroup.  Behind a commit that is not DONE it writes the all-zero maintain header and leaves.
__global__ __launch_bounds__(kMaintainLanes) void cape_map_step_plan_kernel(MapStepParams s)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    MapMaintainParams p = s.maintain;
    if (!map_step_source(p, *s.commit)) // (uniform: one header)
    {
        if (threadIdx.x == 0)
            *p.header = cape_map_maintain_result{};
        return;
    }
    map_maintain_plan(p, smem);
}

// The step's copy kernel: launched to the bound the host knows of the committed map's planes; the workgroups beyond the committed
// count leave (map_maintain_copy: j >= nMap), all of them behind a commit that is not DONE.
__global__ __launch_bounds__(kMaintainLanes) void cape_map_step_copy_kernel(MapStepParams s)
{
    MapMaintainParams p = s.maintain;
    if (!map_step_source(p, *s.commit))
        return;
    map_maintain_copy(p);
}

hipError_t launch_map_step_maintain(const MapStepParams& s, int planesBound, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_map_step_plan_kernel, dim3(1), dim3(kMaintainLanes), map_maintain_layout().bytes, stream, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    const int planes = planesBound < 1 ? 1 : (planesBound > CAPE_MAP_MAX_PLANES ? CAPE_MAP_MAX_PLANES : planesBound);
    hipLaunchKernelGGL(cape_map_step_copy_kernel, dim3(planes), dim3(kMaintainLanes), 0, stream, s);
    return hipGetLastError();
}

hipError_t launch_map_maintain(const MapMaintainParams& p, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_map_maintain_plan_kernel, dim3(1), dim3(kMaintainLanes), map_maintain_layout().bytes, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    const int planes = p.nMap < 1 ? 1 : (p.nMap > CAPE_MAP_MAX_PLANES ? CAPE_MAP_MAX_PLANES : p.nMap);
    hipLaunchKernelGGL(cape_map_maintain_copy_kernel, dim3(planes), dim3(kMaintainLanes), 0, stream, p);
    return hipGetLastError();
}

} // namespace cape

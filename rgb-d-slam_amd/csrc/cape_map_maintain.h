// cape_map_maintain: the rules that execute PROMOTE, DROP and LOST on the ordered map list -- the list maintenance of
// Feature_Map::update_local_map / update_staged_map (feature_map.hpp:748-762, :805-830) with the constructor
// LocalMapPlane(const StagedMapPlane&) (map_primitive.cpp:286-318) -- and lay out the map and the retired log after it.  Pure data
// movement and integer decisions: no floating-point statement anywhere; the one arithmetic check of the call (is the staged plane's
// covariance valid and its normal a unit vector) is made by the caller and passed in as `promotable`.
//
// Plain per-plane functions, so that the plan kernel (cape_map_maintain.hip), the host twin cape_host_map_maintain
// (host/polygon_capi.cpp) and tests/host/map_maintain_plan.cpp compile the same decisions: with hipcc they are __host__ __device__,
// with any other compiler plain inline functions (no HIP header is needed then; one that is on the include path is taken).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CAPE_MAINTAIN_FN __host__ __device__ __forceinline__
#else
#if defined(__has_include)
#if __has_include(<hip/hip_runtime.h>)
#include <hip/hip_runtime.h>
#endif
#endif
#define CAPE_MAINTAIN_FN inline
#endif

#include "../../include/cape_hip.h"

namespace cape {

// what becomes of a map plane
enum : uint32_t
{
    kMaintainKeepLocal = 0,     // a local plane that is not lost
    kMaintainPromoted = 1,      // staged, successive_matched >= 4, promotable: local from now on
    kMaintainKeepStaged = 2,    // staged, neither promoted nor dropped
    kMaintainDropped = 3,       // staged, not a promote candidate, failed_tracking >= 2: removed, not logged
    kMaintainLost = 4,          // local, failed_tracking >= 10: removed and appended to the retired log
    kMaintainPromoteRefused = 5, // staged, successive_matched >= 4, not promotable: stays staged, is not dropped either
    kMaintainClasses = 6
};
// the three output sequences, each laid out back to back in list order: the survivors that are local after the call, the survivors
// that are staged after it (they start where the first sequence ends), and the retired log (it starts at what the log holds)
enum : uint32_t
{
    kMaintainSeqLocal = 0,
    kMaintainSeqStaged = 1,
    kMaintainSeqLog = 2,
    kMaintainSeqNone = 3,
    kMaintainSequences = 3
};
// a plan row's destination and what is changed in the track on the way
enum : uint32_t
{
    kMaintainToNone = 0,
    kMaintainToMap = 1,
    kMaintainToLog = 2
};
enum : uint32_t
{
    kMaintainEditNone = 0,
    kMaintainEditPromote = 1 // CAPE_MAP_TRACK_STAGED cleared, failed_tracking = 0 (a new LocalMapPlane's); everything else kept
};

constexpr int32_t kMaintainPromoteMatches = 4; // should_add_to_local_map
constexpr uint32_t kMaintainDropMisses = 2;    // should_remove_from_staged
constexpr uint32_t kMaintainLostMisses = 10;   // is_lost (planeUnmatchedCountToLoose)
constexpr uint32_t kMaintainMaxRings = 1u + CAPE_MAP_MAX_HOLES;

// a staged plane the reference would try to promote: only for these is `promotable` looked at
CAPE_MAINTAIN_FN bool maintain_promote_candidate(uint32_t flags, int32_t successiveMatched)
{
    return (flags & CAPE_MAP_TRACK_STAGED) && successiveMatched >= kMaintainPromoteMatches;
}

// The class of a plane from its track's flags and counters (not from `result`).  A refused promotion is not dropped: the
// reference's `else if` is not reached.
CAPE_MAINTAIN_FN uint32_t maintain_class(uint32_t flags, int32_t successiveMatched, uint32_t failedTracking, bool promotable)
{
    if (flags & CAPE_MAP_TRACK_STAGED)
    {
        if (successiveMatched >= kMaintainPromoteMatches)
            return promotable ? kMaintainPromoted : kMaintainPromoteRefused;
        return failedTracking >= kMaintainDropMisses ? kMaintainDropped : kMaintainKeepStaged;
    }
    return failedTracking >= kMaintainLostMisses ? kMaintainLost : kMaintainKeepLocal;
}

CAPE_MAINTAIN_FN uint32_t maintain_sequence(uint32_t cls)
{
    return cls == kMaintainKeepLocal || cls == kMaintainPromoted          ? kMaintainSeqLocal
           : cls == kMaintainKeepStaged || cls == kMaintainPromoteRefused ? kMaintainSeqStaged
           : cls == kMaintainLost                                         ? kMaintainSeqLog
                                                                          : kMaintainSeqNone;
}

// What one map plane takes: its class, its sizes, and whether its rings do not lie in the map's buffers (the call is refused then).
struct MaintainItem
{
    uint32_t cls;
    uint32_t rings, vertices;
    uint32_t outside; // 1: CAPE_MAINTAIN_CAPACITY
};

// Map plane M with the track's flags and counters; the map's rings with what the ring and vertex buffers hold.  Every count read
// from the map is checked against its buffer before it is used.
CAPE_MAINTAIN_FN MaintainItem maintain_plane(const cape_map_plane& M, const cape_map_ring* mapRings, uint64_t nMapRings, uint64_t nMapVertices,
                                             uint32_t flags, int32_t successiveMatched, uint32_t failedTracking, bool promotable)
{
    MaintainItem it{};
    it.cls = maintain_class(flags, successiveMatched, failedTracking, promotable);
    if (M.ring_count < 1u || M.ring_count > kMaintainMaxRings || (uint64_t)M.ring_first + M.ring_count > nMapRings)
    {
        it.outside = 1u;
        return it;
    }
    uint32_t vertices = 0;
    for (uint32_t k = 0; k < M.ring_count; ++k)
    {
        const cape_map_ring r = mapRings[M.ring_first + k];
        if (r.vertex_count > (uint32_t)CAPE_MAP_MAX_RING || (uint64_t)r.vertex_offset + r.vertex_count > nMapVertices)
        {
            it.outside = 1u;
            return it;
        }
        vertices += r.vertex_count;
    }
    it.rings = M.ring_count;
    it.vertices = vertices;
    return it;
}

// A plan row: what the copy kernel needs to move input plane j without looking at its neighbours.
struct MaintainPlanRow
{
    uint32_t dest;                     // kMaintainTo*
    uint32_t plane;                    // the destination plane: in the new map, or in the log's own arrays
    uint32_t ringFirst, ringCount;     // in the destination's ring array
    uint32_t vertexFirst, vertexCount; // in the destination's vertex array, all rings
    uint32_t edit;                     // kMaintainEdit*
    uint32_t cls;                      // kMaintain*: the class that was decided
};

// where a sequence stands: planes, rings and vertices written so far
struct MaintainCursor
{
    int32_t planes, rings;
    int64_t vertices;
};

CAPE_MAINTAIN_FN MaintainPlanRow maintain_row(const MaintainItem& it, const MaintainCursor& at)
{
    const uint32_t seq = maintain_sequence(it.cls);
    MaintainPlanRow row{};
    row.cls = it.cls;
    if (seq == kMaintainSeqNone)
        return row;
    row.dest = seq == kMaintainSeqLog ? kMaintainToLog : kMaintainToMap;
    row.plane = (uint32_t)at.planes;
    row.ringFirst = (uint32_t)at.rings;
    row.ringCount = it.rings;
    row.vertexFirst = (uint32_t)at.vertices;
    row.vertexCount = it.vertices;
    row.edit = it.cls == kMaintainPromoted ? kMaintainEditPromote : kMaintainEditNone;
    return row;
}

// what the plan counted over all planes
struct MaintainTotals
{
    MaintainCursor seq[kMaintainSequences]; // the sizes of each sequence (the log's: of this call's lost planes)
    int32_t promoted, promoteRefused, dropped, outside;
};

CAPE_MAINTAIN_FN void maintain_count(MaintainTotals& t, const MaintainItem& it)
{
    const uint32_t seq = maintain_sequence(it.cls);
    for (uint32_t s = 0; s < kMaintainSequences; ++s) // (compare and add: no array indexed by the sequence, so none in scratch memory)
    {
        const bool here = seq == s;
        t.seq[s].planes += here ? 1 : 0;
        t.seq[s].rings += here ? (int32_t)it.rings : 0;
        t.seq[s].vertices += here ? (int64_t)it.vertices : 0;
    }
    t.promoted += it.cls == kMaintainPromoted;
    t.promoteRefused += it.cls == kMaintainPromoteRefused;
    t.dropped += it.cls == kMaintainDropped;
    t.outside += (int32_t)it.outside;
}

// the retired log as the call finds it, and what its arrays may take
struct MaintainLog
{
    MaintainCursor held;
    uint64_t planesCapacity, ringsCapacity, verticesCapacity;
};

// What the log may take in a maintenance of a map of these sizes: the whole map on top of what it holds, CAPE_MAP_RETIRED_MAX_PLANES
// planes at the most.  The host grows the log's arrays to at least this before the launch.
CAPE_MAINTAIN_FN MaintainLog maintain_log_bounds(const MaintainCursor& held, uint64_t planes, uint64_t rings, uint64_t vertices)
{
    const uint64_t all = (uint64_t)held.planes + planes;
    MaintainLog log{};
    log.held = held;
    log.planesCapacity = all < (uint64_t)CAPE_MAP_RETIRED_MAX_PLANES ? all : (uint64_t)CAPE_MAP_RETIRED_MAX_PLANES;
    log.ringsCapacity = (uint64_t)held.rings + rings;
    log.verticesCapacity = (uint64_t)held.vertices + vertices;
    return log;
}

// The result header.  Refused (nothing changes, log included): CAPE_MAINTAIN_CAPACITY for a plane whose rings do not lie in the
// map's buffers or a new map beyond the buffers it is written to; CAPE_MAINTAIN_LOG_FULL where the lost planes do not fit
// CAPE_MAP_RETIRED_MAX_PLANES, the log's arrays or a uint32 offset.  Otherwise NOTHING if no plane is promoted, dropped or lost, else
// DONE.  The sizes are the new map's and log's if DONE, the old ones' otherwise; the class counts are what the plan counted either way.
CAPE_MAINTAIN_FN cape_map_maintain_result maintain_result(const MaintainTotals& t, int32_t oldPlanes, int32_t oldRings, int64_t oldVertices,
                                                          uint64_t planesCapacity, uint64_t ringsCapacity, uint64_t verticesCapacity,
                                                          const MaintainLog& log)
{
    const MaintainCursor &L = t.seq[kMaintainSeqLocal], &S = t.seq[kMaintainSeqStaged], &X = t.seq[kMaintainSeqLog];
    const int32_t planes = L.planes + S.planes, rings = L.rings + S.rings;
    const int64_t vertices = L.vertices + S.vertices;
    uint32_t refusal = 0;
    if (t.outside > 0 || (uint64_t)planes > planesCapacity || (uint64_t)rings > ringsCapacity || (uint64_t)vertices > verticesCapacity)
        refusal |= CAPE_MAINTAIN_CAPACITY;
    const int64_t logPlanes = (int64_t)log.held.planes + X.planes, logRings = (int64_t)log.held.rings + X.rings,
                  logVertices = log.held.vertices + X.vertices;
    if (X.planes > 0 && (logPlanes > (int64_t)CAPE_MAP_RETIRED_MAX_PLANES || (uint64_t)logPlanes > log.planesCapacity ||
                         (uint64_t)logRings > log.ringsCapacity || (uint64_t)logVertices > log.verticesCapacity || logRings > (int64_t)0x7FFFFFFFll ||
                         logVertices > (int64_t)0xFFFFFFFFll))
        refusal |= CAPE_MAINTAIN_LOG_FULL;
    const bool due = t.promoted + t.dropped + X.planes > 0;
    const bool done = refusal == 0 && due;
    cape_map_maintain_result r{};
    r.flags = refusal ? refusal : (due ? (uint32_t)CAPE_MAINTAIN_DONE : (uint32_t)CAPE_MAINTAIN_NOTHING);
    r.n_planes = done ? planes : oldPlanes;
    r.n_rings = done ? rings : oldRings;
    r.n_vertices = done ? vertices : oldVertices;
    r.n_local = L.planes;
    r.n_staged = S.planes;
    r.n_promoted = t.promoted;
    r.n_promote_refused = t.promoteRefused;
    r.n_dropped = t.dropped;
    r.n_lost = X.planes;
    r.n_retired = done ? (int32_t)logPlanes : log.held.planes;
    r.n_retired_rings = done ? (int32_t)logRings : log.held.rings;
    r.n_retired_vertices = done ? logVertices : log.held.vertices;
    return r;
}

// The whole plan, one plane after the other: what the plan kernel computes with its scans.  tracks: parallel to the planes;
// promotable[j]: read for a promote candidate only (maintain_promote_candidate).  rows: one per map plane, written whatever the
// result says (the rows of a call that is not DONE are not used).
inline cape_map_maintain_result maintain_plan_serial(const cape_map_plane* mapPlanes, int32_t nMap, const cape_map_ring* mapRings, int32_t nMapRings,
                                                     int64_t nMapVertices, const cape_map_track* tracks, const uint8_t* promotable,
                                                     uint64_t planesCapacity, uint64_t ringsCapacity, uint64_t verticesCapacity,
                                                     const MaintainLog& log, MaintainPlanRow* rows)
{
    MaintainTotals t{};
    const auto item = [&](int32_t j) {
        const cape_map_track& T = tracks[j];
        const bool ok = maintain_promote_candidate(T.flags, T.successive_matched) && promotable[j] != 0;
        return maintain_plane(mapPlanes[j], mapRings, (uint64_t)(nMapRings < 0 ? 0 : nMapRings), (uint64_t)(nMapVertices < 0 ? 0 : nMapVertices), T.flags,
                              T.successive_matched, T.failed_tracking, ok);
    };
    for (int32_t j = 0; j < nMap; ++j)
        maintain_count(t, item(j));
    MaintainCursor at[kMaintainSequences] = {MaintainCursor {0, 0, 0}, t.seq[kMaintainSeqLocal], log.held};
    for (int32_t j = 0; j < nMap; ++j)
    {
        const MaintainItem it = item(j);
        const uint32_t seq = maintain_sequence(it.cls);
        if (seq == kMaintainSeqNone)
        {
            rows[j] = maintain_row(it, MaintainCursor {0, 0, 0});
            continue;
        }
        rows[j] = maintain_row(it, at[seq]);
        at[seq].planes += 1;
        at[seq].rings += (int32_t)it.rings;
        at[seq].vertices += (int64_t)it.vertices;
    }
    return maintain_result(t, nMap, nMapRings, nMapVertices, planesCapacity, ringsCapacity, verticesCapacity, log);
}

#if defined(__HIPCC__)
// cape_map_maintain's two kernels (cape_map_maintain.hip)
struct MapMaintainParams
{
    // the map, its tracks and their ids: the front buffers and what they hold
    const cape_map_plane* mapPlanes;
    const cape_map_ring* mapRings;
    const double* mapVertices; // (x, y) pairs
    const struct MapTrackState* tracks;
    const struct MapTrackTag* tags;
    int nMap, nMapRings;
    long long nMapVertices; // (what the map holds: no ring or vertex index of a map plane may reach beyond)
    // the back buffers and what they take
    cape_map_plane* outPlanes;
    cape_map_ring* outRings;
    double* outVertices;
    struct MapTrackState* outTracks;
    struct MapTrackTag* outTags;
    unsigned long long planesCapacity, ringsCapacity, verticesCapacity;
    // the retired log: its arrays, what they hold and what they take
    cape_map_plane* logPlanes;
    cape_map_ring* logRings;
    double* logVertices;
    cape_map_track* logTracks;
    MaintainLog log;
    // the plan
    MaintainPlanRow* plan;            // CAPE_MAP_MAX_PLANES rows
    cape_map_maintain_result* header; // device memory
};
#endif

} // namespace cape

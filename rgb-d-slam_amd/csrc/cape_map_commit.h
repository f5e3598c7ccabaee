// cape_map_commit: the rules that turn a frame's device results (cape_map_kalman's track results and fusion rows, cape_map_measure's
// rows, the rows / rings table / slab of cape_map_union[_holes|_cut]) and the uploaded map into the map after the frame -- the
// map_out of cape_host_map_update.  Pure data movement: no floating-point statement anywhere.
//
// Plain per-plane functions, so that the plan kernel (cape_map_commit.hip), the host twin cape_host_map_commit
// (host/polygon_capi.cpp) and tests/host/map_commit_plan.cpp compile the same decisions: with hipcc they are __host__ __device__,
// with any other compiler plain inline functions (no HIP header is needed then; one that is on the include path is taken).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CAPE_COMMIT_FN __host__ __device__ __forceinline__
#else
#if defined(__has_include)
#if __has_include(<hip/hip_runtime.h>)
#include <hip/hip_runtime.h>
#endif
#endif
#define CAPE_COMMIT_FN inline
#endif

#include "../../include/cape_hip.h"

namespace cape {

// id and result of a track (cape_map_track's last two members), which MapTrackState does not hold: an array of its own beside
// Handle::Kalman::tracks, written by cape_map_upload_tracks and by the commit
struct MapTrackTag
{
    uint64_t id;
    uint32_t result, pad;
};

// where an output plane comes from
enum : uint32_t
{
    kCommitFromMap = 0,    // the old map: plane, frame, rings and covariance are its own
    kCommitFromUnion = 1,  // a served union row: state of the fusion row, frame and rings of the union
    kCommitFromMeasure = 2 // an appended staged plane: a stageable measurement row and its world ring
};

constexpr uint32_t kCommitMaxRings = 1u + CAPE_MAP_MAX_HOLES;
constexpr uint32_t kCommitMaxAppended = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
constexpr uint32_t kUnionHostBits =
    CAPE_UNION_HOST_MAP_HOLES | CAPE_UNION_HOST_NEW_HOLE | CAPE_UNION_HOST_CAPACITY | CAPE_UNION_HOST_AMBIGUOUS | CAPE_UNION_HOST_HOLE_CUT;

// What one output plane takes: its source, what it refuses the frame for (CAPE_COMMIT_* bits, 0: nothing) and its sizes.
struct CommitItem
{
    uint32_t source;   // kCommitFrom*
    uint32_t index;    // map plane j (kCommitFromMap) or kept plane i
    uint32_t refusal;  // CAPE_COMMIT_HOST_PAIR, CAPE_COMMIT_FAIL_POLYGON or CAPE_COMMIT_CAPACITY (a map plane whose rings do not lie in the map)
    uint32_t rings, vertices;
    uint32_t srcVertex; // kCommitFromUnion: the first vertex in the frame's slab
};

// A plan row: what the copy kernel needs to write output plane b without looking at its neighbours.
struct CommitPlanRow
{
    uint32_t source, index;
    uint32_t ringFirst, ringCount;     // in the new map
    uint32_t vertexFirst, vertexCount; // in the new map, all rings
    uint32_t srcRow, pad;              // kCommitFromMeasure: the measurement row, record x CAPE_MAX_PLANES + segment
    uint64_t srcVertex;                // first source vertex: kCommitFromUnion in the union slabs, kCommitFromMeasure in the world-vertex slabs
};

// The rings of a served union row: their number and total length, or false if the row, the rings table (null: a plain cape_map_union,
// one ring) or the slab's capacity do not agree -- such a pair is the host's.
CAPE_COMMIT_FN bool commit_union_rings(const cape_plane_union& U, const cape_plane_union_rings* R, uint32_t& rings, uint32_t& vertices)
{
    rings = R ? R->ring_count : 1u;
    if (rings < 1u || rings > kCommitMaxRings)
        return false;
    uint64_t total = 0;
    for (uint32_t k = 0; k < rings; ++k)
    {
        const uint32_t n = R ? R->vertex_count[k] : U.vertex_count;
        if (n < 3u || n > (uint32_t)CAPE_MAP_MAX_RING)
            return false;
        total += n;
    }
    if ((R && R->vertex_count[0] != U.vertex_count) || U.vertex_offset > (uint32_t)CAPE_MAP_UNION_FRAME_VERTICES ||
        total > (uint64_t)CAPE_MAP_UNION_FRAME_VERTICES - U.vertex_offset)
        return false;
    vertices = (uint32_t)total;
    return true;
}

// Map plane j.  tr: its track result of the frame; fusion, unionRows, ringRows (null: plain union): the frame's rows, nCur of them
// meaningful; the map's rings with what the ring and vertex buffers hold.
CAPE_COMMIT_FN CommitItem commit_map_plane(int32_t j, const cape_map_plane& M, const cape_map_ring* mapRings, uint64_t nMapRings, uint64_t nMapVertices,
                                           const cape_map_track_result& tr, int32_t nCur, const cape_plane_fusion* fusion, const cape_plane_union* unionRows,
                                           const cape_plane_union_rings* ringRows)
{
    CommitItem it{};
    it.source = kCommitFromMap;
    it.index = (uint32_t)j;
    const int32_t i = tr.kept_plane;
    if (i >= 0 && i < nCur && fusion[i].map_plane == j && (fusion[i].flags & CAPE_FUSION_STATE))
    {
        const cape_plane_union& U = unionRows[i];
        if (U.map_plane != j)
            it.refusal = CAPE_COMMIT_FAIL_POLYGON; // no union pair: the host's polygon is the projected or the old one
        else if (!(U.flags & CAPE_UNION_SERVED))
            it.refusal = (U.flags & kUnionHostBits) ? (uint32_t)CAPE_COMMIT_HOST_PAIR : (uint32_t)CAPE_COMMIT_FAIL_POLYGON;
        else if (!commit_union_rings(U, ringRows ? ringRows + i : nullptr, it.rings, it.vertices))
            it.refusal = CAPE_COMMIT_HOST_PAIR;
        else
        {
            it.source = kCommitFromUnion;
            it.index = (uint32_t)i;
            it.srcVertex = U.vertex_offset;
            return it;
        }
    }
    // the old map's polygon (also counted for a refused pair: the sizes of a refused frame are not used)
    it.rings = it.vertices = 0;
    if (M.ring_count < 1u || M.ring_count > kCommitMaxRings || (uint64_t)M.ring_first + M.ring_count > nMapRings)
    {
        it.refusal |= CAPE_COMMIT_CAPACITY;
        return it;
    }
    it.rings = M.ring_count;
    for (uint32_t k = 0; k < M.ring_count; ++k)
    {
        const cape_map_ring r = mapRings[M.ring_first + k];
        if (r.vertex_count > (uint32_t)CAPE_MAP_MAX_RING || (uint64_t)r.vertex_offset + r.vertex_count > nMapVertices)
        {
            it.refusal |= CAPE_COMMIT_CAPACITY;
            return it;
        }
        it.vertices += r.vertex_count;
    }
    return it;
}

// Kept plane i is appended as a staged plane: no map plane used it and its measurement row (null: the kept-plane table points outside
// the row buffer) is stageable, its world ring inside the slab of slabCapacity vertices it lies in.
CAPE_COMMIT_FN bool commit_appends(const cape_plane_fusion& F, const cape_plane_measurement* m, uint64_t slabCapacity)
{
    return !(F.flags & CAPE_FUSION_USED) && m && (m->flags & CAPE_MEASURE_STAGEABLE) && m->vertex_count >= 3u &&
           m->vertex_count <= (uint32_t)CAPE_MAP_MAX_RING && (uint64_t)m->vertex_offset + m->vertex_count <= slabCapacity;
}

// kept planes of a frame the commit looks at, and what the frame's header alone refuses
CAPE_COMMIT_FN int32_t commit_kept_planes(const cape_frame_map_kalman& hd)
{
    if (hd.flags & CAPE_MATCH_EXACT_OVERFLOW)
        return 0;
    return hd.n_cur < 0 ? 0 : (hd.n_cur > (int32_t)CAPE_MATCH_MAP_WIDE_MAX_PLANES ? (int32_t)CAPE_MATCH_MAP_WIDE_MAX_PLANES : hd.n_cur);
}
CAPE_COMMIT_FN uint32_t commit_frame_refusal(const cape_frame_map_kalman& hd)
{
    return ((hd.flags & CAPE_MATCH_EXACT_OVERFLOW) ? (uint32_t)CAPE_COMMIT_FRAME_OVERFLOW : 0u) |
           ((hd.flags & CAPE_KALMAN_BAD_POSE_COV) ? (uint32_t)CAPE_COMMIT_BAD_POSE_COV : 0u);
}

// what the plan counted over all output planes
struct CommitTotals
{
    uint32_t refusal;                               // CAPE_COMMIT_* bits of the frame and of every plane, OR-ed
    int32_t planes, rings;                          // of the new map
    int64_t vertices;
    int32_t updated, appended, hostPairs, failPolygon;
};

// The result header: the capacity check (the new map within CAPE_MAP_MAX_PLANES, a uint32 offset and the buffers it is written to),
// DONE or the refusal bits, and the sizes -- the new map's if DONE, the old one's otherwise.
CAPE_COMMIT_FN cape_map_commit_result commit_result(CommitTotals t, int32_t frame, int32_t oldPlanes, int32_t oldRings, int64_t oldVertices,
                                                    uint64_t planesCapacity, uint64_t ringsCapacity, uint64_t verticesCapacity, uint64_t nextId)
{
    if (t.planes > (int32_t)CAPE_MAP_MAX_PLANES || t.vertices > (int64_t)0xFFFFFFFFll || (uint64_t)t.planes > planesCapacity ||
        (uint64_t)t.rings > ringsCapacity || (uint64_t)t.vertices > verticesCapacity)
        t.refusal |= CAPE_COMMIT_CAPACITY;
    const bool done = t.refusal == 0;
    cape_map_commit_result r{};
    r.flags = done ? (uint32_t)CAPE_COMMIT_DONE : t.refusal;
    r.frame = frame;
    r.n_planes = done ? t.planes : oldPlanes;
    r.n_rings = done ? t.rings : oldRings;
    r.n_vertices = done ? t.vertices : oldVertices;
    r.n_updated = t.updated;
    r.n_appended = t.appended;
    r.n_host_pairs = t.hostPairs;
    r.n_fail_polygon = t.failPolygon;
    r.next_id = nextId + (done ? (uint64_t)t.appended : 0u);
    return r;
}

CAPE_COMMIT_FN void commit_count(CommitTotals& t, const CommitItem& it)
{
    t.refusal |= it.refusal;
    t.updated += it.source == kCommitFromUnion;
    t.hostPairs += (it.refusal & CAPE_COMMIT_HOST_PAIR) != 0;
    t.failPolygon += (it.refusal & CAPE_COMMIT_FAIL_POLYGON) != 0;
}

// The whole plan, one plane after the other: what the plan kernel computes with its scans.  measurements: the frame's rows in
// KEPT-PLANE order, their world rings back to back (the layout the host twins take; srcVertex of an appended plane counts in it,
// srcRow is the kept plane).  rows: room for planes of the old map + kCommitMaxAppended.  The capacities: what the new map may take.
inline cape_map_commit_result commit_plan_serial(const cape_map_plane* mapPlanes, int32_t nMap, const cape_map_ring* mapRings, int32_t nMapRings,
                                                 int64_t nMapVertices, int32_t frame, const cape_frame_map_kalman& hd,
                                                 const cape_map_track_result* trackResults, const cape_plane_fusion* fusion,
                                                 const cape_plane_measurement* measurements, const cape_plane_union* unionRows,
                                                 const cape_plane_union_rings* ringRows, uint32_t flags, uint64_t nextId, uint64_t planesCapacity,
                                                 uint64_t ringsCapacity, uint64_t verticesCapacity, CommitPlanRow* rows)
{
    const int32_t nCur = commit_kept_planes(hd);
    CommitTotals t{};
    t.refusal = commit_frame_refusal(hd);
    uint32_t ring = 0;
    uint64_t vertex = 0;
    int32_t b = 0;
    for (int32_t j = 0; j < nMap; ++j, ++b)
    {
        const CommitItem it = commit_map_plane(j, mapPlanes[j], mapRings, (uint64_t)nMapRings, (uint64_t)nMapVertices, trackResults[j], nCur, fusion,
                                               unionRows, ringRows);
        commit_count(t, it);
        rows[b] = CommitPlanRow {it.source, it.index, ring, it.rings, (uint32_t)vertex, it.vertices, 0u, 0u, it.srcVertex};
        ring += it.rings;
        vertex += it.vertices;
    }
    uint64_t world = 0;
    for (int32_t i = 0; i < nCur; ++i)
    {
        const cape_plane_measurement& m = measurements[i];
        if ((flags & CAPE_COMMIT_ADD_STAGED) && commit_appends(fusion[i], &m, (uint64_t)m.vertex_offset + m.vertex_count))
        {
            rows[b++] = CommitPlanRow {kCommitFromMeasure, (uint32_t)i, ring, 1u, (uint32_t)vertex, m.vertex_count, (uint32_t)i, 0u, world};
            ring += 1;
            vertex += m.vertex_count;
            ++t.appended;
        }
        world += m.vertex_count;
    }
    t.planes = b;
    t.rings = (int32_t)ring;
    t.vertices = (int64_t)vertex;
    return commit_result(t, frame, nMap, nMapRings, nMapVertices, planesCapacity, ringsCapacity, verticesCapacity, nextId);
}

#if defined(__HIPCC__)
// cape_map_commit's two kernels (cape_map_commit.hip)
struct MapCommitParams
{
    // the map, its tracks and their ids: the front buffers and what they hold
    const cape_map_plane* mapPlanes;
    const cape_map_ring* mapRings;
    const double* mapVertices; // (x, y) pairs
    const struct MapTrackState* tracks;
    const MapTrackTag* tags;
    int nMap, nMapRings;
    long long nMapVertices; // (what the map holds: no ring or vertex index of a map plane may reach beyond)
    // the frame's results
    int frame;
    const cape_frame_map_kalman* kalmanFrame;    // the frame's header
    const cape_map_track_result* trackResults;   // the frame's nMap
    const cape_plane_fusion* fusion;             // the frame's 128
    const uint2* kept;                           // the frame's 128: (record, segment in that record) of kept plane i
    const cape_plane_measurement* measurements;  // nRecords x CAPE_MAX_PLANES
    const double* worldVertices;                 // nRecords slabs of boundaryCapacity (x, y) pairs
    int nRecords, boundaryCapacity;
    const cape_plane_union* unionRows;           // the frame's 128
    const cape_plane_union_rings* ringRows;      // the frame's 128, or null: a plain cape_map_union
    const double* slab;                          // the frame's CAPE_MAP_UNION_FRAME_VERTICES (x, y) pairs
    uint32_t flags;
    unsigned long long nextId;
    // the back buffers and what they take
    cape_map_plane* outPlanes;
    cape_map_ring* outRings;
    double* outVertices;
    struct MapTrackState* outTracks;
    MapTrackTag* outTags;
    unsigned long long planesCapacity, ringsCapacity, verticesCapacity;
    // the plan
    CommitPlanRow* plan;            // CAPE_MAP_MAX_PLANES rows
    cape_map_commit_result* header; // device memory
};
#endif

} // namespace cape

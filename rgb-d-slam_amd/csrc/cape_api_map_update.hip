// C ABI, host side: what changes the device map -- the measurements, the Kalman step and the polygon unions of the map update, the
// commit, the maintenance with its retired log, and the step that runs one frame through all of them with one wait.
#include <algorithm>
#include <cstring>

#include "cape_api_map.h"

using namespace cape::abi;

namespace {

// the results of the last cape_map_kalman still describe the current batch, match and measurements (a cape_extract clears the latter
// two; every other call that replaces an input says so through invalidate_frame_results)
bool kalman_results_live(const cape_handle_s* h)
{
    const auto& K = h->kalman;
    return K.kalmanFrames > 0 && h->mapWide.matchFrames >= K.kalmanFrames && h->measure.frames >= K.kalmanFrames;
}

// ... and those of the last cape_map_union the Kalman results they were made from
bool union_results_live(const cape_handle_s* h)
{
    const auto& U = h->mapUnion;
    return U.unionFrames > 0 && kalman_results_live(h) && h->kalman.kalmanFrames >= U.unionFrames && U.kalmanRun == h->kalman.runs;
}

// The kernel parameters of the map update's calls, bound to the handle's buffers: cape_map_kalman, cape_map_union* and cape_map_commit
// run them on the first n frames of the batch-wide tables, cape_map_step on the one frame whose rows it has put at row 0 of them.
cape::MapKalmanParams bind_map_kalman(const cape_handle_s* h)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    const auto& K = h->kalman;
    const auto& W = h->mapWide;
    cape::MapKalmanParams p{};
    p.mapPlanes = h->maps.front.planes;
    p.tracks = h->maps.front.tracks;
    p.nMap = h->maps.n;
    p.matchFrames = W.frames;
    p.match = W.match;
    p.mapOf = W.planes + (size_t)h->cfg.max_batch * WP;
    p.kept = W.kept;
    p.measurements = h->measure.rows;
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords; // (the rows cape_map_measure allocated: a row of CAPE_MAX_PLANES per record)
    p.frames = K.frames;
    p.rows = K.rows;
    p.trackResults = K.trackResults;
    return p;
}
cape::MapUnionParams bind_map_union(const cape_handle_s* h)
{
    const auto& W = h->mapWide;
    const auto& M = h->measure;
    cape::MapUnionParams p{};
    p.mapPlanes = h->maps.front.planes;
    p.mapRings = h->maps.front.rings;
    p.mapVertices = reinterpret_cast<const double2*>(h->maps.front.vertices.get());
    p.nMap = h->maps.n;
    p.nMapRings = (unsigned)h->maps.front.rings.size();
    p.nMapVertices = (unsigned long long)(h->maps.front.vertices.size() / 2);
    p.matchFrames = W.frames;
    p.match = W.match;
    p.kept = W.kept;
    p.measurements = M.rows;
    p.worldVertices = reinterpret_cast<const double2*>(M.vertices.get());
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords; // (the rows and slabs cape_map_measure allocated: one per record)
    p.boundaryCapacity = h->boundaryCap;
    p.fusion = h->kalman.rows;
    p.rows = h->mapUnion.rows;
    p.vertices = reinterpret_cast<double2*>(h->mapUnion.vertices.get());
    return p;
}
// what a commit's destination set takes, to bounds the host knows: at most 128 appended planes of one ring each, a frame's slab of
// served rings, the world rings of the frame's chain
struct CommitBounds
{
    size_t planes, rings, vertices;
};
CommitBounds commit_bounds(const cape_handle_s* h)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    const size_t n = (size_t)h->maps.n, cap = (size_t)h->boundaryCap;
    CommitBounds b;
    b.planes = std::min<size_t>(CAPE_MAP_MAX_PLANES, n + WP);
    b.rings = b.planes * (1 + CAPE_MAP_MAX_HOLES);
    b.vertices = (size_t)h->maps.nVertices + SLAB + std::min<size_t>(WP * CAPE_MAP_MAX_RING, (size_t)(1 + h->chain.spillRecords) * cap);
    return b;
}
// workgroups of the commit's copy kernel: the planes of the new map at most
int commit_planes_bound(const cape_handle_s* h, const CommitBounds& b, uint32_t flags)
{
    return (int)std::min<size_t>(b.planes, (size_t)h->maps.n + ((flags & CAPE_COMMIT_ADD_STAGED) ? (size_t)CAPE_MATCH_MAP_WIDE_MAX_PLANES : 0));
}
// frame `frame` of the batch, whose rows are row `row` of the per-frame tables; withRings: the union's rings table belongs to its rows
cape::MapCommitParams bind_map_commit(const cape_handle_s* h, size_t row, int32_t frame, bool withRings, uint32_t flags, uint64_t nextId,
                                      const CommitBounds& b, cape_map_commit_result* header)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    const auto& M = h->maps;
    const auto& K = h->kalman;
    const auto& U = h->mapUnion;
    cape::MapCommitParams p{};
    p.mapPlanes = M.front.planes;
    p.mapRings = M.front.rings;
    p.mapVertices = M.front.vertices;
    p.tracks = M.front.tracks;
    p.tags = M.front.tags;
    p.nMap = M.n;
    p.nMapRings = M.nRings;
    p.nMapVertices = M.nVertices;
    p.frame = frame;
    p.kalmanFrame = K.frames + row;
    p.trackResults = K.trackResults + row * (size_t)M.n;
    p.fusion = K.rows + row * WP;
    p.kept = h->mapWide.kept + row * WP;
    p.measurements = h->measure.rows;
    p.worldVertices = h->measure.vertices;
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords; // (the rows and slabs cape_map_measure allocated: one per record)
    p.boundaryCapacity = h->boundaryCap;
    p.unionRows = U.rows + row * WP;
    p.ringRows = withRings ? h->mapUnionRings.rows + row * WP : nullptr;
    p.slab = U.vertices + row * SLAB * 2;
    p.flags = flags;
    p.nextId = nextId;
    p.outPlanes = M.back.planes;
    p.outRings = M.back.rings;
    p.outVertices = M.back.vertices;
    p.outTracks = M.back.tracks;
    p.outTags = M.back.tags;
    p.planesCapacity = b.planes;
    p.ringsCapacity = b.rings;
    p.verticesCapacity = b.vertices;
    p.plan = h->mapCommit.plan;
    p.header = header;
    return p;
}
// the retired log's arrays take what `log` says, their contents kept (behind drain_handle: a call in flight may read them)
int grow_retired_log(cape_handle_s* h, const cape::MaintainLog& log)
{
    auto& R = h->mapMaintain;
    const auto drain = [h] { return drain_handle(h); };
    CAPE_HIP_TRY(R.planes.grow_keeping((size_t)log.planesCapacity, (size_t)R.nPlanes, drain));
    CAPE_HIP_TRY(R.tracks.grow_keeping((size_t)log.planesCapacity, (size_t)R.nPlanes, drain));
    CAPE_HIP_TRY(R.rings.grow_keeping((size_t)log.ringsCapacity, (size_t)R.nRings, drain));
    CAPE_HIP_TRY(R.vertices.grow_keeping((size_t)log.verticesCapacity * 2, (size_t)R.nVertices * 2, drain));
    return CAPE_OK;
}
// what the log holds after a DONE maintenance
void retired_log_holds(cape_handle_s* h, const cape_map_maintain_result& done)
{
    auto& R = h->mapMaintain;
    R.nPlanes = done.n_retired;
    R.nRings = done.n_retired_rings;
    R.nVertices = done.n_retired_vertices;
}

// cape_map_step and cape_map_step_visible: one frame through match, Kalman step, union with cuts, commit and maintenance, the last
// decided on the device from the commit's header.  Every buffer is grown before the first launch; one copy brings both headers back,
// one wait ends the call; the host learns which buffer set holds the map from the same function the maintenance kernels took their
// source from.  visible == nullptr: the gate reads the caller's skip words (or none).  Else they are decided ahead of the gate, on
// the same stream, from the pose row the gate reads and the front set's planes and tracks, into MapStepVisible::skip; their
// counters come back in a second small copy before the one wait.
int map_step_body(cape_handle h, int32_t frame, const double* world_to_camera, const uint32_t* skip, cape_map_step_visible_result* visible, uint32_t match_flags,
                  uint32_t commit_flags, uint64_t* next_id, cape_map_step_result* out, void* stream_)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    constexpr uint32_t kStepMatchFlags = CAPE_MATCH_ADVANCED | CAPE_MATCH_ALLOW_INDEX0;
    if (!h || !out || !next_id || !world_to_camera || frame < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, result, next_id or pose, or a negative frame");
    if (match_flags & (CAPE_MATCH_MAP_AREAS | CAPE_MATCH_MAP_DEVICE_SKIP))
        return fail(CAPE_ERR_INVALID_ARGUMENT, visible ? "cape_map_step_visible takes neither CAPE_MATCH_MAP_AREAS nor CAPE_MATCH_MAP_DEVICE_SKIP (it decides the words itself)"
                                                       : "cape_map_step takes neither CAPE_MATCH_MAP_AREAS nor CAPE_MATCH_MAP_DEVICE_SKIP (the visibility words do not survive a commit)");
    if ((match_flags & ~kStepMatchFlags) || (commit_flags & ~(uint32_t)CAPE_COMMIT_ADD_STAGED))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown match or commit flag");
    auto& M = h->maps;
    auto& K = h->kalman;
    auto& U = h->mapUnion;
    auto& R = h->mapMaintain;
    auto& S = h->mapStep;
    auto& SV = h->mapStepVisible;
    if (M.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (M.tracksN != M.n)
        return fail(CAPE_ERR_CAPACITY, "no tracks are current for the map (cape_map_upload_tracks, or a DONE commit, maintenance or step)");
    if (frame >= h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "`frame` lies beyond the frames of the last cape_build_polygons (build the polygons of the batch first)");
    if (frame >= h->measure.frames)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_measure of the current batch covers `frame`");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    // the step works in row 0 of the batch-wide tables of the three calls it stands for: whatever they held is gone from here on
    h->mapWide.matchFrames = 0;
    invalidate_frame_results(h);
    U.unionFrames = 0;
    h->mapUnionRings.current = false;
    // ---- every buffer of the five steps, before the first launch.  The wide match of frame `frame`: its pose and skip words at
    // row 0, its chain found through the chain base
    const int nMap = M.n;
    const size_t n = (size_t)nMap;
    MapMatchCall match = wide_map_match_call(h, 1, world_to_camera, skip, match_flags);
    match.chainBase = frame;
    if (const int rc = prepare_map_match(h, match); rc != CAPE_OK)
        return rc;
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    CAPE_HIP_TRY(K.frames.grow(1, drain));
    CAPE_HIP_TRY(K.rows.grow(WP, drain));
    CAPE_HIP_TRY(K.trackResults.grow(std::max<size_t>(n, 1), drain));
    CAPE_HIP_TRY(U.rows.grow(WP, drain));
    CAPE_HIP_TRY(U.vertices.grow(SLAB * 2, drain));
    CAPE_HIP_TRY(h->mapUnionRings.rows.grow(WP, drain));
    // the commit's destination and the maintenance's, both to the commit's bounds: the committed map is the largest of the three
    const CommitBounds bounds = commit_bounds(h);
    CAPE_HIP_TRY(M.back.grow(bounds.planes, bounds.rings, bounds.vertices, drain));
    CAPE_HIP_TRY(h->mapCommit.plan.ensure(CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(M.third.grow(bounds.planes, bounds.rings, bounds.vertices, drain));
    // ... and the log, for the committed map's bounds in place of a map's sizes (the kernels derive the log's capacities from the
    // committed sizes, which are no larger)
    cape::MaintainLog log{};
    log.held = cape::MaintainCursor {R.nPlanes, R.nRings, R.nVertices};
    if (const int rc = grow_retired_log(h, cape::maintain_log_bounds(log.held, bounds.planes, bounds.rings, bounds.vertices)); rc != CAPE_OK)
        return rc;
    CAPE_HIP_TRY(R.plan.ensure(CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(S.header.ensure(1));
    if (!S.headerHost)
        CAPE_HIP_TRY(S.headerHost.alloc_host(1, hipHostMallocDefault));
    // ... and what the visibility kernels take: one frame's words, work list and tier lists, the counters' pinned twin
    const VisibilityWorkLayout visLay = visibility_work_layout(n);
    const bool decide = visible && nMap > 0; // (an empty map has no words: no kernel runs for them)
    if (visible)
    {
        SV.n = -1; // (whatever words it held: gone from here on)
        CAPE_HIP_TRY(SV.skip.grow(CAPE_MAP_MAX_PLANES / 32, drain));
        CAPE_HIP_TRY(SV.work.grow(visLay.total, drain));
        if (!SV.countsHost)
            CAPE_HIP_TRY(SV.countsHost.alloc_host(16, hipHostMallocDefault));
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    cape_map_step_result result{};
    unsigned counts[16] = {};
    {
        StreamScope streamScope(h, stream);
        if (streamScope.rc() != CAPE_OK)
            return streamScope.rc();
        // ---- the frame's skip words, where the call decides them: behind the pose upload and ahead of the gate, from the pose row
        // the gate reads and the FRONT set's planes and tracks
        const auto decide_words = [&](cape::MatchMapParams& pm) -> int {
            if (!decide)
                return CAPE_OK;
            cape::MapVisibilityParams pv = bind_map_visibility(h, SV.work, visLay, n);
            pv.poses = pm.poses;
            pv.skip = SV.skip;
            CAPE_HIP_TRY(cape::launch_map_step_visibility(pv, M.front.tracks, stream));
            pm.skip = SV.skip;
            return CAPE_OK;
        };
        if (const int rc = enqueue_map_match(h, match, nullptr, stream, decide_words); rc != CAPE_OK)
            return rc;
        // ---- the Kalman step and the union with cuts on the same rows
        CAPE_HIP_TRY(cape::launch_map_kalman(bind_map_kalman(h), 1, stream));
        ++K.runs; // (cape_map_union's results belong to the rows this call replaced)
        CAPE_HIP_TRY(cape::launch_map_union_cut(bind_map_union(h), h->mapUnionRings.rows, 1, stream));
        // ---- the commit: front set -> back set
        cape_map_step_result* header = S.header.get();
        const cape::MapCommitParams pc = bind_map_commit(h, 0, frame, true, commit_flags, *next_id, bounds, &header->commit);
        CAPE_HIP_TRY(cape::launch_map_commit(pc, commit_planes_bound(h, bounds, commit_flags), stream));
        // ---- the maintenance behind it: back set -> third set, its sizes and whether it runs read from the commit's header
        cape::MapStepParams ps{};
        ps.commit = &header->commit;
        ps.maintain = bind_map_maintain(h, M.back, M.third, MapSizes{}, log, R.plan, &header->maintain);
        CAPE_HIP_TRY(cape::launch_map_step_maintain(ps, commit_planes_bound(h, bounds, commit_flags), stream));
        CAPE_HIP_TRY(hipMemcpyAsync(S.headerHost, S.header, sizeof(cape_map_step_result), hipMemcpyDeviceToHost, stream));
        if (decide)
            CAPE_HIP_TRY(hipMemcpyAsync(SV.countsHost, SV.work + visLay.counts, sizeof(counts), hipMemcpyDeviceToHost, stream));
        CAPE_HIP_TRY(hipStreamSynchronize(stream)); // the one wait of the call: both headers, and with them every kernel
        result = *S.headerHost.get();
        if (decide)
            std::memcpy(counts, SV.countsHost.get(), sizeof(counts));
    }
    if (visible)
    {
        // the words stand for the map as the call found it, whatever becomes of it below
        SV.n = nMap;
        visible->n_map = nMap;
        visible->n_moving = (int32_t)counts[10];
        visible->n_listed = (int32_t)counts[11];
        unsigned long long undecided = 0;
        std::memcpy(&undecided, counts + 8, sizeof(undecided));
        visible->n_undecided = (int64_t)undecided;
    }
    // ---- where the map lies now, and what it holds
    const cape::StepMapState after = cape::step_map_after(result.commit, result.maintain);
    if (after.set != cape::kStepSetFront)
    {
        adopt_map(h, after.set == cape::kStepSetBack ? M.back : M.third, MapSizes {after.planes, after.rings, after.vertices});
        invalidate_for_new_map(h);
        *next_id = result.commit.next_id;
    }
    if (result.maintain.flags & CAPE_MAINTAIN_DONE)
        retired_log_holds(h, result.maintain);
    K.matchedThisMap = false; // (the one-frame match is the step's own: a cape_map_kalman needs a cape_match_map_wide of its frames)
    *out = result;
    return CAPE_OK;
}

} // namespace

extern "C" {

int cape_map_measure(cape_handle h, int32_t n_frames, const double* camera_to_world, const double* pose_covariance, void* stream_)
{
    if (!h || n_frames < 0 || !pose_covariance)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, negative frame count or no pose covariance (the zero matrix is not a valid covariance)");
    if (n_frames > h->poly.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_build_polygons (build the polygons of the batch first)");
    auto& M = h->measure;
    M.frames = 0;
    invalidate_frame_results(h); // (cape_map_kalman's results belong to the rows this call replaces)
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const size_t B = (size_t)h->cfg.max_batch, nRecords = B + (size_t)h->chain.spillRecords; // a row / slab per record, spill pool included
    const size_t slab = (size_t)h->boundaryCap * 2;
    const bool fresh = !M.rows || !M.vertices;
    CAPE_HIP_TRY(M.rows.ensure(nRecords * CAPE_MAX_PLANES));
    CAPE_HIP_TRY(M.vertices.ensure(nRecords * slab));
    CAPE_HIP_TRY(M.poses.ensure(B * 25));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    if (fresh)
    {
        // (rows and slabs of records outside the chains of a call's frames are never written: they read as zeros)
        CAPE_HIP_TRY(hipMemsetAsync(M.rows, 0, nRecords * CAPE_MAX_PLANES * sizeof(cape_plane_measurement), stream));
        CAPE_HIP_TRY(hipMemsetAsync(M.vertices, 0, nRecords * slab * sizeof(double), stream));
    }
    // the poses (the identity where none are given), then the pose covariances, through the pinned twin like cape_match_map_wide's
    const size_t poseBytes = (size_t)n_frames * 16 * sizeof(double), covBytes = (size_t)n_frames * 9 * sizeof(double);
    CAPE_HIP_TRY(M.posesTwin.upload(M.poses, poseBytes + covBytes, B * 25 * sizeof(double), stream, [&](void* stage) {
        fill_poses(stage, n_frames, camera_to_world, poseBytes, nullptr, 0);
        std::memcpy(static_cast<unsigned char*>(stage) + poseBytes, pose_covariance, covBytes);
    }));
    cape::MapMeasureParams p{};
    p.records = h->res.records;
    p.polygons = h->poly.polygons;
    p.vertices = reinterpret_cast<const double2*>(h->poly.vertices.get());
    p.boundaryCapacity = h->boundaryCap;
    p.maxBatch = h->cfg.max_batch;
    p.nRecords = (int)nRecords;
    p.poses = M.poses;
    p.poseCov = M.poses + (size_t)n_frames * 16;
    p.rows = M.rows;
    p.worldVertices = reinterpret_cast<double2*>(M.vertices.get());
    CAPE_HIP_TRY(cape::launch_map_measure(p, n_frames, stream));
    M.frames = n_frames;
    return CAPE_OK;
}

int cape_device_map_measurements(cape_handle h, cape_plane_measurement** rows, double** world_vertices)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (h->measure.frames <= 0)
        return fail(CAPE_ERR_CAPACITY, "no measurements of the current batch: cape_map_measure has not run since the last cape_build_polygons");
    if (rows)
        *rows = h->measure.rows;
    if (world_vertices)
        *world_vertices = h->measure.vertices;
    return CAPE_OK;
}

int cape_copy_map_measurements(cape_handle h, int32_t n_frames, cape_plane_measurement* rows, double* world_vertices)
{
    if (!h || n_frames < 0 || n_frames > h->cfg.max_batch)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& M = h->measure;
    if (n_frames > M.frames)
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_measure of the current batch");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t n = (size_t)n_frames;
    CAPE_HIP_TRY(copy_out(rows, M.rows, 0, n * CAPE_MAX_PLANES));
    CAPE_HIP_TRY(copy_out(world_vertices, M.vertices, 0, n * (size_t)h->boundaryCap * 2));
    return CAPE_OK;
}

int cape_copy_spill_measurements(cape_handle h, int32_t first, int32_t count, cape_plane_measurement* rows, double* world_vertices)
{
    if (!h || first < 0 || count < 0 || first > h->chain.spillRecords || count > h->chain.spillRecords - first)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / spill record range");
    const auto& M = h->measure;
    if (M.frames <= 0)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_measure has run on the current batch");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t at = (size_t)h->cfg.max_batch + (size_t)first, n = (size_t)count, cap = (size_t)h->boundaryCap;
    CAPE_HIP_TRY(copy_out(rows, M.rows, at * CAPE_MAX_PLANES, n * CAPE_MAX_PLANES));
    CAPE_HIP_TRY(copy_out(world_vertices, M.vertices, at * cap * 2, n * cap * 2));
    return CAPE_OK;
}

int cape_map_kalman(cape_handle h, int32_t n_frames, void* stream_)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& K = h->kalman;
    const auto& W = h->mapWide;
    const auto& M = h->measure;
    const int nMap = h->maps.n;
    K.kalmanFrames = 0;
    if (nMap < 0 || h->maps.tracksN != nMap)
        return fail(CAPE_ERR_CAPACITY, "no tracks for the uploaded map (cape_map_upload, then cape_map_upload_tracks)");
    if (!K.matchedThisMap || W.matchN != nMap || n_frames > W.matchFrames)
        return fail(CAPE_ERR_CAPACITY, "no cape_match_map_wide of the current batch against the uploaded map covers n_frames");
    if (n_frames > M.frames)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_measure of the current batch covers n_frames");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be writing them
    CAPE_HIP_TRY(K.frames.grow((size_t)n_frames, drain));
    CAPE_HIP_TRY(K.rows.grow((size_t)n_frames * WP, drain));
    CAPE_HIP_TRY(K.trackResults.grow((size_t)n_frames * (size_t)std::max(nMap, 1), drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    CAPE_HIP_TRY(cape::launch_map_kalman(bind_map_kalman(h), n_frames, stream));
    K.kalmanFrames = n_frames;
    K.kalmanN = nMap;
    ++K.runs; // (cape_map_union's results belong to the rows this call replaced)
    return CAPE_OK;
}

int cape_device_map_kalman(cape_handle h, cape_frame_map_kalman** frames, cape_plane_fusion** rows, cape_map_track_result** track_results)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!kalman_results_live(h))
        return fail(CAPE_ERR_CAPACITY, "no cape_map_kalman has run on the current batch, map, match and measurements");
    if (frames)
        *frames = h->kalman.frames;
    if (rows)
        *rows = h->kalman.rows;
    if (track_results)
        *track_results = h->kalman.trackResults;
    return CAPE_OK;
}

int cape_copy_map_kalman(cape_handle h, int32_t n_frames, cape_frame_map_kalman* frames, cape_plane_fusion* rows,
                         cape_map_track_result* track_results)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& K = h->kalman;
    if (n_frames > (kalman_results_live(h) ? K.kalmanFrames : 0))
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_kalman on the current batch, map, match and measurements");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(frames, K.frames, 0, (size_t)n_frames));
    CAPE_HIP_TRY(copy_out(rows, K.rows, 0, (size_t)n_frames * WP));
    CAPE_HIP_TRY(copy_out(track_results, K.trackResults, 0, (size_t)n_frames * (size_t)K.kalmanN));
    return CAPE_OK;
}

// cape_map_union, cape_map_union_holes and cape_map_union_cut: the same preconditions, rows and slab; the kernels of the last two
// and their rings table
enum MapUnionMode { kUnionPlain, kUnionWithHoles, kUnionWithCuts };
static int map_union(cape_handle h, int32_t n_frames, void* stream_, MapUnionMode mode)
{
    const bool holes = mode != kUnionPlain;
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& U = h->mapUnion;
    const auto& K = h->kalman;
    U.unionFrames = 0;
    h->mapUnionRings.current = false;
    if (!kalman_results_live(h) || n_frames > K.kalmanFrames || K.kalmanN != h->maps.n)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_kalman on the current batch, map, tracks and measurements covers n_frames");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be writing them
    CAPE_HIP_TRY(U.rows.grow((size_t)n_frames * WP, drain));
    CAPE_HIP_TRY(U.vertices.grow((size_t)n_frames * SLAB * 2, drain));
    if (holes)
        CAPE_HIP_TRY(h->mapUnionRings.rows.grow((size_t)n_frames * WP, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    const cape::MapUnionParams p = bind_map_union(h);
    CAPE_HIP_TRY(mode == kUnionWithCuts    ? cape::launch_map_union_cut(p, h->mapUnionRings.rows, n_frames, stream)
                 : mode == kUnionWithHoles ? cape::launch_map_union_holes(p, h->mapUnionRings.rows, n_frames, stream)
                                           : cape::launch_map_union(p, n_frames, stream));
    U.unionFrames = n_frames;
    U.kalmanRun = K.runs;
    h->mapUnionRings.current = holes;
    return CAPE_OK;
}

int cape_map_union(cape_handle h, int32_t n_frames, void* stream) { return map_union(h, n_frames, stream, kUnionPlain); }
int cape_map_union_holes(cape_handle h, int32_t n_frames, void* stream) { return map_union(h, n_frames, stream, kUnionWithHoles); }
int cape_map_union_cut(cape_handle h, int32_t n_frames, void* stream) { return map_union(h, n_frames, stream, kUnionWithCuts); }

int cape_device_map_union_rings(cape_handle h, cape_plane_union_rings** rings)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!union_results_live(h) || !h->mapUnionRings.current)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_union_holes or cape_map_union_cut has run on the current batch, map, match, measurements and Kalman results, or a cape_map_union has replaced its rows");
    if (rings)
        *rings = h->mapUnionRings.rows;
    return CAPE_OK;
}

int cape_copy_map_union_rings(cape_handle h, int32_t n_frames, cape_plane_union_rings* rings)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& U = h->mapUnion;
    if (n_frames > (union_results_live(h) && h->mapUnionRings.current ? U.unionFrames : 0))
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_union_holes or cape_map_union_cut on the current batch, map, match, measurements and Kalman results (a cape_map_union replaces its rows)");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(rings, h->mapUnionRings.rows, 0, (size_t)n_frames * WP));
    return CAPE_OK;
}

int cape_device_map_union(cape_handle h, cape_plane_union** rows, double** vertices)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!union_results_live(h))
        return fail(CAPE_ERR_CAPACITY, "no cape_map_union has run on the current batch, map, match, measurements and Kalman results");
    if (rows)
        *rows = h->mapUnion.rows;
    if (vertices)
        *vertices = h->mapUnion.vertices;
    return CAPE_OK;
}

int cape_copy_map_union(cape_handle h, int32_t n_frames, cape_plane_union* rows, double* vertices)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES, SLAB = CAPE_MAP_UNION_FRAME_VERTICES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& U = h->mapUnion;
    if (n_frames > (union_results_live(h) ? U.unionFrames : 0))
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_union on the current batch, map, match, measurements and Kalman results");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(rows, U.rows, 0, (size_t)n_frames * WP));
    CAPE_HIP_TRY(copy_out(vertices, U.vertices, 0, (size_t)n_frames * SLAB * 2));
    return CAPE_OK;
}

// cape_map_commit: the sequential step of a tracking loop.  Two launches behind the union, then the one small read that tells the host
// the new map's sizes: front and back buffers are swapped here, on the host, only if the header says DONE.
int cape_map_commit(cape_handle h, int32_t frame, uint32_t flags, uint64_t* next_id, cape_map_commit_result* out, void* stream_)
{
    if (!h || !out || !next_id || frame < 0 || (flags & ~(uint32_t)CAPE_COMMIT_ADD_STAGED))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, result or next_id, a negative frame or an unknown flag");
    auto& M = h->maps;
    auto& X = h->mapCommit;
    if (!union_results_live(h) || frame >= h->mapUnion.unionFrames || h->kalman.kalmanN != M.n || M.tracksN != M.n)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_union, cape_map_union_holes or cape_map_union_cut on the current batch, map, match, measurements and Kalman results covers `frame`");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    // the back set, to bounds the host knows
    const CommitBounds bounds = commit_bounds(h);
    CAPE_HIP_TRY(M.back.grow(bounds.planes, bounds.rings, bounds.vertices, [h] { return drain_handle(h); }));
    CAPE_HIP_TRY(X.plan.ensure(CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(X.header.ensure(1));
    if (!X.headerHost)
        CAPE_HIP_TRY(X.headerHost.alloc_host(1, hipHostMallocDefault));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    cape_map_commit_result result{};
    {
        StreamScope streamScope(h, stream);
        if (streamScope.rc() != CAPE_OK)
            return streamScope.rc();
        const cape::MapCommitParams p = bind_map_commit(h, (size_t)frame, frame, h->mapUnionRings.current, flags, *next_id, bounds, X.header);
        CAPE_HIP_TRY(cape::launch_map_commit(p, commit_planes_bound(h, bounds, flags), stream));
        CAPE_HIP_TRY(hipMemcpyAsync(X.headerHost, X.header, sizeof(cape_map_commit_result), hipMemcpyDeviceToHost, stream));
        CAPE_HIP_TRY(hipStreamSynchronize(stream)); // the one wait of the call: the header, and with it both kernels
        result = *X.headerHost.get();
    }
    if (result.flags & CAPE_COMMIT_DONE)
    {
        adopt_map(h, M.back, MapSizes {result.n_planes, result.n_rings, result.n_vertices});
        invalidate_for_new_map(h);
        *next_id = result.next_id;
    }
    *out = result;
    return CAPE_OK;
}

// cape_map_maintain: PROMOTE, DROP and LOST executed on the device map.  Like the commit: two launches, then the one small read that
// tells the host the new sizes; front and back buffers are swapped here, on the host, only if the header says DONE.
int cape_map_maintain(cape_handle h, uint32_t flags, cape_map_maintain_result* out, void* stream_)
{
    if (!h || !out || flags != 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or result, or a flag (none is defined)");
    auto& M = h->maps;
    auto& R = h->mapMaintain;
    if (M.n < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "no map has been uploaded (cape_map_upload)");
    if (M.tracksN != M.n)
        return fail(CAPE_ERR_CAPACITY, "no tracks are current for the map (cape_map_upload_tracks, or a DONE cape_map_commit)");
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    // the back set and the log, to bounds the host knows: the new map is no larger than the old one, and the log takes at most
    // the whole map on top of what it holds
    const MapSizes sizes{M.n, M.nRings, M.nVertices};
    CAPE_HIP_TRY(M.back.grow((size_t)sizes.planes, (size_t)sizes.rings, (size_t)sizes.vertices, [h] { return drain_handle(h); }));
    const cape::MaintainLog log = cape::maintain_log_bounds(cape::MaintainCursor {R.nPlanes, R.nRings, R.nVertices}, (uint64_t)sizes.planes,
                                                            (uint64_t)sizes.rings, (uint64_t)sizes.vertices);
    if (const int rc = grow_retired_log(h, log); rc != CAPE_OK)
        return rc;
    CAPE_HIP_TRY(R.plan.ensure(CAPE_MAP_MAX_PLANES));
    CAPE_HIP_TRY(R.header.ensure(1));
    if (!R.headerHost)
        CAPE_HIP_TRY(R.headerHost.alloc_host(1, hipHostMallocDefault));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    cape_map_maintain_result result{};
    {
        StreamScope streamScope(h, stream);
        if (streamScope.rc() != CAPE_OK)
            return streamScope.rc();
        CAPE_HIP_TRY(cape::launch_map_maintain(bind_map_maintain(h, M.front, M.back, sizes, log, R.plan, R.header), stream));
        CAPE_HIP_TRY(hipMemcpyAsync(R.headerHost, R.header, sizeof(cape_map_maintain_result), hipMemcpyDeviceToHost, stream));
        CAPE_HIP_TRY(hipStreamSynchronize(stream)); // the one wait of the call: the header, and with it both kernels
        result = *R.headerHost.get();
    }
    if (result.flags & CAPE_MAINTAIN_DONE)
    {
        adopt_map(h, M.back, MapSizes {result.n_planes, result.n_rings, result.n_vertices});
        invalidate_for_new_map(h);
        retired_log_holds(h, result);
    }
    *out = result;
    return CAPE_OK;
}

int cape_map_retired_info(cape_handle h, int32_t* n_planes, int32_t* n_rings, int64_t* n_vertices)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (n_planes)
        *n_planes = h->mapMaintain.nPlanes;
    if (n_rings)
        *n_rings = h->mapMaintain.nRings;
    if (n_vertices)
        *n_vertices = h->mapMaintain.nVertices;
    return CAPE_OK;
}

int cape_map_retired_download(cape_handle h, cape_map_plane* planes, int32_t planes_capacity, cape_map_ring* rings, int32_t rings_capacity,
                              double* vertices, int64_t vertices_capacity, cape_map_track* tracks)
{
    if (!h || planes_capacity < 0 || rings_capacity < 0 || vertices_capacity < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative capacity");
    const auto& R = h->mapMaintain;
    if (R.nPlanes > planes_capacity || R.nRings > rings_capacity || R.nVertices > vertices_capacity)
        return fail(CAPE_ERR_CAPACITY, "an array is too small for the retired log (cape_map_retired_info tells its sizes)");
    if ((R.nPlanes > 0 && !planes) || (R.nRings > 0 && !rings) || (R.nVertices > 0 && !vertices))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null array");
    if (R.nPlanes == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(hipMemcpy(planes, R.planes, (size_t)R.nPlanes * sizeof(cape_map_plane), hipMemcpyDeviceToHost));
    CAPE_HIP_TRY(hipMemcpy(rings, R.rings, (size_t)R.nRings * sizeof(cape_map_ring), hipMemcpyDeviceToHost));
    CAPE_HIP_TRY(hipMemcpy(vertices, R.vertices, (size_t)R.nVertices * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (tracks)
        CAPE_HIP_TRY(hipMemcpy(tracks, R.tracks, (size_t)R.nPlanes * sizeof(cape_map_track), hipMemcpyDeviceToHost));
    return CAPE_OK;
}

int cape_map_retired_clear(cape_handle h)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    auto& R = h->mapMaintain;
    if (R.nPlanes > 0)
    {
        CAPE_ON_DEVICE(h);
        CAPE_HIP_TRY(drain_handle(h));
    }
    R.nPlanes = R.nRings = 0;
    R.nVertices = 0;
    return CAPE_OK;
}

int cape_map_step(cape_handle h, int32_t frame, const double* world_to_camera, const uint32_t* skip, uint32_t match_flags, uint32_t commit_flags,
                  uint64_t* next_id, cape_map_step_result* out, void* stream)
{
    return map_step_body(h, frame, world_to_camera, skip, nullptr, match_flags, commit_flags, next_id, out, stream);
}

// cape_map_step_visible: cape_map_step with the frame's skip words decided on the device, ahead of the gate, from the tracks' moving
// bits and the map as the call finds it
int cape_map_step_visible(cape_handle h, int32_t frame, const double* world_to_camera, uint32_t match_flags, uint32_t commit_flags,
                          uint64_t* next_id, cape_map_step_visible_result* out, void* stream)
{
    if (!out)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle, result, next_id or pose, or a negative frame");
    cape_map_step_visible_result result{}; // (what describes the words beside the step's result: filled by the body)
    if (const int rc = map_step_body(h, frame, world_to_camera, nullptr, &result, match_flags, commit_flags, next_id, &result.step, stream); rc != CAPE_OK)
        return rc;
    *out = result;
    return CAPE_OK;
}

int cape_map_step_skip_words(cape_handle h, uint32_t* words, int32_t words_capacity, int32_t* n_map)
{
    if (!h || words_capacity < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative capacity");
    const auto& SV = h->mapStepVisible;
    if (SV.n < 0)
        return fail(CAPE_ERR_CAPACITY, "no cape_map_step_visible has run since the last cape_map_upload");
    if (n_map)
        *n_map = SV.n;
    const int nWords = (SV.n + 31) / 32;
    if (nWords > words_capacity)
        return fail(CAPE_ERR_CAPACITY, "words_capacity is too small for the words of the last cape_map_step_visible ((n_map + 31) / 32)");
    if (nWords == 0)
        return CAPE_OK;
    if (!words)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null words");
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    CAPE_HIP_TRY(copy_out(words, SV.skip, 0, (size_t)nWords));
    return CAPE_OK;
}

} // extern "C"

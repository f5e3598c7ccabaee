// C ABI, host side: the stage between the match and the update -- a batch of pose hypotheses per frame scored against the frame's
// map matches (cape_pose_score.hip).  It reads the front map, its tracks, the batch's records and the last cape_match_map_wide and
// writes only the buffers of cape_handle_s::PoseScore.
#include <algorithm>
#include <cstring>

#include "cape_api_map.h"

using namespace cape::abi;

namespace {

constexpr uint32_t kPoseScoreFlags = CAPE_POSE_SCORE_DEVICE_POSES | CAPE_POSE_SCORE_RESIDUALS;
constexpr size_t kPoseResidualsBudget = (size_t)1 << 30; // bytes of the per-pair table at most, like kMapAreasBudget
constexpr size_t kPoseResidualDoubles = (size_t)CAPE_MATCH_MAP_WIDE_MAX_PLANES * 7; // of one (frame, hypothesis)

} // namespace

extern "C" {

int cape_map_pose_score(cape_handle h, int32_t n_frames, int32_t n_hypotheses, const double* world_to_camera, uint32_t flags, void* stream_)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    // (what needs no handle comes first)
    if (n_hypotheses < 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "n_hypotheses must be at least 1");
    if (flags & ~kPoseScoreFlags)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown pose-score flag");
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (!world_to_camera && n_frames > 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null poses");
    auto& P = h->poseScore;
    const auto& W = h->mapWide;
    const int nMap = h->maps.n;
    P.frames = 0;
    if (nMap < 0 || h->maps.tracksN != nMap)
        return fail(CAPE_ERR_CAPACITY, "no tracks for the uploaded map (cape_map_upload, then cape_map_upload_tracks)");
    if (!h->kalman.matchedThisMap || W.matchN != nMap || n_frames > W.matchFrames)
        return fail(CAPE_ERR_CAPACITY, "no cape_match_map_wide of the current batch against the uploaded map covers n_frames");
    const size_t rowsPerFrame = (size_t)n_hypotheses, rows = (size_t)n_frames * rowsPerFrame;
    const bool keep = (flags & CAPE_POSE_SCORE_RESIDUALS) != 0, devicePoses = (flags & CAPE_POSE_SCORE_DEVICE_POSES) != 0;
    if (keep && rows > kPoseResidualsBudget / (kPoseResidualDoubles * sizeof(double)))
        return fail(CAPE_ERR_CAPACITY, "the residual table of this call would exceed 1 GiB (fewer frames or hypotheses per call, or no CAPE_POSE_SCORE_RESIDUALS)");
    if ((rowsPerFrame + cape::kPoseScoreGroupHypotheses - 1) / cape::kPoseScoreGroupHypotheses > 65535)
        return fail(CAPE_ERR_CAPACITY, "more than 65 535 x 256 hypotheses per frame");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    const size_t poseDoubles = rows * 16;
    if (!devicePoses && P.poses.size() < poseDoubles)
    {
        // (the pinned twin has the size of its device buffer: both are replaced)
        CAPE_HIP_TRY(drain());
        P.posesTwin = PinnedTwin{};
        CAPE_HIP_TRY(P.poses.alloc(poseDoubles));
    }
    CAPE_HIP_TRY(P.frameInfo.grow((size_t)n_frames, drain));
    CAPE_HIP_TRY(P.features.grow((size_t)n_frames * WP, drain));
    CAPE_HIP_TRY(P.scores.grow(rows, drain));
    if (keep)
        CAPE_HIP_TRY(P.residuals.grow(rows * kPoseResidualDoubles, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    if (!devicePoses)
        CAPE_HIP_TRY(P.posesTwin.upload(P.poses, poseDoubles * sizeof(double), P.poses.size() * sizeof(double), stream,
                                        [&](void* stage) { std::memcpy(stage, world_to_camera, poseDoubles * sizeof(double)); }));
    if (keep) // (rows beyond a frame's pairs read as zeros)
        CAPE_HIP_TRY(hipMemsetAsync(P.residuals, 0, rows * kPoseResidualDoubles * sizeof(double), stream));
    cape::PoseScoreParams p{};
    p.mapPlanes = h->maps.front.planes;
    p.tracks = h->maps.front.tracks;
    p.tags = h->maps.front.tags;
    p.nMap = nMap;
    p.matchFrames = W.frames;
    p.match = W.match;
    p.kept = W.kept;
    p.records = h->res.records;
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords; // (the batch's records, then the spill pool's)
    p.poses = devicePoses ? world_to_camera : P.poses.get();
    p.nHypotheses = n_hypotheses;
    p.frameInfo = P.frameInfo;
    p.features = P.features;
    p.scores = P.scores;
    p.residuals = keep ? P.residuals.get() : nullptr;
    CAPE_HIP_TRY(cape::launch_map_pose_score(p, n_frames, stream));
    P.frames = n_frames;
    P.hypotheses = n_hypotheses;
    P.keptResiduals = keep;
    return CAPE_OK;
}

int cape_copy_pose_scores(cape_handle h, int32_t n_frames, cape_pose_score* scores, cape_pose_feature* features, double* residuals)
{
    constexpr size_t WP = CAPE_MATCH_MAP_WIDE_MAX_PLANES;
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");
    const auto& P = h->poseScore;
    if (n_frames > (pose_scores_live(h) ? P.frames : 0))
        return fail(CAPE_ERR_CAPACITY, "n_frames exceeds the frames of the last cape_map_pose_score on the current batch, map, tracks and match");
    if (residuals && n_frames > 0 && !P.keptResiduals)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "the last cape_map_pose_score did not keep the residual table (CAPE_POSE_SCORE_RESIDUALS)");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_HIP_TRY(drain_handle(h));
    const size_t rows = (size_t)n_frames * (size_t)P.hypotheses;
    CAPE_HIP_TRY(copy_out(scores, P.scores, 0, rows));
    CAPE_HIP_TRY(copy_out(features, P.features, 0, (size_t)n_frames * WP));
    CAPE_HIP_TRY(copy_out(residuals, P.residuals, 0, rows * kPoseResidualDoubles));
    return CAPE_OK;
}

int cape_pose_score_device(cape_handle h, const cape_pose_score** scores, const cape_pose_feature** features)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!pose_scores_live(h))
        return fail(CAPE_ERR_CAPACITY, "no cape_map_pose_score has run on the current batch, map, tracks and match");
    if (scores)
        *scores = h->poseScore.scores;
    if (features)
        *features = h->poseScore.features;
    return CAPE_OK;
}

} // extern "C"

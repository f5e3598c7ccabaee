// C ABI, host side: the stage between the match and the update -- a batch of pose hypotheses per frame scored against the frame's
// map matches (cape_pose_score.hip).  It reads the front map, its tracks, the batch's records and the last cape_match_map_wide and
// writes the buffers of cape_handle_s::PoseScore and, where they are not current, the stage's pair rows (enqueue_pose_pairs).
#include <algorithm>
#include <cstring>

#include "cape_api_pose.h"

using namespace cape::abi;

namespace {

constexpr uint32_t kPoseScoreFlags = CAPE_POSE_SCORE_DEVICE_POSES | CAPE_POSE_SCORE_RESIDUALS;
constexpr size_t kPoseResidualsBudget = (size_t)1 << 30; // bytes of the per-pair table at most, like kMapAreasBudget
constexpr size_t kPoseResidualDoubles = (size_t)CAPE_MATCH_MAP_WIDE_MAX_PLANES * 7; // of one (frame, hypothesis)

} // namespace

extern "C" {

int cape_map_pose_score(cape_handle h, int32_t n_frames, int32_t n_hypotheses, const double* world_to_camera, uint32_t flags, void* stream_)
{
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
    P.frames = 0;
    if (const int rc = check_pose_inputs(h, n_frames); rc != CAPE_OK)
        return rc;
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
    if (const int rc = reserve_pose_pairs(h); rc != CAPE_OK)
        return rc;
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
    if (const int rc = enqueue_pose_pairs(h, n_frames, stream); rc != CAPE_OK)
        return rc;
    cape::PoseScoreParams p{};
    p.frameInfo = h->posePairs.frameInfo;
    p.features = h->posePairs.features;
    p.poses = devicePoses ? world_to_camera : P.poses.get();
    p.nHypotheses = n_hypotheses;
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
    CAPE_POSE_COPY_OUT(h, n_frames, pose_scores_live(h) ? h->poseScore.frames : 0,
                       "n_frames exceeds the frames of the last cape_map_pose_score on the current batch, map, tracks and match",
                       if (residuals && !h->poseScore.keptResiduals)
                           return fail(CAPE_ERR_INVALID_ARGUMENT, "the last cape_map_pose_score did not keep the residual table (CAPE_POSE_SCORE_RESIDUALS)"));
    const auto& P = h->poseScore;
    const size_t rows = (size_t)n_frames * (size_t)P.hypotheses;
    CAPE_HIP_TRY(copy_out(scores, P.scores, 0, rows));
    CAPE_HIP_TRY(copy_out(features, h->posePairs.features, 0, (size_t)n_frames * CAPE_MATCH_MAP_WIDE_MAX_PLANES)); // (the shared rows cover the score's frames)
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
        *features = h->posePairs.features;
    return CAPE_OK;
}

} // extern "C"

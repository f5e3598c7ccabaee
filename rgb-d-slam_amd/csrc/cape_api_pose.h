// Private header of the pose stage's entry points (cape_api_pose_score.hip, cape_api_pose_solve.hip, cape_api_pose_covariance.hip): what
// the three share that is not a stage's own arithmetic -- when a result is still current, the preconditions on the map and the match,
// the one owner of the pair rows, the upload of a call's x and subsets, and the preamble of a copy-out.  Host code only; every function
// is inline and defined here once.
#pragma once

#include "cape_api_map.h"

namespace cape::abi {

// ---- a result of the pose stage over `frames` frames still describes the current batch, map, tracks and match: a cape_extract ends the
// match; every other call that replaces an input says so through invalidate_frame_results, which zeroes the count
inline bool pose_frames_live(const cape_handle_s* h, int frames) { return frames > 0 && h->mapWide.matchFrames >= frames; }
inline bool pose_pairs_live(const cape_handle_s* h) { return pose_frames_live(h, h->posePairs.frames); }
inline bool pose_scores_live(const cape_handle_s* h) { return pose_frames_live(h, h->poseScore.frames); }
inline bool pose_solutions_live(const cape_handle_s* h) { return pose_frames_live(h, h->poseSolve.frames); }
inline bool pose_selection_live(const cape_handle_s* h) { return pose_frames_live(h, h->poseSolve.selectFrames); }
inline bool pose_covariance_live(const cape_handle_s* h) { return pose_frames_live(h, h->poseCovariance.frames); }

// ---- what score, solve and covariance need before anything else of the handle is touched: tracks for the uploaded map, and a wide
// match of the current batch against it over n_frames
inline int check_pose_inputs(const cape_handle_s* h, int n_frames)
{
    const auto& W = h->mapWide;
    const int nMap = h->maps.n;
    if (nMap < 0 || h->maps.tracksN != nMap)
        return fail(CAPE_ERR_CAPACITY, "no tracks for the uploaded map (cape_map_upload, then cape_map_upload_tracks)");
    if (!h->kalman.matchedThisMap || W.matchN != nMap || n_frames > W.matchFrames)
        return fail(CAPE_ERR_CAPACITY, "no cape_match_map_wide of the current batch against the uploaded map covers n_frames");
    return CAPE_OK;
}

// ---- the pair rows (cape_handle_s::PosePairs).  The pairs kernel runs only where the rows do not already cover n_frames for the current
// batch, map, tracks and match; a launch over more frames writes the frames it covered before again, with the bytes they hold.  A failed
// launch leaves no coverage.  reserve_pose_pairs sizes the rows once, beside the call's other buffers and ahead of its enqueueing part:
// n_frames <= mapWide.matchFrames <= max_batch (check_pose_inputs).
inline int reserve_pose_pairs(cape_handle_s* h)
{
    auto& R = h->posePairs;
    CAPE_HIP_TRY(R.frameInfo.ensure((size_t)h->cfg.max_batch));
    CAPE_HIP_TRY(R.features.ensure((size_t)h->cfg.max_batch * CAPE_MATCH_MAP_WIDE_MAX_PLANES));
    return CAPE_OK;
}
inline int enqueue_pose_pairs(cape_handle_s* h, int n_frames, hipStream_t stream)
{
    auto& R = h->posePairs;
    if (pose_pairs_live(h) && R.frames >= n_frames)
        return CAPE_OK;
    R.frames = 0;
    const auto& W = h->mapWide;
    cape::PosePairsParams p{};
    p.mapPlanes = h->maps.front.planes;
    p.tracks = h->maps.front.tracks;
    p.tags = h->maps.front.tags;
    p.nMap = h->maps.n;
    p.matchFrames = W.frames;
    p.match = W.match;
    p.kept = W.kept;
    p.records = h->res.records;
    p.nRecords = h->cfg.max_batch + h->chain.spillRecords; // (the batch's records, then the spill pool's)
    p.frameInfo = R.frameInfo;
    p.features = R.features;
    CAPE_HIP_TRY(cape::launch_map_pose_pairs(p, n_frames, stream));
    R.frames = n_frames;
    return CAPE_OK;
}

// ---- a call's x (rows x 6 doubles), then its subsets (rows x 4 words), for the groups that hold an `input` buffer and its pinned twin
// (PoseSolve, PoseCovariance).  Host memory travels through the twin; reserve_pose_input sizes the buffer for it ahead of the call's
// enqueueing part, behind drain_handle: an earlier call may still be working in it.
constexpr size_t pose_input_x_bytes(size_t rows) { return rows * 6 * sizeof(double); }
constexpr size_t pose_input_bytes(size_t rows) { return pose_input_x_bytes(rows) + rows * 4 * sizeof(uint32_t); }
template <typename Group> int reserve_pose_input(cape_handle_s* h, Group& P, size_t rows)
{
    if (P.input.size() >= pose_input_bytes(rows))
        return CAPE_OK;
    // (the pinned twin has the size of its device buffer: both are replaced)
    CAPE_HIP_TRY(drain_handle(h));
    P.inputTwin = PinnedTwin{};
    CAPE_HIP_TRY(P.input.alloc(pose_input_bytes(rows)));
    return CAPE_OK;
}
// The device addresses of x and the subsets by the call's route: the caller's host memory uploaded on the stream (read before the call
// returns), the caller's device memory as it is, or -- fromResults: a selection or a solution on the device holds both -- null.
enum class PoseInputRoute { kHost, kDevice, kFromResults };
template <typename Group>
int bind_pose_input(Group& P, PoseInputRoute route, size_t rows, const double* x, const uint32_t* subsets, hipStream_t stream, const double** xDevice,
                    const uint32_t** subsetsDevice)
{
    *xDevice = route == PoseInputRoute::kDevice ? x : nullptr;
    *subsetsDevice = route == PoseInputRoute::kDevice ? subsets : nullptr;
    if (route != PoseInputRoute::kHost)
        return CAPE_OK;
    const size_t xBytes = pose_input_x_bytes(rows), inputBytes = pose_input_bytes(rows);
    CAPE_HIP_TRY(P.inputTwin.upload(P.input, inputBytes, P.input.size(), stream, [&](void* stage) {
        std::memcpy(stage, x, xBytes);
        std::memcpy(static_cast<unsigned char*>(stage) + xBytes, subsets, inputBytes - xBytes);
    }));
    *xDevice = reinterpret_cast<const double*>(P.input.get());
    *subsetsDevice = reinterpret_cast<const uint32_t*>(P.input.get() + xBytes);
    return CAPE_OK;
}

// ---- the preamble of a copy-out: the handle and the count, the result's liveness, nothing to copy, then the handle's device and its
// enqueued work done.  `frames`: the frames the result covers where it is current, else 0 (evaluated behind the null check).  What
// follows the message is a refusal of the call's own, if it has one: a statement that runs behind these checks and ahead of any
// device work.  Returns from the entry point where a check fails, and with CAPE_OK for no frames.
#define CAPE_POSE_COPY_OUT(h, n_frames, frames, message, ...)                                                 \
    if (!(h) || (n_frames) < 0)                                                                               \
        return ::cape::abi::fail(CAPE_ERR_INVALID_ARGUMENT, "bad handle / frame count");                      \
    if ((n_frames) > (frames))                                                                                \
        return ::cape::abi::fail(CAPE_ERR_CAPACITY, message);                                                 \
    if ((n_frames) == 0)                                                                                      \
        return CAPE_OK;                                                                                       \
    __VA_ARGS__;                                                                                              \
    CAPE_ON_DEVICE(h);                                                                                        \
    CAPE_HIP_TRY(drain_handle(h))

} // namespace cape::abi

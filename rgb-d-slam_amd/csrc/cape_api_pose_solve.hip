// C ABI, host side: the pose solver between the match and the update -- Levenberg-Marquardt per (frame, hypothesis) on the frame's
// map matches, the RANSAC bookkeeping over the scored hypotheses and the refit from the selection (cape_pose_solve.hip).  It reads what
// cape_map_pose_score reads, that call's score rows for the selection, and writes the buffers of cape_handle_s::PoseSolve and, where
// they are not current, the stage's pair rows (enqueue_pose_pairs).
#include <algorithm>
#include <cstring>

#include "cape_api_pose.h"

using namespace cape::abi;

namespace {

constexpr uint32_t kPoseSolveFlags = CAPE_POSE_SOLVE_DEVICE_INPUT | CAPE_POSE_SOLVE_FROM_SELECTION;

} // namespace

extern "C" {

int cape_map_pose_solve(cape_handle h, int32_t n_frames, int32_t n_hypotheses, const double* x0, const uint32_t* subsets,
                        const cape_pose_solve_params* params, uint32_t flags, void* stream_)
{
    // (what needs no handle comes first)
    if (n_hypotheses < 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "n_hypotheses must be at least 1");
    if (flags & ~kPoseSolveFlags)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "unknown pose-solve flag");
    const bool fromSelection = (flags & CAPE_POSE_SOLVE_FROM_SELECTION) != 0, deviceInput = (flags & CAPE_POSE_SOLVE_DEVICE_INPUT) != 0;
    if (fromSelection && n_hypotheses != 1)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "CAPE_POSE_SOLVE_FROM_SELECTION solves one problem per frame: n_hypotheses must be 1");
    cape::PoseSolveSettings settings;
    if (!cape::pose_solve_settings(params, settings))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "a pose-solve parameter is NaN, negative or out of range");
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    if (!fromSelection && n_frames > 0 && (!x0 || !subsets))
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null x0 or subsets");
    auto& P = h->poseSolve;
    const int selectFrames = pose_selection_live(h) ? P.selectFrames : 0;
    P.frames = 0;
    if (!fromSelection) // (the selection was made over the rows this call replaces)
        P.selectFrames = 0;
    if (const int rc = check_pose_inputs(h, n_frames); rc != CAPE_OK)
        return rc;
    if (fromSelection && n_frames > selectFrames)
        return fail(CAPE_ERR_CAPACITY, "no current cape_map_pose_select covers n_frames");
    const size_t rowsPerFrame = (size_t)n_hypotheses, rows = (size_t)n_frames * rowsPerFrame;
    if ((rowsPerFrame + cape::kPoseSolveGroupProblems - 1) / cape::kPoseSolveGroupProblems > 65535)
        return fail(CAPE_ERR_CAPACITY, "more than 65 535 x 256 hypotheses per frame");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); }; // an earlier call may still be working in them
    const PoseInputRoute route = fromSelection ? PoseInputRoute::kFromResults : deviceInput ? PoseInputRoute::kDevice : PoseInputRoute::kHost;
    if (route == PoseInputRoute::kHost)
        if (const int rc = reserve_pose_input(h, P, rows); rc != CAPE_OK)
            return rc;
    if (const int rc = reserve_pose_pairs(h); rc != CAPE_OK)
        return rc;
    CAPE_HIP_TRY(P.solutions.grow(rows, drain));
    CAPE_HIP_TRY(P.poses.grow(rows * 16, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    cape::PoseSolveParams p{};
    if (const int rc = bind_pose_input(P, route, rows, x0, subsets, stream, &p.x0, &p.subsets); rc != CAPE_OK)
        return rc;
    if (const int rc = enqueue_pose_pairs(h, n_frames, stream); rc != CAPE_OK)
        return rc;
    p.frameInfo = h->posePairs.frameInfo;
    p.features = h->posePairs.features;
    p.selection = fromSelection ? P.selection.get() : nullptr;
    p.nProblems = n_hypotheses;
    p.settings = settings;
    p.solutions = P.solutions;
    p.poses = P.poses;
    CAPE_HIP_TRY(cape::launch_map_pose_solve(p, n_frames, stream));
    P.frames = n_frames;
    P.problems = n_hypotheses;
    P.fromSelection = fromSelection;
    return CAPE_OK;
}

int cape_copy_pose_solutions(cape_handle h, int32_t n_frames, cape_pose_solution* solutions, double* world_to_camera)
{
    CAPE_POSE_COPY_OUT(h, n_frames, pose_solutions_live(h) ? h->poseSolve.frames : 0,
                       "n_frames exceeds the frames of the last cape_map_pose_solve on the current batch, map, tracks and match");
    const auto& P = h->poseSolve;
    const size_t rows = (size_t)n_frames * (size_t)P.problems;
    CAPE_HIP_TRY(copy_out(solutions, P.solutions, 0, rows));
    CAPE_HIP_TRY(copy_out(world_to_camera, P.poses, 0, rows * 16));
    return CAPE_OK;
}

int cape_pose_solve_device(cape_handle h, const cape_pose_solution** solutions, const double** world_to_camera)
{
    if (!h)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle");
    if (!pose_solutions_live(h))
        return fail(CAPE_ERR_CAPACITY, "no cape_map_pose_solve has run on the current batch, map, tracks and match");
    if (solutions)
        *solutions = h->poseSolve.solutions;
    if (world_to_camera)
        *world_to_camera = h->poseSolve.poses;
    return CAPE_OK;
}

int cape_map_pose_select(cape_handle h, int32_t n_frames, void* stream_)
{
    if (!h || n_frames < 0)
        return fail(CAPE_ERR_INVALID_ARGUMENT, "null handle or negative frame count");
    auto& P = h->poseSolve;
    const auto& S = h->poseScore;
    P.selectFrames = 0;
    if (!pose_solutions_live(h) || P.fromSelection || n_frames > P.frames)
        return fail(CAPE_ERR_CAPACITY, "no current cape_map_pose_solve over hypotheses covers n_frames");
    if (!pose_scores_live(h) || n_frames > S.frames)
        return fail(CAPE_ERR_CAPACITY, "no current cape_map_pose_score covers n_frames");
    if (S.hypotheses != P.problems)
        return fail(CAPE_ERR_CAPACITY, "the current cape_map_pose_score and cape_map_pose_solve differ in n_hypotheses");
    if (n_frames == 0)
        return CAPE_OK;
    CAPE_ON_DEVICE(h);
    CAPE_SETTLE_RESULTS(h);
    const auto drain = [h] { return drain_handle(h); };
    CAPE_HIP_TRY(P.selection.grow((size_t)n_frames, drain));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StreamScope streamScope(h, stream);
    if (streamScope.rc() != CAPE_OK)
        return streamScope.rc();
    cape::PoseSelectParams p{};
    p.scores = S.scores;
    p.solutions = P.solutions;
    p.nHypotheses = P.problems;
    p.selection = P.selection;
    CAPE_HIP_TRY(cape::launch_map_pose_select(p, n_frames, stream));
    P.selectFrames = n_frames;
    return CAPE_OK;
}

int cape_copy_pose_selection(cape_handle h, int32_t n_frames, cape_pose_selection* selection)
{
    CAPE_POSE_COPY_OUT(h, n_frames, pose_selection_live(h) ? h->poseSolve.selectFrames : 0,
                       "n_frames exceeds the frames of the last cape_map_pose_select on the current batch, map, tracks and match");
    CAPE_HIP_TRY(copy_out(selection, h->poseSolve.selection, 0, (size_t)n_frames));
    return CAPE_OK;
}

} // extern "C"

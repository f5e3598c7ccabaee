// cape_map_pose_solve / cape_map_pose_select: the pose solver on the pairs of cape_map_pose_score -- Levenberg-Marquardt per (frame,
// hypothesis) and the RANSAC bookkeeping over a frame's scored hypotheses.  The statements are those of cape_pose_solve.h, which the
// host twins cape_host_pose_solve / cape_host_pose_select compile too.  The solve reads the pose stage's shared pair rows
// (the pairs kernel of cape_pose_score.hip, enqueue_pose_pairs); both kernels write only the call's own result buffers.
//
//   cape_pose_solve_kernel : one lane per problem, one workgroup of four waves per (frame, 256 problems), as in the score kernel.
//        The frame's feature rows -- the two planes and the kept plane -- are copied to LDS once per workgroup (the reasons are in
//        the header of cape_pose_score.hip: a broadcast read without a bank conflict, and an explicit copy instead of a proof the
//        compiler would owe for scalar loads), then every lane runs MINPACK's lmstr driver on its own subset of the pairs:
//        pose_solve_problem.  Every sum is lane-private and taken in pair order: no cross-lane reduction, no atomic, and a problem's
//        bytes do not depend on which problems share its wave.  The lanes of a wave finish after different numbers of iterations
//        and of lmpar rounds; the wave runs to its slowest lane (the nfev spread per wave is in profiles/map_pose_solve_rate.txt).
//        No scratch: n = 6 is unrolled everywhere and the pivot vector of lmpar / qrsolv is resolved by selects (lm_gather,
//        lm_scatter), so R (36 doubles), Q^T f, the work vectors and the seven poses of a forward-difference Jacobian (84 doubles)
//        live in registers; the register count and the occupancy it leaves are in DESIGN.md 4.6.
//   cape_pose_select_kernel : one frame per lane-0 of a wave, four frames per workgroup: a serial scan of the frame's score and
//        solution rows (pose_select_frame), 96 bytes out.
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_layout.h"
#include "cape_map_camera.h"
#include "cape_pose_solve.h"

namespace cape {

namespace {

constexpr int WP = kPoseScoreMaxPairs;
constexpr int kSelectFrames = 4; // frames (waves) of a select workgroup
static_assert(sizeof(cape_pose_solution) == 96 && sizeof(cape_pose_selection) == 96, "the layouts of include/cape_hip.h");
static_assert(sizeof(cape_pose_solution) % 16 == 0 && sizeof(cape_pose_selection) % 16 == 0, "16-byte rows");

} // namespace

__global__ __launch_bounds__(kPoseSolveGroupProblems) void cape_pose_solve_kernel(PoseSolveParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int frame = blockIdx.x;
    const int problem = blockIdx.y * kPoseSolveGroupProblems + threadIdx.x; // the workgroup's offset, then the lane
    const int4 info = p.frameInfo[frame];
    const int nPairs = info.x < 0 ? 0 : (info.x < WP ? info.x : WP);
    double* s_planes;
    int* s_kept;
    pose_rows_stage(smem, p.features + (size_t)frame * WP, nPairs, s_planes, s_kept);
    if (problem >= p.nProblems) // (idle lanes of the frame's last workgroup store nothing)
        return;
    const size_t at = (size_t)frame * p.nProblems + problem;
    double x0[6];
    uint32_t words[4];
    bool selected = true;
    if (p.selection)
    {
        const cape_pose_selection& sel = p.selection[frame];
        selected = sel.best >= 0;
#pragma unroll
        for (int c = 0; c < 6; ++c)
            x0[c] = sel.x[c];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            words[c] = sel.inlier_words[c];
    }
    else
    {
#pragma unroll
        for (int c = 0; c < 6; ++c)
            x0[c] = p.x0[at * 6 + c];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            words[c] = p.subsets[at * 4 + c];
    }
    PoseSolveRows rows;
    rows.planes = s_planes, rows.kept = s_kept, rows.nPairs = selected ? nPairs : 0;
    pose_subset(words, rows.subsetLo, rows.subsetHi);
    double T[12];
    cape_pose_solution r = pose_solve_problem(rows, info.y, (uint32_t)info.z, x0, p.settings, DevicePlaneToCamera{}, T);
    if (!selected)
        r.status = CAPE_POSE_SOLVE_NO_SELECTION;
    store_pose_solution(p.solutions + at, r);
    double* pose = p.poses + at * 16;
#pragma unroll
    for (int c = 0; c < 12; ++c)
        pose[c] = T[c];
    pose[12] = pose[13] = pose[14] = 0.0, pose[15] = 1.0;
}

__global__ __launch_bounds__(64 * kSelectFrames) void cape_pose_select_kernel(PoseSelectParams p, int nFrames)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frame = blockIdx.x * kSelectFrames + wave;
    if (frame >= nFrames || lane != 0) // (no barrier in this kernel)
        return;
    const size_t at = (size_t)frame * p.nHypotheses;
    p.selection[frame] = pose_select_frame(p.scores + at, p.solutions + at, p.nHypotheses);
}

hipError_t launch_map_pose_solve(const PoseSolveParams& p, int nFrames, hipStream_t stream)
{
    const int groups = (p.nProblems + kPoseSolveGroupProblems - 1) / kPoseSolveGroupProblems;
    hipLaunchKernelGGL(cape_pose_solve_kernel, dim3(nFrames, groups), dim3(kPoseSolveGroupProblems), pose_rows_layout().bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_map_pose_select(const PoseSelectParams& p, int nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_pose_select_kernel, dim3((nFrames + kSelectFrames - 1) / kSelectFrames), dim3(64 * kSelectFrames), 0, stream, p, nFrames);
    return hipGetLastError();
}

} // namespace cape

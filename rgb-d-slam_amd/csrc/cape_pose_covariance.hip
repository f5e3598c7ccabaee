// cape_map_pose_covariance: compute_pose_variance on the device, one more stage on the stream behind the refit.  The statements are those
// of cape_pose_covariance.h (and, for a sample, of cape_pose_solve.h), which the host twin cape_host_pose_covariance compiles too.  It
// reads the pose stage's shared pair rows (the pairs kernel of cape_pose_score.hip, enqueue_pose_pairs); per chunk of frames that fits the
// slab's byte budget, vary and solve; at the end one reduce over all frames.
//
//   cape_pose_vary_kernel : one workgroup of 256 lanes per (frame, 256 iterations), a lane per iteration.  Lane 0 of the frame's first
//        workgroup resolves the frame's x, subset and refusal (pose_cov_frame) for the kernels behind it.  Every lane walks the frame's
//        pairs serially; for a pair of the subset it takes its four deviates -- Philox4x32-10 at the counter (frame + frame_base,
//        iteration, pair slot, block), or the caller's table [iteration][128][4] -- and stores the varied plane into the slab
//        [frame][pair][component][iteration]: the lanes of a wave write consecutive addresses, and the lanes of the solve read them so.
//        The feature row is the same address in every lane (one request); the kept planes, which name the subset's bits, go through LDS.
//   cape_pose_solve_varied_kernel : cape_pose_solve_kernel's carve and lane mapping, a lane per (frame, iteration): matched planes and
//        kept-plane indices from LDS, the map plane of pair k from the lane's column of the slab (PoseVariedRows::map_plane), the
//        minimiser the one body of pose_solve_problem.  Behind it the lane turns its x into the pose vector (pose_vector: three atan2, a
//        sin and a cos, after the minimiser's registers are dead) and stores the 64-byte sample row the reduction reads and, if kept,
//        the solution row.  Code-object figures: DESIGN.md 4.6.
//   cape_pose_cov_reduce_kernel : one wavefront per frame, four per workgroup.  Lane l < 36 owns covariance entry (l / 6, l % 6) and
//        computes the two means it needs itself: every lane walks the frame's sample rows serially in ascending iteration order over
//        the successes (the same address in all lanes), so every sum is ordered and lane-private -- no atomic, no cross-lane sum.  The
//        36 entries are then handed to every lane by shuffles and is_covariance_valid<6> (cape_map_tracking.h) decides the status.
//   cape_pose_draw_kernel : the table [iteration][128][4] of one frame index through pose_deviate_uniforms / pose_deviate_normals, the
//        device functions the vary kernel calls.
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_layout.h"
#include "cape_map_camera.h"
#include "cape_map_tracking.h"
#include "cape_pose_covariance.h"

namespace cape {

namespace {

constexpr int WP = kPoseScoreMaxPairs;
constexpr int kReduceFrames = 4; // frames (waves) of a reduce workgroup
static_assert(sizeof(cape_pose_covariance) == 368 && sizeof(cape_pose_covariance) % 16 == 0, "the layout of include/cape_hip.h, 16-byte rows");
static_assert(sizeof(PoseCovSample) == 64 && sizeof(PoseCovFrame) == 80, "the rows of cape_pose_covariance.h");

__device__ __forceinline__ int clamp_pairs(int n) { return n < 0 ? 0 : (n < WP ? n : WP); }

__device__ __forceinline__ void lane_deviates(const PoseCovParams& p, uint32_t frameIndex, int iteration, int slot, double z[4])
{
    if (p.table)
    {
        const double* row = p.table + ((size_t)iteration * WP + slot) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            z[c] = row[c];
    }
    else
    {
        double u[4];
        pose_deviate_uniforms(p.seed, frameIndex, (uint32_t)iteration, (uint32_t)slot, u);
        pose_deviate_normals(u, z);
    }
}

} // namespace

__global__ __launch_bounds__(kPoseCovGroupIterations) void cape_pose_vary_kernel(PoseCovParams p)
{
    const int frame = p.firstFrame + blockIdx.x;
    const int iteration = blockIdx.y * kPoseCovGroupIterations + threadIdx.x;
    const int4 info = p.frameInfo[frame];
    const int nPairs = clamp_pairs(info.x);
    const cape_pose_feature* features = p.features + (size_t)frame * WP;
    // ---- the frame's x, subset and refusal, by one lane of the frame's first workgroup; the kept planes name the subset's bits
    __shared__ int s_kept[WP];
    if ((int)threadIdx.x < nPairs)
        s_kept[threadIdx.x] = features[threadIdx.x].kept_plane;
    __syncthreads();
    uint32_t words[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        words[c] = p.selection ? p.selection[frame].inlier_words[c] : p.subsets[(size_t)frame * 4 + c];
    if (blockIdx.y == 0 && threadIdx.x == 0)
    {
        PoseSolveRows frameRows; // (the refusal reads the kept planes and the subset, no plane)
        frameRows.planes = nullptr, frameRows.kept = s_kept, frameRows.nPairs = nPairs, frameRows.subsetLo = frameRows.subsetHi = 0ull;
        p.frames[frame] = pose_cov_frame(frameRows, info.y, (uint32_t)info.z, p.x ? p.x + (size_t)frame * 6 : nullptr, words,
                                         p.solutions ? p.solutions + frame : nullptr, nullptr);
    }
    if (iteration >= p.nIterations)
        return;
    unsigned long long lo, hi;
    pose_subset(words, lo, hi);
    double* column = p.slab + (size_t)blockIdx.x * WP * 4 * (size_t)p.nIterations + iteration;
    const uint32_t frameIndex = (uint32_t)frame + p.frameBase;
#pragma unroll 1
    for (int k = 0; k < nPairs; ++k)
    {
        const cape_pose_feature& F = features[k];
        const int i = s_kept[k];
        if ((((i < 64 ? lo : hi) >> (i & 63)) & 1ull) == 0ull)
            continue; // (the solve never reads the planes of a pair outside the subset)
        double z[4], varied[4];
        lane_deviates(p, frameIndex, iteration, k, z);
        pose_vary_plane(F.map_plane, F.stddev, z, varied);
#pragma unroll
        for (int c = 0; c < 4; ++c)
            column[(size_t)(4 * k + c) * (size_t)p.nIterations] = varied[c];
    }
}

__global__ __launch_bounds__(kPoseCovGroupIterations) void cape_pose_solve_varied_kernel(PoseCovParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int frame = p.firstFrame + blockIdx.x;
    const int iteration = blockIdx.y * kPoseCovGroupIterations + threadIdx.x;
    const PoseCovFrame& F = p.frames[frame];
    if (F.refusal != 0) // (the whole workgroup: no lane reaches the barrier)
        return;
    const int nPairs = clamp_pairs(F.nPairs);
    double* s_planes;
    int* s_kept;
    pose_rows_stage(smem, p.features + (size_t)frame * WP, nPairs, s_planes, s_kept);
    if (iteration >= p.nIterations)
        return;
    double x0[6];
#pragma unroll
    for (int c = 0; c < 6; ++c)
        x0[c] = F.x[c];
    PoseVariedRows rows;
    rows.planes = s_planes, rows.kept = s_kept, rows.nPairs = nPairs;
    const uint32_t words[4] = {F.words[0], F.words[1], F.words[2], F.words[3]}; // (a copy, as in cape_pose_solve_kernel: handed over in
    pose_subset(words, rows.subsetLo, rows.subsetHi);                           // place, the kernel spills 15 more SGPRs)
    rows.varied = p.slab + (size_t)blockIdx.x * WP * 4 * (size_t)p.nIterations + iteration;
    rows.stride = (size_t)p.nIterations;
    double T[12];
    const cape_pose_solution r = pose_solve_problem(rows, F.nInvalid, F.frameFlags, x0, p.settings, DevicePlaneToCamera{}, T);
    const size_t at = (size_t)frame * (size_t)p.nIterations + iteration;
    if (p.kept)
        store_pose_solution(p.kept + at, r);
    const PoseCovSample s = pose_cov_sample(r);
    double* out = reinterpret_cast<double*>(p.samples + at);
#pragma unroll
    for (int c = 0; c < 6; ++c)
        out[c] = s.v[c];
    *reinterpret_cast<uint4*>(out + 6) = make_uint4((unsigned)s.status, (unsigned)s.nfev, (unsigned)s.ok, (unsigned)s.ran);
}

__global__ __launch_bounds__(64 * kReduceFrames) void cape_pose_cov_reduce_kernel(PoseCovParams p, int nFrames)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frame = blockIdx.x * kReduceFrames + wave;
    if (frame >= nFrames) // (a whole wave; no barrier in this kernel)
        return;
    const PoseCovFrame& F = p.frames[frame];
    const PoseCovSample* samples = p.samples + (size_t)frame * (size_t)p.nIterations;
    const int entry = lane < 36 ? lane : 35, er = entry / 6, ec = entry % 6;
    PoseCovCounts counts;
    counts.nOk = 0, counts.nfevMin = 0, counts.nfevMax = 0, counts.nfevSum = 0;
    int status = F.refusal;
    double mine = 0.0, meanR = 0.0;
    if (status == 0)
    {
        counts = pose_cov_counts(samples, p.nIterations);
        if (pose_cov_too_many_failed(counts.nOk, p.nIterations))
            status = CAPE_POSE_COVARIANCE_TOO_MANY_FAILED;
        else
        {
            meanR = pose_cov_mean(samples, p.nIterations, er, counts.nOk);
            const double meanC = pose_cov_mean(samples, p.nIterations, ec, counts.nOk);
            mine = pose_cov_entry(samples, p.nIterations, er, ec, meanR, meanC, counts.nOk);
        }
    }
    // every lane gets the 36 entries (all 64 lanes of the wave are here: the status is the frame's)
    double cov[36];
#pragma unroll
    for (int e = 0; e < 36; ++e)
        cov[e] = __shfl(mine, e);
    if (status == 0)
        status = is_covariance_valid<6>(cov) ? (int)CAPE_POSE_COVARIANCE_VALID : (int)CAPE_POSE_COVARIANCE_INVALID;
    double* out = reinterpret_cast<double*>(p.rows + frame);
    if (lane < 36)
        out[6 + lane] = mine;
    if (lane % 7 == 0 && lane < 36) // the diagonal lanes hold the means: lane 7 c has er = ec = c
        out[er] = meanR;
    if (lane == 0)
    {
        uint4* tail = reinterpret_cast<uint4*>(out + 42);
        tail[0] = make_uint4((unsigned)counts.nOk, (unsigned)p.nIterations, (unsigned)status,
                             (F.frameFlags & (uint32_t)CAPE_MATCH_EXACT_OVERFLOW) | (F.nInvalid > 0 ? (uint32_t)CAPE_POSE_SCORE_INVALID_FEATURE : 0u));
        tail[1] = make_uint4((unsigned)counts.nfevMin, (unsigned)counts.nfevMax, (unsigned)(unsigned long long)counts.nfevSum,
                             (unsigned)((unsigned long long)counts.nfevSum >> 32));
    }
}

__global__ __launch_bounds__(256) void cape_pose_draw_kernel(uint64_t seed, uint32_t frameIndex, int nIterations, int uniforms, double* out)
{
    // a lane per (iteration, pair slot): four consecutive doubles
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)nIterations * WP)
        return;
    double u[4], z[4];
    pose_deviate_uniforms(seed, frameIndex, (uint32_t)(at / WP), (uint32_t)(at % WP), u);
    pose_deviate_normals(u, z);
#pragma unroll
    for (int c = 0; c < 4; ++c)
        out[at * 4 + c] = uniforms ? u[c] : z[c];
}

hipError_t launch_map_pose_covariance_chunk(const PoseCovParams& p, hipStream_t stream)
{
    const int groups = (p.nIterations + kPoseCovGroupIterations - 1) / kPoseCovGroupIterations;
    hipLaunchKernelGGL(cape_pose_vary_kernel, dim3(p.chunkFrames, groups), dim3(kPoseCovGroupIterations), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(cape_pose_solve_varied_kernel, dim3(p.chunkFrames, groups), dim3(kPoseCovGroupIterations), pose_rows_layout().bytes, stream, p);
    return hipGetLastError();
}

hipError_t launch_map_pose_covariance_reduce(const PoseCovParams& p, int nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_pose_cov_reduce_kernel, dim3((nFrames + kReduceFrames - 1) / kReduceFrames), dim3(64 * kReduceFrames), 0, stream, p, nFrames);
    return hipGetLastError();
}

hipError_t launch_pose_draw_deviates(uint64_t seed, uint32_t frameIndex, int nIterations, bool uniforms, double* out, hipStream_t stream)
{
    const size_t lanes = (size_t)nIterations * WP;
    hipLaunchKernelGGL(cape_pose_draw_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, seed, frameIndex, nIterations,
                       uniforms ? 1 : 0, out);
    return hipGetLastError();
}

} // namespace cape

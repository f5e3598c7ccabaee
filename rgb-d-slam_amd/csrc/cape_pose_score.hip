// cape_map_pose_score: the plane cost function of the pose solver (PlaneOptimizationFeature, map_primitive.cpp:15-85) for a batch of
// pose hypotheses per frame, on the match of the last cape_match_map_wide, the front map and its tracks.  The statements are those of
// cape_pose_score.h, which the host twin cape_host_pose_score compiles too.  Two kernels: the pairs kernel writes the pose stage's shared
// pair rows, for this call and for the solve and the covariance behind it, and runs only where they are not current (enqueue_pose_pairs,
// cape_api_pose.h); the score kernel writes only the call's own result buffers.
//
//   cape_pose_pairs_kernel : one wavefront per frame, four per workgroup, no barrier, no LDS.
//        Lanes over the map planes 64 at a time: lane l reads match[f][chunk + l]; a ballot and a count of the bits below the lane
//        (pose_pair_slot) give the pair's place k in the ordered list; the lane resolves kept plane i through the wide match's table
//        to (record, segment) -- both checked against the record buffer -- and writes feature row k: one writer per row.  Rows at and
//        beyond n_pairs are zeroed by lanes k and k + 64 afterwards.  Lane 0 writes the frame's (n_pairs, n_invalid, flags).
//   cape_pose_score_kernel : one lane per hypothesis, one workgroup of four waves per (frame, 256 hypotheses).
//        The frame's feature rows -- the two planes and the kept plane, 68 of a row's 112 bytes -- are copied to LDS once per
//        workgroup, then every lane walks the pairs in order: plane_to_camera of the map plane under its own pose, the distances, the
//        sums.  LDS rather than scalar-cache loads: every lane of a wave reads the same row, which the LDS serves as a broadcast
//        without a bank conflict, and the copy is explicit -- scalar loads would need the compiler to prove both that the address is
//        wave-uniform and that nothing writes the rows while the kernel runs, and fall back to 64 identical vector loads per value
//        where it cannot.  8.5 KB of LDS per workgroup limit nothing: the registers of the double-precision sin / cos / atan2 do.
//        Every sum is lane-private and taken in pair order: no cross-lane reduction, no atomic, and no result depends on which other
//        hypotheses share the wave.  Idle lanes of the last workgroup store nothing.  No indexed private array: no scratch.
//
// With few hypotheses per frame most lanes of the score kernel idle (n_hypotheses = 1: one lane in 256 works); accepted here, the
// measured rates are in DESIGN.md 4.6.  Everything but the three atan2(sin, cos) values per pair is + - x / sqrt in the order of the
// host twin (-ffp-contract=off) and equals it bit for bit; sin, cos and atan2 are ocml's.
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_layout.h"
#include "cape_map_camera.h"
#include "cape_map_commit.h"
#include "cape_pose_solve.h" // (the carve and the staging of the rows, shared with the solve kernels)

namespace cape {

namespace {

constexpr int kPairsFrames = 4; // frames (waves) of a pairs workgroup
constexpr int WP = kPoseScoreMaxPairs;
static_assert(WP == 128, "a lane zeroes rows k and k + 64");
static_assert(sizeof(cape_pose_score) == 48 && sizeof(cape_pose_feature) == 112, "the layouts of include/cape_hip.h");
static_assert(sizeof(cape_pose_score) % 16 == 0 && sizeof(cape_pose_feature) % 16 == 0, "16-byte stores");

} // namespace

__global__ __launch_bounds__(64 * kPairsFrames) void cape_pose_pairs_kernel(PosePairsParams p, int nFrames)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frame = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kPairsFrames + wave));
    if (frame >= nFrames) // (idle waves of the last workgroup; the kernel has no barrier)
        return;
    const cape_frame_map_match_wide hd = p.matchFrames[frame];
    const bool reports = !(hd.flags & CAPE_MATCH_EXACT_OVERFLOW);
    const int nMap = reports ? p.nMap : 0;
    const int nCur = hd.n_cur < 0 ? 0 : (hd.n_cur > WP ? WP : hd.n_cur);
    const int32_t* match = p.match + (size_t)frame * p.nMap;
    const uint2* kept = p.kept + (size_t)frame * WP;
    cape_pose_feature* rows = p.features + (size_t)frame * WP;
    int nPairs = 0, nInvalid = 0; // (wave-uniform: they come out of ballots)
    for (int jb = 0; jb < nMap; jb += 64)
    {
        const int j = jb + lane;
        const int i = j < nMap ? match[j] : -1;
        const bool pair = pose_is_pair(i) && i < nCur;
        const unsigned long long ballot = __ballot(pair);
        const int k = pose_pair_slot(ballot, lane, nPairs);
        bool invalid = false;
        if (pair && k < WP)
        {
            cape_pose_feature F;
            // kept plane i's segment, through the wide match's table: (record, segment in that record)
            const uint2 at = kept[i];
            if (at.x < (unsigned)p.nRecords && at.y < (unsigned)CAPE_MAX_PLANES)
            {
                const cape_plane_segment& S = p.records[at.x].segments[at.y];
                F.matched[0] = S.out_normal[0], F.matched[1] = S.out_normal[1], F.matched[2] = S.out_normal[2], F.matched[3] = S.d;
            }
            else
                F.matched[0] = F.matched[1] = F.matched[2] = F.matched[3] = __builtin_nan(""); // (no such segment: an invalid feature)
            const cape_map_plane& M = p.mapPlanes[j];
            F.map_plane[0] = M.normal[0], F.map_plane[1] = M.normal[1], F.map_plane[2] = M.normal[2], F.map_plane[3] = M.d;
            pose_feature_stddev(p.tracks[j].covariance, F.stddev);
            F.map_id = p.tags[j].id;
            F.map_index = j;
            F.kept_plane = i;
            invalid = !pose_feature_valid(F);
            rows[k] = F;
        }
        nInvalid += __popcll(__ballot(invalid));
        nPairs += __popcll(ballot);
    }
    nPairs = nPairs < WP ? nPairs : WP;
#pragma unroll
    for (int s = 0; s < 2; ++s)
    {
        const int k = lane + 64 * s;
        if (k >= nPairs)
            rows[k] = cape_pose_feature{};
    }
    if (lane == 0)
        p.frameInfo[frame] = make_int4(nPairs, nInvalid, (int)(hd.flags & CAPE_MATCH_EXACT_OVERFLOW), 0);
}

__global__ __launch_bounds__(kPoseScoreGroupHypotheses) void cape_pose_score_kernel(PoseScoreParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int frame = blockIdx.x;
    const int hyp = blockIdx.y * kPoseScoreGroupHypotheses + threadIdx.x; // the workgroup's offset, then the lane
    const int4 info = p.frameInfo[frame];
    const int nPairs = info.x < WP ? info.x : WP;
    double* s_planes;
    int* s_kept;
    pose_rows_stage(smem, p.features + (size_t)frame * WP, nPairs, s_planes, s_kept);
    if (hyp >= p.nHypotheses) // (idle lanes of the frame's last workgroup store nothing)
        return;
    const size_t at = (size_t)frame * p.nHypotheses + hyp;
    double T[12];
#pragma unroll
    for (int c = 0; c < 12; ++c)
        T[c] = p.poses[at * 16 + c];
    PoseScoreSums S;
    double* residuals = p.residuals ? p.residuals + at * WP * 7 : nullptr;
#pragma unroll 1
    for (int k = 0; k < nPairs; ++k)
    {
        const double* row = s_planes + 8 * k;
        const double cn[3] = {row[0], row[1], row[2]}, cd = row[3];
        double qn[3], qd;
        plane_to_camera(T, row + 4, row[7], qn, qd);
        double signedDistance[4], reduced[3];
        pose_pair_distances(cn, cd, qn, qd, signedDistance, reduced);
        pose_score_add(S, s_kept[k], signedDistance, reduced);
        if (residuals)
        {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                residuals[7 * k + c] = signedDistance[c];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                residuals[7 * k + 4 + c] = reduced[c];
        }
    }
    const cape_pose_score r = pose_score_row(S, nPairs, info.y, (uint32_t)info.z);
    uint4* out = reinterpret_cast<uint4*>(p.scores + at);
    out[0] = make_uint4((unsigned)r.n_pairs, (unsigned)r.n_inliers, (unsigned)r.n_invalid, r.flags);
    out[1] = make_uint4((unsigned)__double2loint(r.score), (unsigned)__double2hiint(r.score), (unsigned)__double2loint(r.sum_sq), (unsigned)__double2hiint(r.sum_sq));
    out[2] = make_uint4(r.inlier_words[0], r.inlier_words[1], r.inlier_words[2], r.inlier_words[3]);
}

hipError_t launch_map_pose_pairs(const PosePairsParams& p, int nFrames, hipStream_t stream)
{
    hipLaunchKernelGGL(cape_pose_pairs_kernel, dim3((nFrames + kPairsFrames - 1) / kPairsFrames), dim3(64 * kPairsFrames), 0, stream, p, nFrames);
    return hipGetLastError();
}

hipError_t launch_map_pose_score(const PoseScoreParams& p, int nFrames, hipStream_t stream)
{
    const int groups = (p.nHypotheses + kPoseScoreGroupHypotheses - 1) / kPoseScoreGroupHypotheses;
    hipLaunchKernelGGL(cape_pose_score_kernel, dim3(nFrames, groups), dim3(kPoseScoreGroupHypotheses), pose_rows_layout().bytes, stream, p);
    return hipGetLastError();
}

} // namespace cape

// cape_map_pose_score: the plane cost function of the pose solver -- PlaneOptimizationFeature (map_primitive.cpp:15-85) -- as the rules
// one (frame, hypothesis, pair) follows.  A pair is a map plane j with match[f][j] = i >= 0; its feature row holds the detected plane
// (cn, cd) of kept plane i, the map plane and the track's standard deviations.  For a hypothesis T the map plane goes through
// plane_to_camera (cape_map_camera.h on the device, utils::plane_to_camera on the host: the caller of these functions does it) and
//
//   signed[c]  = atan2(sin(cn[c] - qn[c]), cos(cn[c] - qn[c])), c < 3    get_signed_distance (plane_coordinates.cpp:26-37) through
//   signed[3]  = cd - qd                                                  angle_distance (distance_utils.cpp:6-9): normal COMPONENTS
//                                                                         fed to an angle function, the reference's quirk
//   inlier     = |signed[c]| <= (double)0.2f for c < 3 and |signed[3]| <= (double)50.0f     (is_inlier, map_primitive.cpp:44-48;
//                                                                         parameters.hpp:27-30; a NaN compares false: an outlier)
//   reduced[c] = cd * cn[c] - qd * qn[c]                                  get_reduced_signed_distance (plane_coordinates.cpp:49-56)
//   r[c]       = reduced[c] * 1.0 / 3.0,  sum_sq += r[c] * r[c]           the LM functor: distance * get_alpha_reduction() / partCount
//   score     += 1.0 / 3 per inlier                                       get_score (map_primitive.cpp:27-31), pose_optimization.cpp:63
//
// in pair order k ascending, c ascending within k.  Everything but the three atan2(sin, cos) values is + - x / sqrt.
//
// Plain functions, so that the kernels (cape_pose_score.hip), the host twin cape_host_pose_score (host/pose_score.cpp) and
// tests/host/pose_score_pairs.cpp compile the same statements: with hipcc they are __host__ __device__, with any other compiler
// plain inline functions (no HIP header is needed then; one that is on the include path is taken).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CAPE_POSE_FN __host__ __device__ __forceinline__
#else
#if defined(__has_include)
#if __has_include(<hip/hip_runtime.h>)
#include <hip/hip_runtime.h>
#endif
#endif
#define CAPE_POSE_FN inline
#endif

#include "../../include/cape_hip.h"

namespace cape {

constexpr int kPoseScoreMaxPairs = CAPE_MATCH_MAP_WIDE_MAX_PLANES; // a frame's kept planes, each matched at most once
constexpr int kPoseScoreGroupHypotheses = 256;                     // hypotheses of a score workgroup: four waves, a lane each

// parameters::optimization (parameters.hpp:27-30): constexpr float there, widened to double where is_inlier compares
constexpr float kPoseInlierAngleThreshold = 0.2f;     // planeInlierAngleThreshold
constexpr float kPoseInlierDistanceThreshold = 50.0f; // planeInlierDistanceThreshold_mm

// ---- the pair list: map planes in ascending order whose match names a kept plane
CAPE_POSE_FN bool pose_is_pair(int32_t keptPlane) { return keptPlane >= 0 && keptPlane < kPoseScoreMaxPairs; }
// The pairs kernel takes the map planes 64 at a time, lane l the plane chunk + l: `ballot` has bit l set where lane l holds a pair,
// `base` is the number of pairs in the chunks before.  The slot of lane `lane`'s pair in the ordered list; a slot at or beyond
// kPoseScoreMaxPairs is not stored (a match table that names a kept plane twice: not one the wide match writes).
CAPE_POSE_FN int pose_pair_slot(unsigned long long ballot, int lane, int base)
{
    const unsigned long long below = ballot & ((1ull << lane) - 1ull);
    int c = 0;
    for (unsigned long long v = below; v; v &= v - 1)
        ++c;
    return base + c;
}
// the serial statement of the same list: pairs[k] = the k-th map plane with a pair; returns their number (at most kPoseScoreMaxPairs)
CAPE_POSE_FN int pose_pairs_serial(const int32_t* match, int nMap, int32_t* pairs)
{
    int n = 0;
    for (int j = 0; j < nMap; ++j)
        if (pose_is_pair(match[j]) && n < kPoseScoreMaxPairs)
            pairs[n++] = j;
    return n;
}

// ---- the feature row
// stddev[c] = sqrt(covariance[5 c]) of the track (the constructor argument of PlaneOptimizationFeature)
CAPE_POSE_FN void pose_feature_stddev(const double* covariance16, double stddev[4])
{
    for (int c = 0; c < 4; ++c)
        stddev[c] = sqrt(covariance16[5 * c]);
}
// is_valid (map_primitive.cpp:79-83): no NaN in the two planes, no NaN or negative standard deviation
CAPE_POSE_FN bool pose_feature_valid(const cape_pose_feature& F)
{
    bool ok = true;
    for (int c = 0; c < 4; ++c)
        ok = ok && !(F.matched[c] != F.matched[c]) && !(F.map_plane[c] != F.map_plane[c]) && F.stddev[c] >= 0.0; // (a NaN is not >= 0)
    return ok;
}

// ---- one pair under one hypothesis: (cn, cd) the detected plane, (qn, qd) the map plane in the hypothesis' camera
CAPE_POSE_FN double pose_angle_distance(double a, double b)
{
    const double diff = a - b;
    return atan2(sin(diff), cos(diff));
}
// get_reduced_signed_distance alone: what the LM functor reads of a pair (cape_pose_solve.h evaluates nothing else)
CAPE_POSE_FN void pose_pair_reduced(const double* cn, double cd, const double* qn, double qd, double reduced[3])
{
    for (int c = 0; c < 3; ++c)
        reduced[c] = cd * cn[c] - qd * qn[c];
}
CAPE_POSE_FN void pose_pair_distances(const double* cn, double cd, const double* qn, double qd, double signedDistance[4], double reduced[3])
{
    for (int c = 0; c < 3; ++c)
        signedDistance[c] = pose_angle_distance(cn[c], qn[c]);
    signedDistance[3] = cd - qd;
    pose_pair_reduced(cn, cd, qn, qd, reduced);
}
CAPE_POSE_FN bool pose_pair_inlier(const double signedDistance[4])
{
    const double angle = static_cast<double>(kPoseInlierAngleThreshold), distance = static_cast<double>(kPoseInlierDistanceThreshold);
    return fabs(signedDistance[0]) <= angle && fabs(signedDistance[1]) <= angle && fabs(signedDistance[2]) <= angle &&
           fabs(signedDistance[3]) <= distance;
}

// the sums of one (frame, hypothesis), carried over its pairs in order
struct PoseScoreSums
{
    int32_t nInliers = 0;
    double score = 0.0, sumSq = 0.0;
    unsigned long long inliersLo = 0ull, inliersHi = 0ull; // bit i: kept plane i (Lo), i + 64 (Hi) is matched and an inlier
};
CAPE_POSE_FN void pose_score_add(PoseScoreSums& S, int32_t keptPlane, const double signedDistance[4], const double reduced[3])
{
    for (int c = 0; c < 3; ++c)
    {
        const double r = reduced[c] * 1.0 / 3.0;
        S.sumSq += r * r;
    }
    if (pose_pair_inlier(signedDistance))
    {
        ++S.nInliers;
        S.score += 1.0 / 3;
        // (no indexed word: the kernel keeps the sums in registers)
        S.inliersLo |= keptPlane < 64 ? 1ull << (keptPlane & 63) : 0ull;
        S.inliersHi |= keptPlane < 64 ? 0ull : 1ull << (keptPlane & 63);
    }
}
CAPE_POSE_FN cape_pose_score pose_score_row(const PoseScoreSums& S, int32_t nPairs, int32_t nInvalid, uint32_t frameFlags)
{
    cape_pose_score r;
    r.n_pairs = nPairs;
    r.n_inliers = S.nInliers;
    r.n_invalid = nInvalid;
    r.flags = frameFlags | (nInvalid > 0 ? (uint32_t)CAPE_POSE_SCORE_INVALID_FEATURE : 0u);
    r.score = S.score;
    r.sum_sq = S.sumSq;
    r.inlier_words[0] = (uint32_t)S.inliersLo;
    r.inlier_words[1] = (uint32_t)(S.inliersLo >> 32);
    r.inlier_words[2] = (uint32_t)S.inliersHi;
    r.inlier_words[3] = (uint32_t)(S.inliersHi >> 32);
    return r;
}

#if defined(__HIPCC__)
// what the pairs kernel reads, and the pair rows it writes (cape_pose_score.hip)
struct PosePairsParams
{
    // the front map and its tracks
    const cape_map_plane* mapPlanes;
    const struct MapTrackState* tracks;
    const struct MapTrackTag* tags;
    int nMap;
    // the last cape_match_map_wide and the records its kept-plane table points into
    const cape_frame_map_match_wide* matchFrames;
    const int32_t* match; // frames x nMap
    const uint2* kept;    // frames x 128: (record, segment in that record) of kept plane i
    const cape_frame_record* records;
    int nRecords;
    // the pair rows
    int4* frameInfo;             // per frame: n_pairs, n_invalid, flags, 0
    cape_pose_feature* features; // frames x 128
};
// what the score kernel reads and writes
struct PoseScoreParams
{
    const int4* frameInfo;             // the pair rows
    const cape_pose_feature* features;
    const double* poses; // frames x hypotheses x 16
    int nHypotheses;
    cape_pose_score* scores; // frames x hypotheses
    double* residuals;       // frames x hypotheses x 128 x 7, or null
};
#endif

} // namespace cape

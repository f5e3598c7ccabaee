// cape_map_pose_covariance: compute_pose_variance (pose_optimization.cpp:361-437), the statement that follows a successful RANSAC -- every
// inlier feature varied by Gaussian noise of its map plane's standard deviations (PlaneOptimizationFeature::compute_random_variation,
// map_primitive.cpp:66-77), the LM run again from the optimised x on the varied set, the sample covariance of the resulting pose vectors
// plus 0.001 on the diagonal, is_covariance_valid -- as the rules ONE (frame, iteration) and ONE frame follow.  Plain functions like
// those of cape_pose_solve.h: the kernels (cape_pose_covariance.hip), the host twins cape_host_pose_covariance /
// cape_host_pose_draw_deviates (host/pose_covariance.cpp) and tests/host/pose_covariance_check.cpp compile the same statements.
//
//   deviates : Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11), key = the caller's 64-bit
//              seed (low word, high word), counter = (frame index + frame_base, iteration, pair slot, block).  Blocks 0 and 1 give eight
//              words; words (2 i, 2 i + 1) make the uniform u_i = ((w_2i << 32 | w_2i+1) >> 11) + 1) 2^-53 in (0, 1]; (u_0, u_1) and
//              (u_2, u_3) are two Box-Muller pairs: z = sqrt(-2 log u_a) (cos 2 pi u_b, sin 2 pi u_b).  A lane owns its deviates without
//              any state.  This is NOT the reference's stream (mt19937 behind std::normal_distribution inside a tbb::parallel_for).
//              log, cos and sin are the only statements of the variation that differ between ocml and glibc: a caller's table of deviates
//              (CAPE_POSE_COVARIANCE_TABLE) takes them out, and the device then equals the twin bit for bit up to the Euler angles.
//   variation: n' = n + z[0..2] * stddev[0..2]; s = (n'x^2 + n'y^2) + n'z^2; s > 0: n' / sqrt(s), a division per component (Eigen's
//              normalize()); d' = d + z[3] * stddev[3].  The matched plane and the standard deviations stay.
//   a sample : pose_solve_problem from the optimised x over the subset on the varied planes -- same guards, parameters and statuses; a
//              success iff status > 0 and the end x holds no NaN (pose_optimization.cpp:340-355).
//   the pose vector (PoseBase::get_vector, pose.hpp:31-36): x[0..2], then eulerAngles(0, 1, 2) of the rotation of the coefficients
//              (pose_rotation_from_coefficients: before the camera basis), Eigen 3.4's algorithm restated: three atan2, one sin, one
//              cos, the first angle folded into [0, pi].  The fold is the reference's own: samples that straddle a first angle of 0 land
//              near 0 and near pi.
//   reduction: over the successes in ascending iteration order: n_ok < iterations / 2 -> too many failed; mean = sum / n_ok;
//              cov(i, j) = sum (v_i - mean_i)(v_j - mean_j), / (n_ok - 1) -- NOT guarded: n_ok = 1 divides 0 by 0 and fails
//              is_covariance_valid on "invalid values", as the reference does --, + 0.001 on the diagonal, is_covariance_valid<6>.
#pragma once
#include "cape_pose_solve.h"

namespace cape {

constexpr int kPoseCovGroupIterations = kPoseSolveGroupProblems; // iterations of a workgroup of the varied solve: four waves, a lane each
constexpr double kPoseCovDiagonal = 0.001;                       // pose_optimization.cpp:421

// ---- Philox4x32-10
CAPE_POSE_FN void philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3], k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; ++round)
    {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}
// the four uniforms in (0, 1] of (frame, iteration, pair slot): exact in double, no rounding
CAPE_POSE_FN void pose_deviate_uniforms(uint64_t seed, uint32_t frame, uint32_t iteration, uint32_t slot, double u[4])
{
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    for (uint32_t block = 0; block < 2; ++block)
    {
        const uint32_t counter[4] = {frame, iteration, slot, block};
        uint32_t w[4];
        philox4x32_10(counter, key, w);
        u[2 * block] = ((double)((((uint64_t)w[0] << 32) | w[1]) >> 11) + 1.0) * 0x1p-53;
        u[2 * block + 1] = ((double)((((uint64_t)w[2] << 32) | w[3]) >> 11) + 1.0) * 0x1p-53;
    }
}
// ... and the four standard-normal deviates of them
CAPE_POSE_FN void pose_deviate_normals(const double u[4], double z[4])
{
    const double twoPi = 6.283185307179586476925286766559;
    for (int b = 0; b < 2; ++b)
    {
        const double radius = sqrt(-2.0 * log(u[2 * b])), angle = twoPi * u[2 * b + 1];
        z[2 * b] = radius * cos(angle);
        z[2 * b + 1] = radius * sin(angle);
    }
}

// ---- the variation of a pair's map plane
CAPE_POSE_FN void pose_vary_plane(const double mapPlane[4], const double stddev[4], const double z[4], double out[4])
{
    double nx = mapPlane[0] + z[0] * stddev[0], ny = mapPlane[1] + z[1] * stddev[1], nz = mapPlane[2] + z[2] * stddev[2];
    const double s = (nx * nx + ny * ny) + nz * nz;
    if (s > 0.0)
    {
        const double norm = sqrt(s);
        nx = nx / norm, ny = ny / norm, nz = nz / norm;
    }
    out[0] = nx, out[1] = ny, out[2] = nz;
    out[3] = mapPlane[3] + z[3] * stddev[3];
}

// ---- a sample's rows: the frame's rows with the lane's own varied map planes, [pair][component] at `stride` doubles (the slab keeps
// the iteration as its fastest index: the lanes of a wave, an iteration each, read consecutive addresses)
struct PoseVariedRows : PoseSolveRows
{
    const double* varied; // the sample's first value: pair 0, component 0
    size_t stride;
    CAPE_POSE_FN const double* map_plane(int k, double* own) const
    {
        CAPE_POSE_UNROLL
        for (int c = 0; c < 4; ++c)
            own[c] = varied[(size_t)(4 * k + c) * stride];
        return own;
    }
};

// ---- Eigen 3.4's MatrixBase::eulerAngles(0, 1, 2) on the row-major R (EulerAngles.h: i = 0, j = 1, k = 2, an even permutation)
CAPE_POSE_FN void pose_euler_angles_012(const double R[9], double angles[3])
{
    const double pi = 3.1415926535897932384626433832795;
    double a0 = atan2(R[5], R[8]), a1; // coeff(j, k), coeff(k, k)
    const double c2 = sqrt(R[0] * R[0] + R[1] * R[1]); // Vector2(coeff(i, i), coeff(i, j)).norm()
    if (a0 > 0.0)
    {
        a0 = a0 - pi; // (a0 > 0 here: the other arm of Eigen's branch is for odd permutations)
        a1 = atan2(-R[2], -c2);
    }
    else
        a1 = atan2(-R[2], c2);
    const double s1 = sin(a0), c1 = cos(a0);
    const double a2 = atan2(s1 * R[6] - c1 * R[3], c1 * R[4] - s1 * R[7]);
    angles[0] = -a0, angles[1] = -a1, angles[2] = -a2; // the even permutation's sign: the first angle ends in [0, pi]
}
// PoseBase::get_vector of x
CAPE_POSE_FN void pose_vector(const double x[6], double v[6])
{
    double R[9];
    pose_rotation_from_coefficients(x, R);
    v[0] = x[0], v[1] = x[1], v[2] = x[2];
    pose_euler_angles_012(R, v + 3);
}

// ---- what the reduction reads of a sample: 64 bytes
struct PoseCovSample
{
    double v[6];
    int32_t status, nfev; // the sample's solution row
    int32_t ok;           // status > 0 and no NaN in the end x
    int32_t ran;          // 0: the frame was refused and the row was never written
};
CAPE_POSE_FN PoseCovSample pose_cov_sample(const cape_pose_solution& r)
{
    PoseCovSample s;
    bool nan = false;
    CAPE_POSE_UNROLL
    for (int c = 0; c < 6; ++c)
        nan = nan || r.x[c] != r.x[c];
    pose_vector(r.x, s.v);
    s.status = r.status, s.nfev = r.nfev;
    s.ok = (r.status > 0 && !nan) ? 1 : 0;
    s.ran = 1;
    return s;
}

// ---- one frame's x, subset and refusal, resolved once in front of its samples (the vary kernel's first lane; the twin)
struct PoseCovFrame
{
    double x[6];
    uint32_t words[4];
    int32_t refusal; // 0: the samples run; else the row's status
    int32_t nPairs, nInvalid;
    uint32_t frameFlags;
};
// solution / selection: CAPE_POSE_COVARIANCE_FROM_SOLUTION's rows of the frame, or null with x and words given
CAPE_POSE_FN PoseCovFrame pose_cov_frame(const PoseSolveRows& frameRows, int nInvalid, uint32_t frameFlags, const double* x, const uint32_t* words,
                                         const cape_pose_solution* solution, const cape_pose_selection* selection)
{
    PoseCovFrame F;
    for (int c = 0; c < 6; ++c)
        F.x[c] = solution ? solution->x[c] : x[c];
    for (int c = 0; c < 4; ++c)
        F.words[c] = selection ? selection->inlier_words[c] : words[c];
    F.nPairs = frameRows.nPairs, F.nInvalid = nInvalid, F.frameFlags = frameFlags;
    PoseSolveRows rows = frameRows;
    pose_subset(F.words, rows.subsetLo, rows.subsetHi);
    int nUsed;
    F.refusal = pose_solve_refusal(rows, nInvalid, frameFlags, F.x, nUsed);
    if (solution && solution->status <= 0) // (the refit's own refusal, CAPE_POSE_SOLVE_NO_SELECTION among them, goes first)
        F.refusal = solution->status < 0 ? solution->status : (int32_t)CAPE_POSE_COVARIANCE_NO_SOLUTION;
    return F;
}

// ---- the reduction: every sum over the successes in ascending iteration order
struct PoseCovCounts
{
    int32_t nOk, nfevMin, nfevMax;
    int64_t nfevSum;
};
CAPE_POSE_FN PoseCovCounts pose_cov_counts(const PoseCovSample* samples, int nIterations)
{
    PoseCovCounts C;
    C.nOk = 0, C.nfevMin = 0, C.nfevMax = 0, C.nfevSum = 0;
    for (int i = 0; i < nIterations; ++i)
    {
        const int nfev = samples[i].nfev;
        C.nfevMin = (i == 0 || nfev < C.nfevMin) ? nfev : C.nfevMin;
        C.nfevMax = (i == 0 || nfev > C.nfevMax) ? nfev : C.nfevMax;
        C.nfevSum += nfev;
        C.nOk += samples[i].ok;
    }
    return C;
}
CAPE_POSE_FN double pose_cov_mean(const PoseCovSample* samples, int nIterations, int c, int nOk)
{
    double sum = 0.0;
    for (int i = 0; i < nIterations; ++i)
        if (samples[i].ok)
            sum += samples[i].v[c];
    return sum / static_cast<double>(nOk);
}
// covariance(r, c): meanR, meanC = pose_cov_mean of the two components
CAPE_POSE_FN double pose_cov_entry(const PoseCovSample* samples, int nIterations, int r, int c, double meanR, double meanC, int nOk)
{
    double sum = 0.0;
    for (int i = 0; i < nIterations; ++i)
        if (samples[i].ok)
            sum += (samples[i].v[r] - meanR) * (samples[i].v[c] - meanC);
    const double entry = sum / static_cast<double>(nOk - 1); // (n_ok = 1: 0 / 0, as in the reference)
    return r == c ? entry + kPoseCovDiagonal : entry;
}
CAPE_POSE_FN bool pose_cov_too_many_failed(int nOk, int nIterations) { return nOk < nIterations / 2; }
// the serial statement of a frame's row: what the reduce kernel's lanes compute an entry each.  valid(covariance36): is_covariance_valid<6>
template <class Valid>
CAPE_POSE_FN cape_pose_covariance pose_cov_row_serial(const PoseCovFrame& F, const PoseCovSample* samples, int nIterations, const Valid& valid)
{
    cape_pose_covariance row;
    for (int c = 0; c < 6; ++c)
        row.mean[c] = 0.0;
    for (int c = 0; c < 36; ++c)
        row.covariance[c] = 0.0;
    row.n_ok = 0, row.n_iterations = nIterations, row.status = F.refusal;
    row.flags = (F.frameFlags & (uint32_t)CAPE_MATCH_EXACT_OVERFLOW) | (F.nInvalid > 0 ? (uint32_t)CAPE_POSE_SCORE_INVALID_FEATURE : 0u);
    row.nfev_min = row.nfev_max = 0, row.nfev_sum = 0;
    if (F.refusal != 0)
        return row;
    const PoseCovCounts counts = pose_cov_counts(samples, nIterations);
    row.n_ok = counts.nOk, row.nfev_min = counts.nfevMin, row.nfev_max = counts.nfevMax, row.nfev_sum = counts.nfevSum;
    if (pose_cov_too_many_failed(counts.nOk, nIterations))
    {
        row.status = CAPE_POSE_COVARIANCE_TOO_MANY_FAILED;
        return row;
    }
    for (int c = 0; c < 6; ++c)
        row.mean[c] = pose_cov_mean(samples, nIterations, c, counts.nOk);
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c)
            row.covariance[6 * r + c] = pose_cov_entry(samples, nIterations, r, c, row.mean[r], row.mean[c], counts.nOk);
    row.status = valid(row.covariance) ? (int32_t)CAPE_POSE_COVARIANCE_VALID : (int32_t)CAPE_POSE_COVARIANCE_INVALID;
    return row;
}

#if defined(__HIPCC__)
// what the kernels of cape_pose_covariance.hip read and write
struct PoseCovParams
{
    const int4* frameInfo;             // per frame of the call: n_pairs, n_invalid, flags, 0 (the pairs kernel's)
    const cape_pose_feature* features; // frames x 128
    const double* x;                   // frames x 6, or null: from the solutions
    const uint32_t* subsets;           // frames x 4, or null: from the selection
    const cape_pose_solution* solutions;  // CAPE_POSE_COVARIANCE_FROM_SOLUTION: the refit's rows, one per frame
    const cape_pose_selection* selection; // ... and the selection they were refitted from
    const double* table;               // [iteration][128][4] deviates, or null: Philox
    uint64_t seed;
    uint32_t frameBase;
    int nIterations;
    int firstFrame, chunkFrames;       // the frames of this launch: the slab holds chunkFrames
    PoseSolveSettings settings;
    PoseCovFrame* frames;              // frames of the call
    double* slab;                      // [frame - firstFrame][128][4][iteration]
    int drawUniforms;                  // the draw kernel: the uniforms instead of the normals
    PoseCovSample* samples;            // [frame][iteration]
    cape_pose_solution* kept;          // frames x iterations, or null
    cape_pose_covariance* rows;        // frames
};
#endif

} // namespace cape

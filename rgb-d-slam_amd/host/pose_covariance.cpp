// cape_host_pose_covariance / cape_host_pose_draw_deviates (cape_host_map.h): the host twins of cape_map_pose_covariance and
// cape_pose_draw_deviates for ONE frame -- the pair list and the rows of pose_pairs.h, which cape_host_pose_score builds too, the frame's x, subset
// and refusal, the varied planes of every iteration in the device's slab layout [pair][component][iteration], every sample through
// pose_solve_problem and the reduction, all on the rules of csrc/cape_pose_covariance.h, which the kernels compile too.  Serial: iteration
// after iteration; a caller that wants frames side by side calls it from threads of its own.
#include <cstring>
#include <vector>

#include "boundary_polygon.hpp"
#include "map_tracking.hpp"
#include "pose_pairs.h"
#include "../csrc/cape_pose_covariance.h" // the rules, shared with the kernels

namespace {

struct HostPlaneToCamera
{
    void operator()(const double* T, const double* normal, double d, double qn[3], double& qd) const
    {
        rgbd_slam::utils::plane_to_camera(normal, d, T, qn, &qd);
    }
};
struct HostCovarianceValid
{
    bool operator()(const double* covariance36) const { return rgbd_slam::map_tracking::is_covariance_valid(covariance36, 6); }
};

} // namespace

extern "C" int cape_host_pose_covariance(const cape_host_map* map, const int32_t* match, const cape_host_planes* detected, uint32_t frame_flags,
                                         int32_t n_iterations, const double* x, const uint32_t* subset, const cape_pose_solution* solution,
                                         const cape_pose_selection* selection, const double* deviates, uint64_t seed, uint32_t frame_index,
                                         const cape_pose_solve_params* params, cape_pose_covariance* row_out, cape_pose_solution* samples_out,
                                         double* vectors_out)
{
    constexpr int WP = cape::kPoseScoreMaxPairs;
    cape::PoseSolveSettings settings;
    if (n_iterations < 1 || !cape::pose_solve_settings(params, settings))
        return CAPE_ERR_INVALID_ARGUMENT;
    if ((solution != nullptr) != (selection != nullptr) || (!solution && (!x || !subset)))
        return CAPE_ERR_INVALID_ARGUMENT;
    cape_host::PosePairs P;
    if (const int rc = cape_host::build_pose_pairs(map, match, detected, frame_flags, P); rc != CAPE_OK)
        return rc;
    const std::vector<cape_pose_feature>& features = P.features;
    const int nPairs = P.nPairs;
    cape::PoseSolveRows frameRows;
    frameRows.planes = P.planes.data(), frameRows.kept = P.kept.data(), frameRows.nPairs = nPairs, frameRows.subsetLo = frameRows.subsetHi = 0ull;
    const cape::PoseCovFrame F = cape::pose_cov_frame(frameRows, P.nInvalid, frame_flags & CAPE_MATCH_EXACT_OVERFLOW, x, subset, solution, selection);
    const size_t n = (size_t)n_iterations;
    std::vector<cape::PoseCovSample> samples(n);
    std::memset(samples.data(), 0, n * sizeof(cape::PoseCovSample));
    if (samples_out)
        std::memset(samples_out, 0, n * sizeof(cape_pose_solution));
    if (vectors_out)
        std::memset(vectors_out, 0, n * 6 * sizeof(double));
    if (F.refusal == 0)
    {
        cape::PoseVariedRows rows;
        static_cast<cape::PoseSolveRows&>(rows) = frameRows;
        cape::pose_subset(F.words, rows.subsetLo, rows.subsetHi);
        // ---- vary: the slab of the frame, [pair][component][iteration]
        std::vector<double> slab((size_t)WP * 4 * n);
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < nPairs; ++k)
            {
                if (!cape::pose_solve_takes(rows, k))
                    continue;
                double z[4], varied[4];
                if (deviates)
                    for (int c = 0; c < 4; ++c)
                        z[c] = deviates[(i * WP + (size_t)k) * 4 + c];
                else
                {
                    double u[4];
                    cape::pose_deviate_uniforms(seed, frame_index, (uint32_t)i, (uint32_t)k, u);
                    cape::pose_deviate_normals(u, z);
                }
                cape::pose_vary_plane(features[k].map_plane, features[k].stddev, z, varied);
                for (int c = 0; c < 4; ++c)
                    slab[(size_t)(4 * k + c) * n + i] = varied[c];
            }
        // ---- solve: a sample per iteration
        rows.stride = n;
        for (size_t i = 0; i < n; ++i)
        {
            rows.varied = slab.data() + i;
            double T[12];
            const cape_pose_solution r = cape::pose_solve_problem(rows, F.nInvalid, F.frameFlags, F.x, settings, HostPlaneToCamera{}, T);
            samples[i] = cape::pose_cov_sample(r);
            if (samples_out)
                samples_out[i] = r;
            if (vectors_out)
                std::memcpy(vectors_out + 6 * i, samples[i].v, 6 * sizeof(double));
        }
    }
    if (row_out)
        *row_out = cape::pose_cov_row_serial(F, samples.data(), n_iterations, HostCovarianceValid{});
    return CAPE_OK;
}

extern "C" int cape_host_pose_draw_deviates(uint64_t seed, uint32_t frame, int32_t n_iterations, double* out, uint32_t flags)
{
    constexpr int WP = cape::kPoseScoreMaxPairs;
    if (!out || n_iterations < 1 || (flags & ~(uint32_t)CAPE_POSE_DRAW_UNIFORMS))
        return CAPE_ERR_INVALID_ARGUMENT;
    for (int32_t i = 0; i < n_iterations; ++i)
        for (int k = 0; k < WP; ++k)
        {
            double u[4], z[4];
            cape::pose_deviate_uniforms(seed, frame, (uint32_t)i, (uint32_t)k, u);
            cape::pose_deviate_normals(u, z);
            std::memcpy(out + ((size_t)i * WP + (size_t)k) * 4, (flags & CAPE_POSE_DRAW_UNIFORMS) ? u : z, 4 * sizeof(double));
        }
    return CAPE_OK;
}

// ---- single statements of the rules header, for the tests
extern "C" void cape_host_philox4x32_10(const uint32_t* counter4, const uint32_t* key2, uint32_t* out4) { cape::philox4x32_10(counter4, key2, out4); }
extern "C" void cape_host_pose_vary_plane(const double* map_plane4, const double* stddev4, const double* z4, double* out4)
{
    cape::pose_vary_plane(map_plane4, stddev4, z4, out4);
}
extern "C" void cape_host_pose_vector(const double* x6, double* vector6_out, double* rotation9_out)
{
    cape::pose_vector(x6, vector6_out);
    if (rotation9_out)
        cape::pose_rotation_from_coefficients(x6, rotation9_out);
}
extern "C" void cape_host_euler_angles_012(const double* rotation9, double* angles3_out) { cape::pose_euler_angles_012(rotation9, angles3_out); }

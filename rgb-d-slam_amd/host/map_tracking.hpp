// Covariance and Kalman algebra of a map plane's update (MapPlane::update_with_match, map_primitive.cpp:204-251): the statements
// of the reference's Eigen expressions with their summation order written out, so that a device restatement can follow them
// one for one.  Compiled with -ffp-contract=off like the rest of the host code.
//   compute_plane_covariance                   utils/covariances.cpp:96-150
//   compute_reduced_plane_point_cloud_covariance :152-186
//   get_world_plane_covariance                 :188-226
//   is_covariance_valid / propagate_covariance utils/covariances.hpp:14-64
//   SharedKalmanFilter<4,4>::get_new_state     tracking/kalman_filter.hpp (identity dynamics and output, process noise 1e-6 I)
// Matrices are row-major arrays of doubles.  Third-party choices that the reference leaves to Eigen and that are restated here:
// the order of every sum (left to right), the LDLT of the validity check (Eigen's unblocked pivoting LDLT, inner products left
// to right), and the 4 x 4 inverse / determinant (a fixed cofactor formula over 2 x 2 minors, not Eigen's).
#pragma once
#include <cstdint>

namespace rgbd_slam::map_tracking {

// Eigen::isApprox on N x N (Frobenius) and is_covariance_valid: finite, isApprox(transpose), LDLT of the upper triangle isPositive
constexpr int kMaxCovarianceSize = 6; // 3: a pose's position block; 4: a plane; 6: a pose (cape_host_pose_covariance)
bool is_covariance_valid(const double* M, int n) noexcept;

// PlaneCoordinates(vector4) / operator=: the normal normalised (once per call), d as is
void normalize3(double* n) noexcept;
double norm3(const double* n) noexcept;

// PlaneCameraCoordinates::to_world_coordinates through compute_plane_camera_to_world_matrix (camera_transformation.cpp:53-61):
// [R 0; -t^T R 1] * (n, d), then the PlaneWorldCoordinates constructor's normalisation.  T: cameraToWorld, 16 doubles row-major.
void plane_to_world(const double* normal, double d, const double* T, double* normalOut, double* dOut) noexcept;

// The functions below return false where the reference throws (or is_covariance_valid fails on its path).
bool plane_covariance(const double* normal, double d, const double* pointCloudCov9, double* out16) noexcept;
bool reduced_point_cloud_covariance(const double* normal, double d, const double* planeCov16, double* out9) noexcept;
bool world_plane_covariance(const double* normal, double d, const double* T, const double* planeCov16, const double* poseCov9,
                            double* out16) noexcept;

// 4 x 4 determinant and inverse by cofactors of 2 x 2 minors
double det44(const double* M) noexcept;
void inverse44(const double* M, double det, double* out) noexcept;

enum KalmanStatus
{
    KALMAN_OK = 0,
    KALMAN_INVALID_INPUT = 1, // a state or measurement covariance is not valid (the reference throws invalid_argument)
    KALMAN_SINGULAR = 2,      // innovation determinant 0 within DBL_EPSILON: the reference takes a pseudo-inverse, not restated
    KALMAN_INVALID_OUTPUT = 3 // the new covariance is not valid (the reference throws logic_error)
};
// get_new_state: x, z: 4 doubles; P, R: 4 x 4.  Writes xOut / Pout only on KALMAN_OK.
KalmanStatus kalman_update(const double* x, const double* P, const double* z, const double* R, double* xOut, double* Pout) noexcept;

} // namespace rgbd_slam::map_tracking

// The covariance algebra of the map update's measurement half on the device: host/map_tracking.cpp restated one function for one,
// every sum left to right over its index, under the library's -ffp-contract=off.  Shared by the measurement kernel
// (cape_map_measure.hip) and the debug entry (cape_debug.hip); both files compile their own copy (anonymous namespace; no device
// symbol crosses a file).
//
// Everything is templated on the matrix size and every loop has a compile-time trip count (a bound that depends on the elimination
// step is a predicate inside a full-length loop), so that after unrolling every array index is a constant and the matrices live in
// registers.  The LDLT's pivot is known at run time only: the exchange is written once per candidate row b under `big == b`, with
// the constant indices k and b -- compares and selects over named elements, no array indexed by the pivot, no scratch memory.
//
// One statement is NOT the host's bit for bit: plane_covariance calls pow(s, 3 / 2), here ocml's, there glibc's, neither correctly
// rounded.  What follows it -- both 4 x 4 covariances -- is compared with a tolerance (tests/test_gpu_map_measure.py); the validity
// decisions on the inputs, the world plane and the polygon frame are the host's exactly.
#pragma once
#include <hip/hip_runtime.h>

#include "cape_internal.h"
#include "cape_map_camera.h"

namespace cape {

namespace {

constexpr double kDblEpsilon = 2.220446049250313e-16; // std::numeric_limits<double>::epsilon()
__device__ __forceinline__ bool double_equal(double a, double b) { return fabs(a - b) <= kDblEpsilon; }

// the lower triangle mirrored: Eigen's selfadjointView<Lower>() read as a full matrix
template <int N> __device__ __forceinline__ double sym_lower(const double* S, int i, int j) { return i >= j ? S[i * N + j] : S[j * N + i]; }

// propagate_covariance (covariances.hpp:55-64): (J * S.selfadjointView<Lower>() * J^T).selfadjointView<Lower>() + eps I.
// S: N x N, J: MR x N, out: MR x MR.
template <int N, int MR> __device__ __forceinline__ void propagate(const double* S, const double* J, double eps, double* out)
{
    double T[MR * N];
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int k = 0; k < N; ++k)
        {
            double s = J[i * N] * sym_lower<N>(S, 0, k);
#pragma unroll
            for (int l = 1; l < N; ++l)
                s = s + J[i * N + l] * sym_lower<N>(S, l, k);
            T[i * N + k] = s;
        }
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < MR; ++j)
            if (j <= i)
            {
                double s = T[i * N] * J[j * N];
#pragma unroll
                for (int k = 1; k < N; ++k)
                    s = s + T[i * N + k] * J[j * N + k];
                out[i * MR + j] = s;
                out[j * MR + i] = s;
            }
#pragma unroll
    for (int i = 0; i < MR; ++i)
        out[i * MR + i] = out[i * MR + i] + eps;
}

// is_covariance_valid (covariances.hpp): finite, M.isApprox(M^T), and selfadjointView<Upper>().ldlt() succeeds and is positive
template <int N> __device__ __forceinline__ bool is_covariance_valid(const double* M)
{
    bool finite = true;
#pragma unroll
    for (int i = 0; i < N * N; ++i)
        finite = finite && isfinite(M[i]); // "invalid values"
    if (!finite)
        return false;
    // M.isApprox(M^T): |M - M^T|^2 <= prec^2 min(|M|^2, |M^T|^2), Frobenius, prec = dummy_precision
    double diff = 0.0, a = 0.0, b = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j)
        {
            const double e = M[i * N + j] - M[j * N + i];
            diff = diff + e * e;
            a = a + M[i * N + j] * M[i * N + j];
            b = b + M[j * N + i] * M[j * N + i];
        }
    const double prec = 1e-12;
    if (!(diff <= prec * prec * (b < a ? b : a)))
        return false; // "not symetrical"
    // Eigen's unblocked LDLT with diagonal pivoting on the transpose's lower triangle
    double m[N * N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j)
            m[i * N + j] = M[j * N + i];
    enum
    {
        ZERO,
        POSITIVE,
        NEGATIVE,
        INDEFINITE
    };
    int sign = ZERO;
    // (zeroFirst: the host leaves the loop at a zero first pivot with ok = false; the steps after it run here on values nobody reads)
    bool ok = true, foundZeroPivot = false, zeroFirst = false;
    double temp[N];
#pragma unroll
    for (int i = 0; i < N; ++i)
        temp[i] = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k)
    {
        int big = k;
        double bigAbs = fabs(m[k * N + k]);
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (i > k && fabs(m[i * N + i]) > bigAbs)
            {
                big = i;
                bigAbs = fabs(m[i * N + i]);
            }
#pragma unroll
        for (int bb = 0; bb < N; ++bb)
            if (bb > k && big == bb)
            {
#pragma unroll
                for (int j = 0; j < N; ++j)
                    if (j < k)
                    {
                        const double t = m[k * N + j];
                        m[k * N + j] = m[bb * N + j];
                        m[bb * N + j] = t;
                    }
#pragma unroll
                for (int r = 0; r < N; ++r)
                    if (r > bb)
                    {
                        const double t = m[r * N + k];
                        m[r * N + k] = m[r * N + bb];
                        m[r * N + bb] = t;
                    }
                {
                    const double t = m[k * N + k];
                    m[k * N + k] = m[bb * N + bb];
                    m[bb * N + bb] = t;
                }
#pragma unroll
                for (int i = 0; i < N; ++i)
                    if (i > k && i < bb)
                    {
                        const double t = m[i * N + k];
                        m[i * N + k] = m[bb * N + i];
                        m[bb * N + i] = t;
                    }
            }
        if (k > 0)
        {
#pragma unroll
            for (int i = 0; i < N; ++i)
                if (i < k)
                    temp[i] = m[i * N + i] * m[k * N + i];
            double s = m[k * N] * temp[0];
#pragma unroll
            for (int i = 1; i < N; ++i)
                if (i < k)
                    s = s + m[k * N + i] * temp[i];
            m[k * N + k] = m[k * N + k] - s;
#pragma unroll
            for (int r = 0; r < N; ++r)
                if (r > k)
                {
                    double t = m[r * N] * temp[0];
#pragma unroll
                    for (int i = 1; i < N; ++i)
                        if (i < k)
                            t = t + m[r * N + i] * temp[i];
                    m[r * N + k] = m[r * N + k] - t;
                }
        }
        const double akk = m[k * N + k];
        const bool pivotValid = fabs(akk) > 0.0;
        if (k == 0 && !pivotValid)
            zeroFirst = true;
        if (k < N - 1)
        {
            if (pivotValid)
            {
#pragma unroll
                for (int r = 0; r < N; ++r)
                    if (r > k)
                        m[r * N + k] = m[r * N + k] / akk;
            }
            else
            {
#pragma unroll
                for (int r = 0; r < N; ++r)
                    if (r > k)
                        ok = ok && m[r * N + k] == 0.0;
            }
        }
        if (foundZeroPivot && pivotValid)
            ok = false;
        else if (!pivotValid)
            foundZeroPivot = true;
        if (sign == POSITIVE)
        {
            if (akk < 0.0)
                sign = INDEFINITE;
        }
        else if (sign == NEGATIVE)
        {
            if (akk > 0.0)
                sign = INDEFINITE;
        }
        else if (sign == ZERO)
        {
            if (akk > 0.0)
                sign = POSITIVE;
            else if (akk < 0.0)
                sign = NEGATIVE;
        }
    }
    return !zeroFirst && ok && (sign == POSITIVE || sign == ZERO); // info() == Success and isPositive()
}

__device__ __forceinline__ double norm3(const double* n) { return sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]); }

__device__ __forceinline__ void normalize3(double* n)
{
    const double z = norm3(n);
    if (z > 0)
    {
        n[0] = n[0] / z;
        n[1] = n[1] / z;
        n[2] = n[2] / z;
    }
}

// the plane matrix of a camera-to-world transform is built like that of a world-to-camera one
__device__ __forceinline__ void plane_to_world(const double* normal, double d, const double* T, double* normalOut, double& dOut)
{
    plane_to_camera(T, normal, d, normalOut, dOut);
}

__device__ __forceinline__ bool plane_covariance(const double* normal, double d, const double* pointCloudCov9, double* out16)
{
    if (!is_covariance_valid<3>(pointCloudCov9))
        return false;
    if (double_equal(d, 0.0) || !double_equal(norm3(normal), 1.0))
        return false;
    const double a = normal[0] * d, b = normal[1] * d, c = normal[2] * d;
    const double aSquared = a * a, bSquared = b * b, cSquared = c * c;
    const double divider = pow(aSquared + bSquared + cSquared, 3.0 / 2.0); // (ocml's pow: see the header comment)
    const double common = 1.0 / sqrt(aSquared + bSquared + cSquared);
    const double J[12] = {common - aSquared / divider, -(a * b) / divider,          -(a * c) / divider,
                          -(a * b) / divider,          common - bSquared / divider, -(b * c) / divider,
                          -(a * c) / divider,          -(b * c) / divider,          common - cSquared / divider,
                          -a / divider,                -b / divider,                -c / divider};
    propagate<3, 4>(pointCloudCov9, J, 0.01, out16);
    return is_covariance_valid<4>(out16);
}

__device__ __forceinline__ bool reduced_point_cloud_covariance(const double* normal, double d, const double* planeCov16, double* out9)
{
    if (!is_covariance_valid<4>(planeCov16))
        return false;
    if (double_equal(d, 0.0) || !double_equal(norm3(normal), 1.0))
        return false;
    const double J[12] = {d, 0, 0, normal[0], 0, d, 0, normal[1], 0, 0, d, normal[2]};
    propagate<4, 3>(planeCov16, J, 0.01, out9);
    return is_covariance_valid<3>(out9);
}

__device__ __forceinline__ bool world_plane_covariance(const double* normal, double d, const double* T, const double* planeCov16,
                                                       const double* poseCov9, double* out16)
{
    if (!is_covariance_valid<4>(planeCov16))
        return false;
    double pcc[9];
    if (!reduced_point_cloud_covariance(normal, d, planeCov16, pcc))
        return false;
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    double world[9];
    propagate<3, 3>(pcc, R, 0.0, world);
#pragma unroll
    for (int i = 0; i < 9; ++i)
        world[i] = world[i] + poseCov9[i];
    if (!is_covariance_valid<3>(world))
        return false;
    double nw[3], dw;
    plane_to_world(normal, d, T, nw, dw);
    return plane_covariance(nw, dw, world, out16);
}

// ---- the state half (cape_map_kalman.hip): no pow on this path, every function below is the host's bit for bit

// 4 x 4 determinant and inverse by cofactors of 2 x 2 minors (map_tracking.cpp:226-258)
__device__ __forceinline__ double det44(const double* a)
{
    const double s0 = a[0] * a[5] - a[4] * a[1], s1 = a[0] * a[6] - a[4] * a[2], s2 = a[0] * a[7] - a[4] * a[3];
    const double s3 = a[1] * a[6] - a[5] * a[2], s4 = a[1] * a[7] - a[5] * a[3], s5 = a[2] * a[7] - a[6] * a[3];
    const double c5 = a[10] * a[15] - a[14] * a[11], c4 = a[9] * a[15] - a[13] * a[11], c3 = a[9] * a[14] - a[13] * a[10];
    const double c2 = a[8] * a[15] - a[12] * a[11], c1 = a[8] * a[14] - a[12] * a[10], c0 = a[8] * a[13] - a[12] * a[9];
    return s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
}

__device__ __forceinline__ void inverse44(const double* a, double det, double* b)
{
    const double s0 = a[0] * a[5] - a[4] * a[1], s1 = a[0] * a[6] - a[4] * a[2], s2 = a[0] * a[7] - a[4] * a[3];
    const double s3 = a[1] * a[6] - a[5] * a[2], s4 = a[1] * a[7] - a[5] * a[3], s5 = a[2] * a[7] - a[6] * a[3];
    const double c5 = a[10] * a[15] - a[14] * a[11], c4 = a[9] * a[15] - a[13] * a[11], c3 = a[9] * a[14] - a[13] * a[10];
    const double c2 = a[8] * a[15] - a[12] * a[11], c1 = a[8] * a[14] - a[12] * a[10], c0 = a[8] * a[13] - a[12] * a[9];
    const double inv = 1.0 / det;
    b[0] = (a[5] * c5 - a[6] * c4 + a[7] * c3) * inv;
    b[1] = (-a[1] * c5 + a[2] * c4 - a[3] * c3) * inv;
    b[2] = (a[13] * s5 - a[14] * s4 + a[15] * s3) * inv;
    b[3] = (-a[9] * s5 + a[10] * s4 - a[11] * s3) * inv;
    b[4] = (-a[4] * c5 + a[6] * c2 - a[7] * c1) * inv;
    b[5] = (a[0] * c5 - a[2] * c2 + a[3] * c1) * inv;
    b[6] = (-a[12] * s5 + a[14] * s2 - a[15] * s1) * inv;
    b[7] = (a[8] * s5 - a[10] * s2 + a[11] * s1) * inv;
    b[8] = (a[4] * c4 - a[5] * c2 + a[7] * c0) * inv;
    b[9] = (-a[0] * c4 + a[1] * c2 - a[3] * c0) * inv;
    b[10] = (a[12] * s4 - a[13] * s2 + a[15] * s0) * inv;
    b[11] = (-a[8] * s4 + a[9] * s2 - a[11] * s0) * inv;
    b[12] = (-a[4] * c3 + a[5] * c1 - a[6] * c0) * inv;
    b[13] = (a[0] * c3 - a[1] * c1 + a[2] * c0) * inv;
    b[14] = (-a[12] * s3 + a[13] * s1 - a[14] * s0) * inv;
    b[15] = (a[8] * s3 - a[9] * s1 + a[10] * s0) * inv;
}

// KalmanStatus of host/map_tracking.hpp
enum
{
    kKalmanOk = 0,
    kKalmanInvalidInput = 1,
    kKalmanSingular = 2,
    kKalmanInvalidOutput = 3
};

// kalman_update (map_tracking.cpp:260-314): SharedKalmanFilter<4, 4>::get_new_state with identity dynamics and output, process noise
// 1e-6 I.  Writes xOut / Pout only on kKalmanOk.
__device__ __forceinline__ int kalman_update(const double* x, const double* P, const double* z, const double* R, double* xOut, double* Pout)
{
    if (!is_covariance_valid<4>(P) || !is_covariance_valid<4>(R))
        return kKalmanInvalidInput;
    const double processNoise = 0.000001;
    // estimateErrorCovariance = propagate(P, I) + 1e-6 I; innovation = propagate(that, I) + R
    double E[16], S[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            E[i * 4 + j] = sym_lower<4>(P, i, j) + (i == j ? processNoise : 0.0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            S[i * 4 + j] = sym_lower<4>(E, i, j) + R[i * 4 + j];
    const double det = det44(S);
    if (double_equal(det, 0.0))
        return kKalmanSingular;
    double Si[16], K[16];
    inverse44(S, det, Si);
    // kalmanGain = E.selfadjointView<Lower>() * I * S^-1
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            double s = sym_lower<4>(E, i, 0) * Si[j];
#pragma unroll
            for (int k = 1; k < 4; ++k)
                s = s + sym_lower<4>(E, i, k) * Si[k * 4 + j];
            K[i * 4 + j] = s;
        }
    double y[4], xn[4], C[16];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        y[k] = z[k] - x[k];
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        double s = K[i * 4] * y[0];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            s = s + K[i * 4 + k] * y[k];
        xn[i] = x[i] + s;
    }
    // (I - K) * E.selfadjointView<Lower>(), then its own selfadjointView<Lower>()
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j <= i)
            {
                double s = ((i == 0 ? 1.0 : 0.0) - K[i * 4]) * sym_lower<4>(E, 0, j);
#pragma unroll
                for (int k = 1; k < 4; ++k)
                    s = s + ((i == k ? 1.0 : 0.0) - K[i * 4 + k]) * sym_lower<4>(E, k, j);
                C[i * 4 + j] = s;
                C[j * 4 + i] = s;
            }
    if (!is_covariance_valid<4>(C))
        return kKalmanInvalidOutput;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        xOut[i] = xn[i];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        Pout[i] = C[i];
    return kKalmanOk;
}

// get_plane_coordinate_system (boundary_polygon.cpp:27-39, 505-513): select_correct_transform, two cross products, two
// normalisations.  false where the host throws (the normal's norm is not 1 within 1e-9); the axes are then not written.
__device__ __forceinline__ bool plane_coordinate_system(const double* n, double* xAxis, double* yAxis)
{
    if (!(fabs(norm3(n) - 1.0) <= 1e-9))
        return false;
    // select_correct_transform; std::min(a, b) is b < a ? b : a
    const double distX = fabs(n[0]), distY = fabs(n[1]), distZ = fabs(n[2]);
    const double yz = distZ < distY ? distZ : distY;
    const double res = yz < distX ? yz : distX;
    double r[3];
    if (fabs(res - distX) <= 0.1)
        r[0] = 1, r[1] = 0, r[2] = 0;
    else if (fabs(res - distY) <= 0.1)
        r[0] = 0, r[1] = 1, r[2] = 0;
    else if (fabs(res - distZ) <= 0.1)
        r[0] = 0, r[1] = 0, r[2] = 1;
    else
    {
        r[0] = n[2], r[1] = n[0], r[2] = n[1];
        normalize3(r);
    }
    xAxis[0] = n[1] * r[2] - n[2] * r[1];
    xAxis[1] = n[2] * r[0] - n[0] * r[2];
    xAxis[2] = n[0] * r[1] - n[1] * r[0];
    normalize3(xAxis);
    yAxis[0] = n[1] * xAxis[2] - n[2] * xAxis[1];
    yAxis[1] = n[2] * xAxis[0] - n[0] * xAxis[2];
    yAxis[2] = n[0] * xAxis[1] - n[1] * xAxis[0];
    normalize3(yAxis);
    return true;
}

} // namespace

} // namespace cape

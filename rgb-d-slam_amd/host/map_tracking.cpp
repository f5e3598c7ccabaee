// See map_tracking.hpp.  Every sum runs left to right over its index; products with the identity dynamics and output
// matrices of the plane filter are written out as the values they produce (x * 1 + 0 * y is exact).
#include "map_tracking.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>

#include "boundary_polygon.hpp"

namespace rgbd_slam::map_tracking {

namespace {

constexpr double kEps = std::numeric_limits<double>::epsilon();
inline bool double_equal(double a, double b) { return std::abs(a - b) <= kEps; }

// the lower triangle mirrored: Eigen's selfadjointView<Lower>() read as a full matrix
inline double sym_lower(const double* S, int n, int i, int j) { return i >= j ? S[i * n + j] : S[j * n + i]; }

// propagate_covariance (covariances.hpp:55-64): (J * S.selfadjointView<Lower>() * J^T).selfadjointView<Lower>() + eps I.
// S: n x n, J: m x n, out: m x m.
void propagate(const double* S, int n, const double* J, int m, double eps, double* out)
{
    double T[4 * 4];
    for (int i = 0; i < m; ++i)
        for (int k = 0; k < n; ++k)
        {
            double s = J[i * n] * sym_lower(S, n, 0, k);
            for (int l = 1; l < n; ++l)
                s = s + J[i * n + l] * sym_lower(S, n, l, k);
            T[i * n + k] = s;
        }
    for (int i = 0; i < m; ++i)
        for (int j = 0; j <= i; ++j)
        {
            double s = T[i * n] * J[j * n];
            for (int k = 1; k < n; ++k)
                s = s + T[i * n + k] * J[j * n + k];
            out[i * m + j] = s;
            out[j * m + i] = s;
        }
    for (int i = 0; i < m; ++i)
        out[i * m + i] = out[i * m + i] + eps;
}

} // namespace

bool is_covariance_valid(const double* M, int n) noexcept
{
    if (n < 1 || n > kMaxCovarianceSize)
        return false;
    for (int i = 0; i < n * n; ++i)
        if (!std::isfinite(M[i]))
            return false; // "invalid values"
    // M.isApprox(M^T): |M - M^T|^2 <= prec^2 min(|M|^2, |M^T|^2), Frobenius, prec = dummy_precision
    double diff = 0.0, a = 0.0, b = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
        {
            const double e = M[i * n + j] - M[j * n + i];
            diff = diff + e * e;
            a = a + M[i * n + j] * M[i * n + j];
            b = b + M[j * n + i] * M[j * n + i];
        }
    const double prec = 1e-12;
    if (!(diff <= prec * prec * std::min(a, b)))
        return false; // "not symetrical"
    // selfadjointView<Upper>().ldlt(): Eigen's unblocked LDLT with diagonal pivoting on the transpose's lower triangle
    double m[kMaxCovarianceSize * kMaxCovarianceSize]; // (the exchange and the elimination below are written for any n)
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            m[i * n + j] = M[j * n + i];
    enum
    {
        ZERO,
        POSITIVE,
        NEGATIVE,
        INDEFINITE
    } sign = ZERO;
    bool ok = true, foundZeroPivot = false;
    double temp[kMaxCovarianceSize];
    for (int k = 0; k < n; ++k)
    {
        int big = k;
        for (int i = k + 1; i < n; ++i)
            if (std::abs(m[i * n + i]) > std::abs(m[big * n + big]))
                big = i;
        if (big != k)
        {
            for (int j = 0; j < k; ++j)
                std::swap(m[k * n + j], m[big * n + j]);
            for (int r = big + 1; r < n; ++r)
                std::swap(m[r * n + k], m[r * n + big]);
            std::swap(m[k * n + k], m[big * n + big]);
            for (int i = k + 1; i < big; ++i)
            {
                const double t = m[i * n + k];
                m[i * n + k] = m[big * n + i];
                m[big * n + i] = t;
            }
        }
        const int rs = n - k - 1;
        if (k > 0)
        {
            for (int i = 0; i < k; ++i)
                temp[i] = m[i * n + i] * m[k * n + i];
            double s = m[k * n] * temp[0];
            for (int i = 1; i < k; ++i)
                s = s + m[k * n + i] * temp[i];
            m[k * n + k] = m[k * n + k] - s;
            for (int r = k + 1; r < n; ++r)
            {
                double t = m[r * n] * temp[0];
                for (int i = 1; i < k; ++i)
                    t = t + m[r * n + i] * temp[i];
                m[r * n + k] = m[r * n + k] - t;
            }
        }
        const double akk = m[k * n + k];
        const bool pivotValid = std::abs(akk) > 0.0;
        if (k == 0 && !pivotValid)
        {
            sign = ZERO;
            ok = false;
            break;
        }
        if (rs > 0 && pivotValid)
            for (int r = k + 1; r < n; ++r)
                m[r * n + k] = m[r * n + k] / akk;
        else if (rs > 0)
            for (int r = k + 1; r < n; ++r)
                ok = ok && m[r * n + k] == 0.0;
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
    return ok && (sign == POSITIVE || sign == ZERO); // info() == Success and isPositive()
}

double norm3(const double* n) noexcept { return std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]); }

void normalize3(double* n) noexcept
{
    const double z = norm3(n);
    if (z > 0)
    {
        n[0] = n[0] / z;
        n[1] = n[1] / z;
        n[2] = n[2] / z;
    }
}

void plane_to_world(const double* normal, double d, const double* T, double* normalOut, double* dOut) noexcept
{
    // the plane matrix of a camera-to-world transform is built like that of a world-to-camera one
    rgbd_slam::utils::plane_to_camera(normal, d, T, normalOut, dOut);
}

bool plane_covariance(const double* normal, double d, const double* pointCloudCov9, double* out16) noexcept
{
    if (!is_covariance_valid(pointCloudCov9, 3))
        return false;
    if (double_equal(d, 0.0) || !double_equal(norm3(normal), 1.0))
        return false;
    const double a = normal[0] * d, b = normal[1] * d, c = normal[2] * d;
    const double aSquared = a * a, bSquared = b * b, cSquared = c * c;
    const double divider = std::pow(aSquared + bSquared + cSquared, 3.0 / 2.0);
    const double common = 1.0 / std::sqrt(aSquared + bSquared + cSquared);
    const double J[12] = {common - aSquared / divider, -(a * b) / divider,          -(a * c) / divider,
                          -(a * b) / divider,          common - bSquared / divider, -(b * c) / divider,
                          -(a * c) / divider,          -(b * c) / divider,          common - cSquared / divider,
                          -a / divider,                -b / divider,                -c / divider};
    propagate(pointCloudCov9, 3, J, 4, 0.01, out16);
    return is_covariance_valid(out16, 4);
}

bool reduced_point_cloud_covariance(const double* normal, double d, const double* planeCov16, double* out9) noexcept
{
    if (!is_covariance_valid(planeCov16, 4))
        return false;
    if (double_equal(d, 0.0) || !double_equal(norm3(normal), 1.0))
        return false;
    const double J[12] = {d, 0, 0, normal[0], 0, d, 0, normal[1], 0, 0, d, normal[2]};
    propagate(planeCov16, 4, J, 3, 0.01, out9);
    return is_covariance_valid(out9, 3);
}

bool world_plane_covariance(const double* normal, double d, const double* T, const double* planeCov16, const double* poseCov9,
                            double* out16) noexcept
{
    if (!is_covariance_valid(planeCov16, 4))
        return false;
    double pcc[9];
    if (!reduced_point_cloud_covariance(normal, d, planeCov16, pcc))
        return false;
    const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    double world[9];
    propagate(pcc, 3, R, 3, 0.0, world);
    for (int i = 0; i < 9; ++i)
        world[i] = world[i] + poseCov9[i];
    if (!is_covariance_valid(world, 3))
        return false;
    double nw[3], dw;
    plane_to_world(normal, d, T, nw, &dw);
    return plane_covariance(nw, dw, world, out16);
}

double det44(const double* a) noexcept
{
    const double s0 = a[0] * a[5] - a[4] * a[1], s1 = a[0] * a[6] - a[4] * a[2], s2 = a[0] * a[7] - a[4] * a[3];
    const double s3 = a[1] * a[6] - a[5] * a[2], s4 = a[1] * a[7] - a[5] * a[3], s5 = a[2] * a[7] - a[6] * a[3];
    const double c5 = a[10] * a[15] - a[14] * a[11], c4 = a[9] * a[15] - a[13] * a[11], c3 = a[9] * a[14] - a[13] * a[10];
    const double c2 = a[8] * a[15] - a[12] * a[11], c1 = a[8] * a[14] - a[12] * a[10], c0 = a[8] * a[13] - a[12] * a[9];
    return s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
}

void inverse44(const double* a, double det, double* b) noexcept
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

KalmanStatus kalman_update(const double* x, const double* P, const double* z, const double* R, double* xOut, double* Pout) noexcept
{
    if (!is_covariance_valid(P, 4) || !is_covariance_valid(R, 4))
        return KALMAN_INVALID_INPUT;
    const double processNoise = 0.000001;
    // estimateErrorCovariance = propagate(P, I) + 1e-6 I; innovation = propagate(that, I) + R
    double E[16], S[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            E[i * 4 + j] = sym_lower(P, 4, i, j) + (i == j ? processNoise : 0.0);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            S[i * 4 + j] = sym_lower(E, 4, i, j) + R[i * 4 + j];
    const double det = det44(S);
    if (double_equal(det, 0.0))
        return KALMAN_SINGULAR;
    double Si[16], K[16];
    inverse44(S, det, Si);
    // kalmanGain = E.selfadjointView<Lower>() * I * S^-1
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
        {
            double s = sym_lower(E, 4, i, 0) * Si[j];
            for (int k = 1; k < 4; ++k)
                s = s + sym_lower(E, 4, i, k) * Si[k * 4 + j];
            K[i * 4 + j] = s;
        }
    double y[4], xn[4], C[16];
    for (int k = 0; k < 4; ++k)
        y[k] = z[k] - x[k];
    for (int i = 0; i < 4; ++i)
    {
        double s = K[i * 4] * y[0];
        for (int k = 1; k < 4; ++k)
            s = s + K[i * 4 + k] * y[k];
        xn[i] = x[i] + s;
    }
    // (I - K) * E.selfadjointView<Lower>(), then its own selfadjointView<Lower>()
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j <= i; ++j)
        {
            double s = ((i == 0 ? 1.0 : 0.0) - K[i * 4]) * sym_lower(E, 4, 0, j);
            for (int k = 1; k < 4; ++k)
                s = s + ((i == k ? 1.0 : 0.0) - K[i * 4 + k]) * sym_lower(E, 4, k, j);
            C[i * 4 + j] = s;
            C[j * 4 + i] = s;
        }
    if (!is_covariance_valid(C, 4))
        return KALMAN_INVALID_OUTPUT;
    for (int i = 0; i < 4; ++i)
        xOut[i] = xn[i];
    for (int i = 0; i < 16; ++i)
        Pout[i] = C[i];
    return KALMAN_OK;
}

} // namespace rgbd_slam::map_tracking

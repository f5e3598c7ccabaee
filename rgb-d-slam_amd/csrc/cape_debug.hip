// Debug / parity entry: evaluates device scalar math on caller-supplied operands so tests can compare the
// gfx950 instruction sequences (f64 div / sqrt expansion, ocml acos / atan2, the restated eigen-solver and plane
// fit) against the CPU oracle bit for bit, and the covariance algebra of cape_map_tracking.h against its host twin
// (decisions equal, values to rounding: it goes through pow; the Kalman step and the plane frame of cape_map_kalman have no pow and
// equal theirs bit for bit).  Not on the hot path.
#include <hip/hip_runtime.h>

#include <string>

#include "cape_device.h"
#include "cape_internal.h"
#include "cape_map_tracking.h"

namespace cape {

__global__ void debug_eval_kernel(int op, const double* a, const double* b, double* out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    switch (op)
    {
    case CAPE_DEBUG_SQRT: out[i] = sqrt(a[i]); break;
    case CAPE_DEBUG_DIV: out[i] = a[i] / b[i]; break;
    case CAPE_DEBUG_ACOS: out[i] = acos(a[i]); break;
    case CAPE_DEBUG_ATAN2: out[i] = atan2(a[i], b[i]); break;
    case CAPE_DEBUG_QUANT: out[i] = depth_quantization(a[i]); break;
    case CAPE_DEBUG_SQRTF: out[i] = (double)sqrtf((float)a[i]); break;
    case CAPE_DEBUG_EIGEN3:
    {
        // a: n x 6 (m00 m10 m11 m20 m21 m22) ; out: n x 12 (3 eigenvalues, 9 eigenvector entries row-major)
        const double* m = a + (size_t)i * 6;
        Eig3 e;
        self_adjoint_eigen3(m[0], m[1], m[2], m[3], m[4], m[5], e);
        double* o = out + (size_t)i * 12;
        o[0] = e.val[0]; o[1] = e.val[1]; o[2] = e.val[2];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                o[3 + 3 * r + c] = e.q[r][c];
        break;
    }
    case CAPE_DEBUG_FIT_PLANE:
    {
        // a: n x 10 (9 sums + count) ; out: n x 10 (nx ny nz d cx cy cz mse score planar)
        const double* s = a + (size_t)i * 10;
        double S[9];
        for (int k = 0; k < 9; ++k)
            S[k] = s[k];
        PlaneFit f;
        fit_plane(S, (uint32_t)s[9], f);
        double* o = out + (size_t)i * 10;
        o[0] = f.nx; o[1] = f.ny; o[2] = f.nz; o[3] = f.d;
        o[4] = f.cx; o[5] = f.cy; o[6] = f.cz;
        o[7] = f.mse; o[8] = f.score; o[9] = f.planar ? 1.0 : 0.0;
        break;
    }
    case CAPE_DEBUG_COV_VALID:
    {
        // a: n x 17 (size, then the matrix row-major in the first size x size entries) ; out: n x 1
        const double* m = a + (size_t)i * 17;
        out[i] = m[0] == 3.0 ? (is_covariance_valid<3>(m + 1) ? 1.0 : 0.0) : m[0] == 4.0 ? (is_covariance_valid<4>(m + 1) ? 1.0 : 0.0) : 0.0;
        break;
    }
    case CAPE_DEBUG_PLANE_COV:
    case CAPE_DEBUG_WORLD_PLANE_COV:
    {
        // a: n x 13 (normal, d, cov9) or n x 45 (normal, d, T16, planeCov16, pose9) ; out: n x 17 (ok, 16 entries: 0 unless ok)
        const bool world = op == CAPE_DEBUG_WORLD_PLANE_COV;
        const double* s = a + (size_t)i * (world ? 45 : 13);
        double cov[16];
        const bool ok = world ? world_plane_covariance(s, s[3], s + 4, s + 20, s + 36, cov) : plane_covariance(s, s[3], s + 4, cov);
        double* o = out + (size_t)i * 17;
        o[0] = ok ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            o[1 + k] = ok ? cov[k] : 0.0;
        break;
    }
    case CAPE_DEBUG_KALMAN:
    {
        // a: n x 40 (x, P, z, R) ; out: n x 21 (status, x', P': 0 unless the status is 0)
        const double* s = a + (size_t)i * 40;
        double xn[4] = {0, 0, 0, 0}, Pn[16];
#pragma unroll
        for (int k = 0; k < 16; ++k)
            Pn[k] = 0.0;
        const int st = kalman_update(s, s + 4, s + 20, s + 24, xn, Pn);
        double* o = out + (size_t)i * 21;
        o[0] = (double)st;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            o[1 + k] = st == kKalmanOk ? xn[k] : 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            o[5 + k] = st == kKalmanOk ? Pn[k] : 0.0;
        break;
    }
    case CAPE_DEBUG_PLANE_FRAME:
    {
        // a: n x 3 (normal) ; out: n x 7 (ok, x axis, y axis: 0 unless ok)
        const double* s = a + (size_t)i * 3;
        double ax[3] = {0, 0, 0}, ay[3] = {0, 0, 0};
        const bool ok = plane_coordinate_system(s, ax, ay);
        double* o = out + (size_t)i * 7;
        o[0] = ok ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o[1 + k] = ok ? ax[k] : 0.0, o[4 + k] = ok ? ay[k] : 0.0;
        break;
    }
    default: out[i] = 0.0;
    }
}

} // namespace cape

extern "C" int cape_debug_eval(int op, const double* a, const double* b, double* out, int n)
{
    if (!a || !out || n <= 0)
        return CAPE_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return CAPE_ERR_NO_DEVICE;
    size_t inW = 1, outW = 1;
    if (op == CAPE_DEBUG_EIGEN3) { inW = 6; outW = 12; }
    if (op == CAPE_DEBUG_FIT_PLANE) { inW = 10; outW = 10; }
    if (op == CAPE_DEBUG_COV_VALID) { inW = 17; outW = 1; }
    if (op == CAPE_DEBUG_PLANE_COV) { inW = 13; outW = 17; }
    if (op == CAPE_DEBUG_WORLD_PLANE_COV) { inW = 45; outW = 17; }
    if (op == CAPE_DEBUG_KALMAN) { inW = 40; outW = 21; }
    if (op == CAPE_DEBUG_PLANE_FRAME) { inW = 3; outW = 7; }
    double *da = nullptr, *db = nullptr, *dout = nullptr;
    int rc = CAPE_OK;
    if (hipMalloc((void**)&da, n * inW * 8) != hipSuccess || hipMalloc((void**)&dout, n * outW * 8) != hipSuccess)
        rc = CAPE_ERR_HIP;
    if (rc == CAPE_OK && b && hipMalloc((void**)&db, (size_t)n * 8) != hipSuccess)
        rc = CAPE_ERR_HIP;
    if (rc == CAPE_OK)
    {
        (void)hipMemcpy(da, a, n * inW * 8, hipMemcpyHostToDevice);
        if (b)
            (void)hipMemcpy(db, b, (size_t)n * 8, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(cape::debug_eval_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, da, db ? db : da, dout, n);
        if (hipMemcpy(out, dout, n * outW * 8, hipMemcpyDeviceToHost) != hipSuccess)
            rc = CAPE_ERR_HIP;
    }
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dout);
    return rc;
}

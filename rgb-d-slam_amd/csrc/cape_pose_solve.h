// cape_map_pose_solve / cape_map_pose_select: the pose solver on the pairs of cape_pose_score.h -- Levenberg-Marquardt over a subset of a
// frame's pairs (compute_optimized_global_pose, pose_optimization.cpp:300-350, through Eigen::LevenbergMarquardt over
// NumericalDiff<Global_Pose_Estimator>) and the RANSAC bookkeeping over a frame's scored hypotheses (pose_optimization.cpp:190-235) -- as
// the rules ONE problem follows.  Plain functions like those of cape_pose_score.h: the kernels (cape_pose_solve.hip), the host twins
// cape_host_pose_solve / cape_host_pose_select (host/pose_solve.cpp) and tests/host/pose_solve_check.cpp compile the same statements.
//
// The pose of x[6] (position, then the three coefficients of get_optimization_coefficients_from_quaternion), stated once:
//   quaternion (w, x, y, z) = (2 c0, 2 c1, 2 c2, 1 - alpha) / (alpha + 1), alpha = c0^2 + c1^2 + c2^2   levenberg_marquardt_functors.cpp:29-38
//   q /= sqrt(((w^2 + x^2) + y^2) + z^2)                                                                PoseBase, pose.cpp:20
//   R = Eigen::Quaternion::toRotationMatrix as it states it (tx = 2x ... R00 = 1 - (tyy + tzz) ...)
//   M = C R, pw = C p; world-to-camera rotation M^T, translation -(M^T pw); every dot product (a + b) + c
//   C: the caller's 3 x 3 camera basis (the reference's constant CameraToWorld, camera_transformation.cpp:11-18; no trigonometric
//   constant is baked in here)
// and the map plane then goes through plane_to_camera (cape_map_camera.h on the device, utils::plane_to_camera on the host: the caller
// hands it in).  Residuals in pair order k ascending, c ascending within a pair: r = reduced[c] * 1.0 / 3.0 (pose_pair_reduced, the LM
// functor's scaling, levenberg_marquardt_functors.cpp:154-166).
//
// Three deliberate departures from the reference, none of which changes the mathematics:
//   1. the world-to-camera transform is the rigid inverse by transposition, not Eigen's general 4 x 4 inverse;
//   2. every norm is the square root of a plain ordered sum, not Eigen's stableNorm / blueNorm;
//   3. the rows come in pair order; the reference's subset is in reverse pick order (ransac.hpp:91-99).
// Eigen is not a dependency of this project: bit parity with it is neither claimed nor tested.  tests/test_pose_solve_host.py measures
// the twin against MINPACK's lmdif (scipy.optimize.leastsq) on the same residuals.
//
// The minimiser is MINPACK's Levenberg-Marquardt (More, Garbow, Hillstrom: User Guide for MINPACK-1, ANL-80-74) with the parameters
// Eigen::LevenbergMarquardt defaults to, written from the published algorithm; each block is named after the routine it restates:
//   fdjac2 : forward differences, h = sqrt(max(epsfcn, eps)) |x_j| (that factor alone where x_j = 0): 6 evaluations, counted in nfev
//   lmstr  : the driver with minimal storage -- the Jacobian's rows are produced pair by pair and folded by Givens rotations (rwupdt)
//            into a 6 x 6 upper-triangular R and Q^T f; the pivoted qrfac runs on R only when a diagonal entry is 0; then lmpar / qrsolv,
//            the actred / prered / ratio updates of delta and par, and the termination tests with info 1..8.
// A problem's state is 36 + O(10 x 6) doubles whatever the subset size: one body serves a 3-pair subset (m = 9) and a 128-pair refit
// (m = 384).  n = 6 everywhere and every loop over it has constant bounds: fully unrolled, no array is indexed by a run-time value
// (the pivot vector is resolved by selects: lm_gather / lm_scatter), so the kernel needs no scratch.
#pragma once
#include <float.h>

#include "cape_pose_score.h"

#if defined(__HIPCC__)
#include "cape_layout.h"     // the LDS carve and plane_to_camera of the device's steps at the end of this file
#include "cape_map_camera.h"
#define CAPE_POSE_UNROLL _Pragma("unroll")
#else
#define CAPE_POSE_UNROLL
#endif

namespace cape {

constexpr int kPoseSolveGroupProblems = kPoseScoreGroupHypotheses; // problems of a solve workgroup: four waves, a lane each
constexpr float kPoseSelectInlierShare = 0.80f; // pose_optimization.cpp:225: a float constant, widened to double where it is used

// the parameters of a call (cape_pose_solve_params with the defaults filled in), passed to the kernel by value
struct PoseSolveSettings
{
    double ftol, xtol, gtol, factor, eps; // eps = sqrt(max(epsfcn, DBL_EPSILON)): the relative step of fdjac2
    int maxfev, mode;
    double C[9];
};
// NaN, negative or out-of-range parameters: false
CAPE_POSE_FN bool pose_solve_settings(const cape_pose_solve_params* p, PoseSolveSettings& S)
{
    S.ftol = S.xtol = sqrt(DBL_EPSILON);
    S.gtol = 0.0;
    S.factor = 100.0;
    S.eps = sqrt(DBL_EPSILON);
    S.maxfev = 400;
    S.mode = 1;
    for (int c = 0; c < 9; ++c)
        S.C[c] = (c % 4 == 0) ? 1.0 : 0.0;
    if (!p)
        return true;
    if (!(p->ftol >= 0.0) || !(p->xtol >= 0.0) || !(p->gtol >= 0.0) || !(p->factor > 0.0) || !(p->epsfcn >= 0.0) || p->maxfev < 1 ||
        (p->mode != 1 && p->mode != 2))
        return false;
    for (int c = 0; c < 9; ++c)
        if (!(fabs(p->camera_basis[c]) <= DBL_MAX))
            return false;
    S.ftol = p->ftol, S.xtol = p->xtol, S.gtol = p->gtol, S.factor = p->factor;
    S.eps = sqrt(p->epsfcn > DBL_EPSILON ? p->epsfcn : DBL_EPSILON);
    S.maxfev = p->maxfev, S.mode = p->mode;
    for (int c = 0; c < 9; ++c)
        S.C[c] = p->camera_basis[c];
    return true;
}

CAPE_POSE_FN bool pose_finite(double v) { return fabs(v) <= DBL_MAX; } // (a NaN compares false)

// ---- the rotation of x's three coefficients, before the camera basis (row-major)
CAPE_POSE_FN void pose_rotation_from_coefficients(const double x[6], double R[9])
{
    const double alpha = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5];
    const double divider = 1.0 / (alpha + 1);
    double qw = 2.0 * x[3] * divider, qx = 2.0 * x[4] * divider, qy = 2.0 * x[5] * divider, qz = (1 - alpha) * divider;
    const double norm = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw = qw / norm, qx = qx / norm, qy = qy / norm, qz = qz / norm;
    const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}
// ---- the pose of x: T[12] = the first three rows of the row-major world-to-camera matrix
CAPE_POSE_FN void pose_from_coefficients(const double x[6], const double C[9], double T[12])
{
    double R[9];
    pose_rotation_from_coefficients(x, R);
    double M[9], pw[3];
    CAPE_POSE_UNROLL
    for (int r = 0; r < 3; ++r)
    {
        CAPE_POSE_UNROLL
        for (int c = 0; c < 3; ++c)
            M[3 * r + c] = (C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c];
        pw[r] = (C[3 * r] * x[0] + C[3 * r + 1] * x[1]) + C[3 * r + 2] * x[2];
    }
    CAPE_POSE_UNROLL
    for (int r = 0; r < 3; ++r)
    {
        CAPE_POSE_UNROLL
        for (int c = 0; c < 3; ++c)
            T[4 * r + c] = M[3 * c + r];
        T[4 * r + 3] = -((M[r] * pw[0] + M[3 + r] * pw[1]) + M[6 + r] * pw[2]);
    }
}
CAPE_POSE_FN void pose_matrix16(const double T[12], double out[16])
{
    for (int c = 0; c < 12; ++c)
        out[c] = T[c];
    out[12] = out[13] = out[14] = 0.0, out[15] = 1.0;
}

// ---- a problem's rows: what the solve reads of the frame's feature rows (the LDS copy on the device, a vector on the host)
struct PoseSolveRows
{
    const double* planes; // 8 per pair: (cn, cd), then the map plane
    const int* kept;      // the pair's kept plane
    int nPairs;
    unsigned long long subsetLo, subsetHi; // bit i: the pair of kept plane i (Lo), i + 64 (Hi) takes part
    // the map plane of pair k: the row's own.  Another source of rows (cape_pose_covariance.h: a lane's varied planes) derives from this
    // struct and answers with four values of its own in `own`
    CAPE_POSE_FN const double* map_plane(int k, double*) const { return planes + 8 * k + 4; }
};
// a subset's four words (cape_map_pose_solve's `subsets`, a selection's or a score's inlier_words) as the rows' two halves
CAPE_POSE_FN void pose_subset(const uint32_t words[4], unsigned long long& lo, unsigned long long& hi)
{
    lo = (unsigned long long)words[0] | ((unsigned long long)words[1] << 32);
    hi = (unsigned long long)words[2] | ((unsigned long long)words[3] << 32);
}
CAPE_POSE_FN bool pose_solve_takes(const PoseSolveRows& rows, int k)
{
    const int i = rows.kept[k];
    return (((i < 64 ? rows.subsetLo : rows.subsetHi) >> (i & 63)) & 1ull) != 0ull;
}
// row k of `planes` and `kept` from the pair's feature row: the two planes and the kept plane, 68 of its 112 bytes
CAPE_POSE_FN void pose_rows_fill(const cape_pose_feature& F, int k, double* planes, int* kept)
{
    CAPE_POSE_UNROLL
    for (int c = 0; c < 4; ++c)
        planes[8 * k + c] = F.matched[c], planes[8 * k + 4 + c] = F.map_plane[c];
    kept[k] = F.kept_plane; // (it selects a subset bit; no address is formed from it)
}
// the three residuals of pair k under T
template <class Rows, class PlaneToCamera>
CAPE_POSE_FN void pose_solve_pair(const Rows& rows, int k, const double T[12], const PlaneToCamera& planeToCamera, double r[3])
{
    const double* row = rows.planes + 8 * k;
    const double cn[3] = {row[0], row[1], row[2]};
    double qn[3], qd, reduced[3], own[4];
    const double* map = rows.map_plane(k, own);
    planeToCamera(T, map, map[3], qn, qd);
    pose_pair_reduced(cn, row[3], qn, qd, reduced);
    CAPE_POSE_UNROLL
    for (int c = 0; c < 3; ++c)
        r[c] = reduced[c] * 1.0 / 3.0;
}
// the norm of the residual vector at x: one evaluation
template <class Rows, class PlaneToCamera>
CAPE_POSE_FN double pose_solve_fnorm(const Rows& rows, const double x[6], const double C[9], const PlaneToCamera& planeToCamera)
{
    double T[12];
    pose_from_coefficients(x, C, T);
    double sum = 0.0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int k = 0; k < rows.nPairs; ++k)
        if (pose_solve_takes(rows, k))
        {
            double r[3];
            pose_solve_pair(rows, k, T, planeToCamera, r);
            sum += r[0] * r[0];
            sum += r[1] * r[1];
            sum += r[2] * r[2];
        }
    return sqrt(sum);
}

// ---- n = 6 vectors
CAPE_POSE_FN double lm_enorm(const double v[6]) // (departure 2: a plain ordered sum)
{
    double s = 0.0;
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
        s += v[j] * v[j];
    return sqrt(s);
}
// out[j] = v[ipvt[j]] and out[ipvt[j]] = v[j] by selects: no run-time index
// (the six values are read once into scalars and every output is a chain of selects over them: written over the array elements
// instead, the compiler turns a select of two loads into a load through a selected address, which keeps the array in memory)
CAPE_POSE_FN double lm_pick(int i, double v0, double v1, double v2, double v3, double v4, double v5)
{
    double o = v0;
    o = i == 1 ? v1 : o;
    o = i == 2 ? v2 : o;
    o = i == 3 ? v3 : o;
    o = i == 4 ? v4 : o;
    o = i == 5 ? v5 : o;
    return o;
}
CAPE_POSE_FN void lm_gather(const double v[6], const int ipvt[6], double out[6])
{
    const double v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5];
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
        out[j] = lm_pick(ipvt[j], v0, v1, v2, v3, v4, v5);
}
CAPE_POSE_FN void lm_scatter(const double v[6], const int ipvt[6], double out[6])
{
    const double v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5];
    const int p1 = ipvt[1], p2 = ipvt[2], p3 = ipvt[3], p4 = ipvt[4], p5 = ipvt[5];
    CAPE_POSE_UNROLL
    for (int k = 0; k < 6; ++k)
    {
        // (ipvt is a permutation: exactly one j names k; j = 0 is the default)
        double o = v0;
        o = p1 == k ? v1 : o;
        o = p2 == k ? v2 : o;
        o = p3 == k ? v3 : o;
        o = p4 == k ? v4 : o;
        o = p5 == k ? v5 : o;
        out[k] = o;
    }
}

// a Givens rotation that eliminates b against a (the statement rwupdt and qrsolv share)
CAPE_POSE_FN void lm_givens(double a, double b, double& cosine, double& sine)
{
    double c, s; // (both results leave through one pair of stores: a store per branch would reach the caller's arrays through a pointer)
    if (fabs(a) < fabs(b))
    {
        const double cotan = a / b;
        s = 0.5 / sqrt(0.25 + 0.25 * (cotan * cotan));
        c = s * cotan;
    }
    else
    {
        const double tangent = b / a;
        c = 0.5 / sqrt(0.25 + 0.25 * (tangent * tangent));
        s = c * tangent;
    }
    cosine = c, sine = s;
}

// rwupdt: fold the row w (and its right-hand side alpha) into the upper triangle R (row-major r[6 i + j]) and b = Q^T f
CAPE_POSE_FN void lm_rwupdt(double r[36], const double w[6], double b[6], double alpha)
{
    double cosine[6], sine[6];
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
    {
        double rowj = w[j];
        // the previous rotations on r(i, j), i < j, and on w(j)
        CAPE_POSE_UNROLL
        for (int i = 0; i < j; ++i)
        {
            const double temp = cosine[i] * r[6 * i + j] + sine[i] * rowj;
            rowj = -sine[i] * r[6 * i + j] + cosine[i] * rowj;
            r[6 * i + j] = temp;
        }
        // the rotation that eliminates w(j)
        cosine[j] = 1.0, sine[j] = 0.0;
        if (rowj != 0.0)
        {
            lm_givens(r[6 * j + j], rowj, cosine[j], sine[j]);
            r[6 * j + j] = cosine[j] * r[6 * j + j] + sine[j] * rowj;
            const double temp = cosine[j] * b[j] + sine[j] * alpha;
            alpha = -sine[j] * b[j] + cosine[j] * alpha;
            b[j] = temp;
        }
    }
}

// qrfac with column pivoting on the 6 x 6 matrix a (row-major): Householder vectors in the lower trapezoid, R's strict upper triangle
// above, its diagonal in rdiag; acnorm = the columns' norms on entry
CAPE_POSE_FN void lm_qrfac(double a[36], int ipvt[6], double rdiag[6], double acnorm[6])
{
    double wa[6];
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
    {
        double s = 0.0;
        CAPE_POSE_UNROLL
        for (int i = 0; i < 6; ++i)
            s += a[6 * i + j] * a[6 * i + j];
        acnorm[j] = sqrt(s);
        rdiag[j] = acnorm[j], wa[j] = rdiag[j], ipvt[j] = j;
    }
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
    {
        // the column of largest norm into the pivot position
        int kmax = j;
        double largest = rdiag[j];
        CAPE_POSE_UNROLL
        for (int k = j + 1; k < 6; ++k)
            if (rdiag[k] > largest)
                largest = rdiag[k], kmax = k;
        CAPE_POSE_UNROLL
        for (int k = j + 1; k < 6; ++k)
            if (kmax == k)
            {
                CAPE_POSE_UNROLL
                for (int i = 0; i < 6; ++i)
                {
                    const double temp = a[6 * i + j];
                    a[6 * i + j] = a[6 * i + k], a[6 * i + k] = temp;
                }
                rdiag[k] = rdiag[j], wa[k] = wa[j];
                const int t = ipvt[j];
                ipvt[j] = ipvt[k], ipvt[k] = t;
            }
        // the Householder transformation that reduces column j to a multiple of the j-th unit vector
        double s = 0.0;
        CAPE_POSE_UNROLL
        for (int i = j; i < 6; ++i)
            s += a[6 * i + j] * a[6 * i + j];
        double ajnorm = sqrt(s);
        if (ajnorm != 0.0)
        {
            if (a[6 * j + j] < 0.0)
                ajnorm = -ajnorm;
            CAPE_POSE_UNROLL
            for (int i = j; i < 6; ++i)
                a[6 * i + j] = a[6 * i + j] / ajnorm;
            a[6 * j + j] = a[6 * j + j] + 1.0;
            // on the remaining columns, and their norms
            CAPE_POSE_UNROLL
            for (int k = j + 1; k < 6; ++k)
            {
                double sum = 0.0;
                CAPE_POSE_UNROLL
                for (int i = j; i < 6; ++i)
                    sum += a[6 * i + j] * a[6 * i + k];
                const double temp = sum / a[6 * j + j];
                CAPE_POSE_UNROLL
                for (int i = j; i < 6; ++i)
                    a[6 * i + k] = a[6 * i + k] - temp * a[6 * i + j];
                if (rdiag[k] != 0.0)
                {
                    const double t = a[6 * j + k] / rdiag[k];
                    const double d = 1.0 - t * t;
                    rdiag[k] = rdiag[k] * sqrt(d > 0.0 ? d : 0.0);
                    const double q = rdiag[k] / wa[k];
                    if (0.05 * (q * q) <= DBL_EPSILON)
                    {
                        double s2 = 0.0;
                        CAPE_POSE_UNROLL
                        for (int i = j + 1; i < 6; ++i)
                            s2 += a[6 * i + k] * a[6 * i + k];
                        rdiag[k] = sqrt(s2), wa[k] = rdiag[k];
                    }
                }
            }
        }
        rdiag[j] = -ajnorm;
    }
}

// qrsolv: with R in the upper triangle of r, the diagonal matrix D (pdiag[j] = the entry of pivoted column j) and qtb, solve
// R z = Q^T b, D z = 0 in the least-squares sense; z comes back in pivoted order (the caller scatters it), S's diagonal in sdiag, its
// strict upper triangle transposed in the strict lower triangle of r
CAPE_POSE_FN void lm_qrsolv(double r[36], const double pdiag[6], const double qtb[6], double z[6], double sdiag[6])
{
    double saved[6];
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
    {
        CAPE_POSE_UNROLL
        for (int i = j; i < 6; ++i)
            r[6 * i + j] = r[6 * j + i];
        saved[j] = r[6 * j + j];
        z[j] = qtb[j];
    }
    // eliminate the diagonal matrix D by Givens rotations
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
    {
        if (pdiag[j] != 0.0)
        {
            CAPE_POSE_UNROLL
            for (int k = j; k < 6; ++k)
                sdiag[k] = 0.0;
            sdiag[j] = pdiag[j];
            double qtbpj = 0.0;
            CAPE_POSE_UNROLL
            for (int k = j; k < 6; ++k)
                if (sdiag[k] != 0.0)
                {
                    double cosine, sine;
                    lm_givens(r[6 * k + k], sdiag[k], cosine, sine);
                    r[6 * k + k] = cosine * r[6 * k + k] + sine * sdiag[k];
                    const double temp = cosine * z[k] + sine * qtbpj;
                    qtbpj = -sine * z[k] + cosine * qtbpj;
                    z[k] = temp;
                    CAPE_POSE_UNROLL
                    for (int i = k + 1; i < 6; ++i)
                    {
                        const double t = cosine * r[6 * i + k] + sine * sdiag[i];
                        sdiag[i] = -sine * r[6 * i + k] + cosine * sdiag[i];
                        r[6 * i + k] = t;
                    }
                }
        }
        sdiag[j] = r[6 * j + j];
        r[6 * j + j] = saved[j];
    }
    // the triangular system; a singular one in the least-squares sense
    int nsing = 6;
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
    {
        if (sdiag[j] == 0.0 && nsing == 6)
            nsing = j;
        if (nsing < 6)
            z[j] = 0.0;
    }
    CAPE_POSE_UNROLL
    for (int j = 5; j >= 0; --j)
        if (j < nsing)
        {
            double sum = 0.0;
            CAPE_POSE_UNROLL
            for (int i = j + 1; i < 6; ++i)
                if (i < nsing)
                    sum += r[6 * i + j] * z[i];
            z[j] = (z[j] - sum) / sdiag[j];
        }
}

// lmpar: the Levenberg-Marquardt parameter par and the step x (in the variables' own order) with ||D x|| within 10 % of delta
CAPE_POSE_FN void lm_lmpar(double r[36], const int ipvt[6], const double diag[6], const double qtb[6], double delta, double& par, double x[6])
{
    const double dwarf = DBL_MIN;
    double pdiag[6], wa1[6], wa2[6], pwa2[6], sdiag[6];
    lm_gather(diag, ipvt, pdiag);
    // the Gauss-Newton direction; a rank-deficient Jacobian: a least-squares solution
    int nsing = 6;
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
    {
        wa1[j] = qtb[j];
        if (r[6 * j + j] == 0.0 && nsing == 6)
            nsing = j;
        if (nsing < 6)
            wa1[j] = 0.0;
    }
    CAPE_POSE_UNROLL
    for (int j = 5; j >= 0; --j)
        if (j < nsing)
        {
            wa1[j] = wa1[j] / r[6 * j + j];
            const double temp = wa1[j];
            CAPE_POSE_UNROLL
            for (int i = 0; i < j; ++i)
                wa1[i] = wa1[i] - r[6 * i + j] * temp;
        }
    lm_scatter(wa1, ipvt, x);
    // the function at the origin; is the Gauss-Newton direction accepted?
    int iter = 0;
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
        wa2[j] = diag[j] * x[j];
    double dxnorm = lm_enorm(wa2);
    double fp = dxnorm - delta;
    if (!(fp <= 0.1 * delta))
    {
        // a full-rank Jacobian: the Newton step gives a lower bound parl for the zero of the function
        double parl = 0.0;
        if (nsing >= 6)
        {
            lm_gather(wa2, ipvt, pwa2);
            CAPE_POSE_UNROLL
            for (int j = 0; j < 6; ++j)
                wa1[j] = pdiag[j] * (pwa2[j] / dxnorm);
            CAPE_POSE_UNROLL
            for (int j = 0; j < 6; ++j)
            {
                double sum = 0.0;
                CAPE_POSE_UNROLL
                for (int i = 0; i < j; ++i)
                    sum += r[6 * i + j] * wa1[i];
                wa1[j] = (wa1[j] - sum) / r[6 * j + j];
            }
            const double temp = lm_enorm(wa1);
            parl = ((fp / delta) / temp) / temp;
        }
        // an upper bound paru
        CAPE_POSE_UNROLL
        for (int j = 0; j < 6; ++j)
        {
            double sum = 0.0;
            CAPE_POSE_UNROLL
            for (int i = 0; i <= j; ++i)
                sum += r[6 * i + j] * qtb[i];
            wa1[j] = sum / pdiag[j];
        }
        const double gnorm = lm_enorm(wa1);
        double paru = gnorm / delta;
        if (paru == 0.0)
            paru = dwarf / (delta < 0.1 ? delta : 0.1);
        // par into (parl, paru)
        par = par > parl ? par : parl;
        par = par < paru ? par : paru;
        if (par == 0.0)
            par = gnorm / dxnorm;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (;;)
        {
            ++iter;
            // the function at the current par
            if (par == 0.0)
                par = dwarf > 0.001 * paru ? dwarf : 0.001 * paru;
            const double root = sqrt(par);
            CAPE_POSE_UNROLL
            for (int j = 0; j < 6; ++j)
                wa1[j] = root * pdiag[j];
            double z[6];
            lm_qrsolv(r, wa1, qtb, z, sdiag);
            lm_scatter(z, ipvt, x);
            CAPE_POSE_UNROLL
            for (int j = 0; j < 6; ++j)
                wa2[j] = diag[j] * x[j];
            dxnorm = lm_enorm(wa2);
            const double temp = fp;
            fp = dxnorm - delta;
            // small enough, or the exceptional cases (parl = 0 and fp still negative; ten iterations); a NaN ends it too
            if (fabs(fp) <= 0.1 * delta || (parl == 0.0 && fp <= temp && temp < 0.0) || iter == 10 || !(fp == fp))
                break;
            // the Newton correction
            lm_gather(wa2, ipvt, pwa2);
            CAPE_POSE_UNROLL
            for (int j = 0; j < 6; ++j)
                wa1[j] = pdiag[j] * (pwa2[j] / dxnorm);
            CAPE_POSE_UNROLL
            for (int j = 0; j < 6; ++j)
            {
                wa1[j] = wa1[j] / sdiag[j];
                const double t = wa1[j];
                CAPE_POSE_UNROLL
                for (int i = j + 1; i < 6; ++i)
                    wa1[i] = wa1[i] - r[6 * i + j] * t;
            }
            const double tnorm = lm_enorm(wa1);
            const double parc = ((fp / delta) / tnorm) / tnorm;
            if (fp > 0.0)
                parl = parl > par ? parl : par;
            if (fp < 0.0)
                paru = paru < par ? paru : par;
            par = parl > par + parc ? parl : par + parc;
        }
    }
    if (iter == 0)
        par = 0.0;
}

// ---- the guards in front of the minimiser (pose_optimization.cpp:270-282, :322-331): 0 = solve, else the refusal's status
CAPE_POSE_FN int pose_solve_refusal(const PoseSolveRows& rows, int nInvalid, uint32_t frameFlags, const double x0[6], int& nUsed)
{
    nUsed = 0;
    double score = 0.0;
    for (int k = 0; k < rows.nPairs; ++k)
        if (pose_solve_takes(rows, k))
        {
            ++nUsed;
            score += 1.0 / 3;
        }
    bool finite = true;
    for (int j = 0; j < 6; ++j)
        finite = finite && pose_finite(x0[j]);
    if (frameFlags & CAPE_MATCH_EXACT_OVERFLOW)
        return CAPE_POSE_SOLVE_OVERFLOW;
    if (nInvalid > 0)
        return CAPE_POSE_SOLVE_INVALID_FEATURE;
    if (!finite)
        return CAPE_POSE_SOLVE_BAD_START;
    if (3 * nUsed <= 6)
        return CAPE_POSE_SOLVE_TOO_FEW_PAIRS;
    if (score < 1.0)
        return CAPE_POSE_SOLVE_LOW_SCORE;
    return 0;
}

// ---- lmstr over fdjac2: one problem from x0; T = the pose of the row's x
template <class Rows, class PlaneToCamera>
CAPE_POSE_FN cape_pose_solution pose_solve_problem(const Rows& rows, int nInvalid, uint32_t frameFlags, const double x0[6],
                                                   const PoseSolveSettings& S, const PlaneToCamera& planeToCamera, double T[12])
{
    cape_pose_solution out;
    out.fnorm0 = out.fnorm = 0.0;
    out.nfev = out.iterations = 0;
    out.flags = (frameFlags & (uint32_t)CAPE_MATCH_EXACT_OVERFLOW) | (nInvalid > 0 ? (uint32_t)CAPE_POSE_SCORE_INVALID_FEATURE : 0u);
    out.reserved[0] = out.reserved[1] = out.reserved[2] = 0u;
    double x[6];
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
        x[j] = x0[j];
    int nUsed;
    int info = pose_solve_refusal(rows, nInvalid, frameFlags, x0, nUsed);
    out.n_pairs_used = nUsed;
    if (info == 0)
    {
        const double epsmch = DBL_EPSILON;
        double r[36], qtf[6], diag[6], wa1[6], wa2[6], wa3[6], wa4[6], pv[6];
        int ipvt[6];
        // the function at the start
        double fnorm = pose_solve_fnorm(rows, x, S.C, planeToCamera);
        int nfev = 1, iter = 1;
        out.fnorm0 = fnorm;
        if (!pose_finite(fnorm))
            info = CAPE_POSE_SOLVE_NOT_FINITE;
        double par = 0.0, delta = 0.0, xnorm = 0.0;
        CAPE_POSE_UNROLL
        for (int j = 0; j < 6; ++j)
            diag[j] = 1.0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        while (info == 0)
        {
            // ---- fdjac2, row by row, into rwupdt: R and Q^T f
            CAPE_POSE_UNROLL
            for (int c = 0; c < 36; ++c)
                r[c] = 0.0;
            CAPE_POSE_UNROLL
            for (int j = 0; j < 6; ++j)
                qtf[j] = 0.0;
            {
                double Tx[7][12], h[6];
                pose_from_coefficients(x, S.C, Tx[6]);
                CAPE_POSE_UNROLL
                for (int j = 0; j < 6; ++j)
                {
                    h[j] = S.eps * fabs(x[j]);
                    if (h[j] == 0.0)
                        h[j] = S.eps;
                    double xs[6];
                    CAPE_POSE_UNROLL
                    for (int i = 0; i < 6; ++i)
                        xs[i] = i == j ? x[i] + h[j] : x[i];
                    pose_from_coefficients(xs, S.C, Tx[j]);
                }
#if defined(__HIPCC__)
#pragma unroll 1
#endif
                for (int k = 0; k < rows.nPairs; ++k)
                    if (pose_solve_takes(rows, k))
                    {
                        double f[3], fj[6][3];
                        pose_solve_pair(rows, k, Tx[6], planeToCamera, f);
                        CAPE_POSE_UNROLL
                        for (int j = 0; j < 6; ++j)
                            pose_solve_pair(rows, k, Tx[j], planeToCamera, fj[j]);
                        CAPE_POSE_UNROLL
                        for (int c = 0; c < 3; ++c)
                        {
                            double w[6];
                            CAPE_POSE_UNROLL
                            for (int j = 0; j < 6; ++j)
                                w[j] = (fj[j][c] - f[c]) / h[j];
                            lm_rwupdt(r, w, qtf, f[c]);
                        }
                    }
                nfev += 6;
            }
            // ---- a rank-deficient Jacobian: the pivoted qrfac on R
            bool sing = false;
            CAPE_POSE_UNROLL
            for (int j = 0; j < 6; ++j)
            {
                if (r[6 * j + j] == 0.0)
                    sing = true;
                ipvt[j] = j;
                double s = 0.0;
                CAPE_POSE_UNROLL
                for (int i = 0; i <= j; ++i)
                    s += r[6 * i + j] * r[6 * i + j];
                wa2[j] = sqrt(s);
            }
            if (sing)
            {
                out.flags |= (uint32_t)CAPE_POSE_SOLVE_RANK_DEFICIENT;
                lm_qrfac(r, ipvt, wa1, wa2);
                CAPE_POSE_UNROLL
                for (int j = 0; j < 6; ++j)
                {
                    if (r[6 * j + j] != 0.0)
                    {
                        double sum = 0.0;
                        CAPE_POSE_UNROLL
                        for (int i = j; i < 6; ++i)
                            sum += r[6 * i + j] * qtf[i];
                        const double temp = -sum / r[6 * j + j];
                        CAPE_POSE_UNROLL
                        for (int i = j; i < 6; ++i)
                            qtf[i] = qtf[i] + r[6 * i + j] * temp;
                    }
                    r[6 * j + j] = wa1[j];
                }
            }
            // ---- the first iteration: scale by the columns' norms, the step bound
            if (iter == 1)
            {
                if (S.mode != 2)
                {
                    CAPE_POSE_UNROLL
                    for (int j = 0; j < 6; ++j)
                        diag[j] = wa2[j] == 0.0 ? 1.0 : wa2[j];
                }
                CAPE_POSE_UNROLL
                for (int j = 0; j < 6; ++j)
                    wa3[j] = diag[j] * x[j];
                xnorm = lm_enorm(wa3);
                delta = S.factor * xnorm;
                if (delta == 0.0)
                    delta = S.factor;
            }
            // ---- the norm of the scaled gradient
            double gnorm = 0.0;
            if (fnorm != 0.0)
            {
                lm_gather(wa2, ipvt, pv);
                CAPE_POSE_UNROLL
                for (int j = 0; j < 6; ++j)
                    if (pv[j] != 0.0)
                    {
                        double sum = 0.0;
                        CAPE_POSE_UNROLL
                        for (int i = 0; i <= j; ++i)
                            sum += r[6 * i + j] * (qtf[i] / fnorm);
                        const double g = fabs(sum / pv[j]);
                        gnorm = gnorm > g ? gnorm : g;
                    }
            }
            if (gnorm <= S.gtol)
                info = 4;
            if (info != 0)
                break;
            if (S.mode != 2)
            {
                CAPE_POSE_UNROLL
                for (int j = 0; j < 6; ++j)
                    diag[j] = diag[j] > wa2[j] ? diag[j] : wa2[j];
            }
            // ---- the inner loop: until a step is accepted
            double ratio = 0.0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
            do
            {
                lm_lmpar(r, ipvt, diag, qtf, delta, par, wa1);
                CAPE_POSE_UNROLL
                for (int j = 0; j < 6; ++j)
                {
                    wa1[j] = -wa1[j];
                    wa2[j] = x[j] + wa1[j];
                    wa3[j] = diag[j] * wa1[j];
                }
                const double pnorm = lm_enorm(wa3);
                if (iter == 1)
                    delta = delta < pnorm ? delta : pnorm;
                // the function at x + p
                bool finite = true;
                CAPE_POSE_UNROLL
                for (int j = 0; j < 6; ++j)
                    finite = finite && pose_finite(wa2[j]);
                const double fnorm1 = finite ? pose_solve_fnorm(rows, wa2, S.C, planeToCamera) : 0.0;
                nfev += finite ? 1 : 0;
                if (!finite || !pose_finite(fnorm1))
                {
                    info = CAPE_POSE_SOLVE_NOT_FINITE;
                    break;
                }
                // the scaled actual reduction
                double actred = -1.0;
                if (0.1 * fnorm1 < fnorm)
                    actred = 1.0 - (fnorm1 / fnorm) * (fnorm1 / fnorm);
                // the scaled predicted reduction and the scaled directional derivative
                lm_gather(wa1, ipvt, pv);
                CAPE_POSE_UNROLL
                for (int j = 0; j < 6; ++j)
                    wa3[j] = 0.0;
                CAPE_POSE_UNROLL
                for (int j = 0; j < 6; ++j)
                {
                    CAPE_POSE_UNROLL
                    for (int i = 0; i <= j; ++i)
                        wa3[i] = wa3[i] + r[6 * i + j] * pv[j];
                }
                const double temp1 = lm_enorm(wa3) / fnorm, temp2 = (sqrt(par) * pnorm) / fnorm;
                const double prered = temp1 * temp1 + (temp2 * temp2) / 0.5;
                const double dirder = -(temp1 * temp1 + temp2 * temp2);
                ratio = prered != 0.0 ? actred / prered : 0.0;
                // the step bound
                if (ratio <= 0.25)
                {
                    double temp = 0.5;
                    if (actred < 0.0)
                        temp = 0.5 * dirder / (dirder + 0.5 * actred);
                    if (0.1 * fnorm1 >= fnorm || temp < 0.1)
                        temp = 0.1;
                    const double bound = pnorm / 0.1;
                    delta = temp * (delta < bound ? delta : bound);
                    par = par / temp;
                }
                else if (par == 0.0 || ratio >= 0.75)
                {
                    delta = pnorm / 0.5;
                    par = 0.5 * par;
                }
                // a successful iteration
                if (ratio >= 0.0001)
                {
                    CAPE_POSE_UNROLL
                    for (int j = 0; j < 6; ++j)
                    {
                        x[j] = wa2[j];
                        wa4[j] = diag[j] * x[j];
                    }
                    xnorm = lm_enorm(wa4);
                    fnorm = fnorm1;
                    ++iter;
                }
                // convergence
                const bool small = fabs(actred) <= S.ftol && prered <= S.ftol && 0.5 * ratio <= 1.0;
                if (small)
                    info = 1;
                if (delta <= S.xtol * xnorm)
                    info = 2;
                if (small && info == 2)
                    info = 3;
                if (info != 0)
                    break;
                // termination and stringent tolerances
                if (nfev >= S.maxfev)
                    info = 5;
                if (fabs(actred) <= epsmch && prered <= epsmch && 0.5 * ratio <= 1.0)
                    info = 6;
                if (delta <= epsmch * xnorm)
                    info = 7;
                if (gnorm <= epsmch)
                    info = 8;
            } while (info == 0 && ratio < 0.0001);
        }
        out.fnorm = fnorm;
        out.nfev = nfev;
        out.iterations = iter - 1;
    }
    CAPE_POSE_UNROLL
    for (int j = 0; j < 6; ++j)
        out.x[j] = x[j];
    out.status = info;
    pose_from_coefficients(x, S.C, T);
    return out;
}

// ---- cape_map_pose_select: the scan of one frame's hypotheses (pose_optimization.cpp:190-235)
CAPE_POSE_FN cape_pose_selection pose_select_frame(const cape_pose_score* scores, const cape_pose_solution* solutions, int nHypotheses)
{
    cape_pose_selection S;
    S.best = -1, S.n_scanned = 0, S.n_inliers = 0, S.flags = 0u;
    S.score = 1.0, S.reserved = 0.0;
    for (int c = 0; c < 4; ++c)
        S.inlier_words[c] = 0u;
    for (int c = 0; c < 6; ++c)
        S.x[c] = 0.0;
    double maxScore = 1.0;
    int bestInliers = 0;
    for (int h = 0; h < nHypotheses; ++h)
    {
        ++S.n_scanned;
        const double score = scores[h].score;
        if (solutions[h].status <= 0 || score < 1.0)
            continue;
        const int nInliers = scores[h].n_inliers;
        if (score > maxScore || (fabs(score - maxScore) <= 0.1 && bestInliers < nInliers))
        {
            maxScore = score, bestInliers = nInliers;
            S.best = h;
        }
        if (h >= 3 && (double)bestInliers > ceil((double)scores[h].n_pairs * static_cast<double>(kPoseSelectInlierShare)))
        {
            if (h + 1 < nHypotheses)
                S.flags |= (uint32_t)CAPE_POSE_SELECT_EARLY_STOP;
            break;
        }
    }
    if (S.best >= 0)
    {
        S.score = maxScore, S.n_inliers = bestInliers;
        for (int c = 0; c < 4; ++c)
            S.inlier_words[c] = scores[S.best].inlier_words[c];
        for (int c = 0; c < 6; ++c)
            S.x[c] = solutions[S.best].x[c];
    }
    else
        S.flags |= (uint32_t)CAPE_POSE_SELECT_NO_CONSENSUS;
    return S;
}

#if defined(__HIPCC__)
// ---- the device's steps around a problem, one copy for the score, solve and varied-solve kernels
// what a lane reads of the frame's feature rows through LDS (the reasons are in the header of cape_pose_score.hip): 8 doubles and the
// kept plane per pair.  The launch's dynamic LDS is this carve's `bytes`.
struct PoseRowsLayout
{
    size_t planes, kept, bytes;
};
__host__ __device__ constexpr PoseRowsLayout pose_rows_layout()
{
    constexpr int WP = kPoseScoreMaxPairs;
    Layout l;
    PoseRowsLayout o{};
    o.planes = l.take<double>((size_t)WP * 8, 16);
    o.kept = l.take<int>((size_t)WP, 16);
    o.bytes = l.end(16);
    return o;
}
// the frame's rows into the carve, once per workgroup: lane k stages pair k, then the barrier -- every lane of the workgroup calls it
__device__ __forceinline__ void pose_rows_stage(unsigned char* smem, const cape_pose_feature* frameFeatures, int nPairs, double*& planes, int*& kept)
{
    constexpr PoseRowsLayout lay = pose_rows_layout();
    planes = carve_at<double>(smem, lay.planes);
    kept = carve_at<int>(smem, lay.kept);
    if ((int)threadIdx.x < nPairs)
        pose_rows_fill(frameFeatures[threadIdx.x], (int)threadIdx.x, planes, kept);
    __syncthreads();
}
struct DevicePlaneToCamera
{
    __device__ __forceinline__ void operator()(const double* T, const double* normal, double d, double qn[3], double& qd) const
    {
        plane_to_camera(T, normal, d, qn, qd);
    }
};
// a 96-byte solution row: eight doubles, then two 16-byte stores
__device__ __forceinline__ void store_pose_solution(cape_pose_solution* at, const cape_pose_solution& r)
{
    double* out = reinterpret_cast<double*>(at);
#pragma unroll
    for (int c = 0; c < 6; ++c)
        out[c] = r.x[c];
    out[6] = r.fnorm0, out[7] = r.fnorm;
    uint4* tail = reinterpret_cast<uint4*>(out + 8);
    tail[0] = make_uint4((unsigned)r.status, (unsigned)r.nfev, (unsigned)r.iterations, (unsigned)r.n_pairs_used);
    tail[1] = make_uint4(r.flags, 0u, 0u, 0u);
}

// what the solve and select kernels read and write (cape_pose_solve.hip)
struct PoseSolveParams
{
    const int4* frameInfo;             // per frame: n_pairs, n_invalid, flags, 0 (the pairs kernel's)
    const cape_pose_feature* features; // frames x 128
    const double* x0;                  // frames x problems x 6, or null: from the selection
    const uint32_t* subsets;           // frames x problems x 4
    const cape_pose_selection* selection; // frames, or null
    int nProblems;                     // per frame
    PoseSolveSettings settings;
    cape_pose_solution* solutions; // frames x problems
    double* poses;                 // frames x problems x 16
};
struct PoseSelectParams
{
    const cape_pose_score* scores;       // frames x hypotheses
    const cape_pose_solution* solutions; // frames x hypotheses
    int nHypotheses;
    cape_pose_selection* selection; // frames
};
#endif

} // namespace cape

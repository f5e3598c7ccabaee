// self_adjoint_eigen3 and fit_plane of csrc/cape_device.h compiled for the HOST and compared bit for bit with the oracle's functions of
// the same name, under the address and undefined-behaviour sanitizers.  A stand-alone program: tests/host/hip_stub stands in for the
// HIP runtime header, and the wave vote __any(x) is (g_force_any || (x)): every matrix is solved with the vote as one lane alone would
// cast it, and again with the vote forced, which is the SELECTED-operand body running with k1 = false -- what a lane in block [0,1] or
// [0,2] executes on the device when another lane of its wave is in block [1,2].  The families are those of tests/cell_fit_cases.py,
// drawn here in greater number.  Build and run from the repository root:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -Itests/host/hip_stub -Irgb-d-slam_amd/csrc -Ioracle \
//       -o cell_fit_algebra.exe tests/host/cell_fit_algebra.cpp oracle/cape_oracle.cpp && ./cell_fit_algebra.exe
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

using std::isinf; // the device header calls the HIP runtime's unqualified overloads
using std::isnan;
static bool g_force_any = false;
#define __any(x) (g_force_any || (x))
#include "cape_device.h"

#include "cape_oracle.hpp"

namespace co = cape_oracle;

// bit for bit, a NaN for a NaN
static bool same(const double* a, const double* b, int n)
{
    for (int i = 0; i < n; ++i)
        if (!(std::isnan(a[i]) && std::isnan(b[i])) && std::memcmp(a + i, b + i, sizeof(double)) != 0)
            return false;
    return true;
}

static std::mt19937_64 gen(20240229);
static std::normal_distribution<double> normal(0.0, 1.0);
static std::uniform_real_distribution<double> uni(0.0, 1.0);
static double decades(double lo, double hi) { return std::pow(10.0, lo + (hi - lo) * uni(gen)); }
static double sign() { return gen() % 2 ? 1.0 : -1.0; }

// lower triangle m00 m10 m11 m20 m21 m22
static void sym_normal(double* m)
{
    for (int k = 0; k < 6; ++k)
        m[k] = normal(gen) * ((k == 0 || k == 2 || k == 5) ? 2.0 : std::sqrt(2.0));
}

enum { DENSE, X_DECOUPLED, RANK1, TINY_M20, NEAR_ISOTROPIC, SCALE_LO, SCALE_HI, REPEATED, SHIFT_UNDERFLOW, TD_ZERO, NON_FINITE, N_SOLVER };
static const char* const solverNames[N_SOLVER] = {"dense", "x_decoupled", "rank1", "tiny_m20", "near_isotropic", "scale_lo",
                                                  "scale_hi", "repeated", "shift_underflow", "td_zero", "non_finite"};

static void solver_case(int family, long c, double* m)
{
    switch (family)
    {
    case DENSE:
    {
        // the scatter matrix of 24 anisotropic points, every seventh without a z extent
        double s[3] = {decades(-2, 2), decades(-2, 2), (c / N_SOLVER) % 7 == 0 ? 0.0 : decades(-2, 2)};
        for (int k = 0; k < 6; ++k)
            m[k] = 0.0;
        for (int p = 0; p < 24; ++p)
        {
            const double x = s[0] * normal(gen), y = s[1] * normal(gen), z = s[2] * normal(gen);
            m[0] += x * x; m[1] += y * x; m[2] += y * y; m[3] += z * x; m[4] += z * y; m[5] += z * z;
        }
        break;
    }
    case X_DECOUPLED:
    {
        const double a = normal(gen), b = normal(gen), c2 = normal(gen), d = normal(gen), s = decades(-3, 3);
        m[0] = normal(gen); m[1] = 0.0; m[3] = 0.0;
        if (gen() % 2)
        {
            m[2] = s * normal(gen); m[4] = s * normal(gen); m[5] = s * normal(gen); // indefinite
        }
        else
        {
            m[0] = std::fabs(m[0]) + 1e-3;
            m[2] = s * (a * a + b * b + 1e-3); m[4] = s * (a * c2 + b * d); m[5] = s * (c2 * c2 + d * d + 1e-3); // positive definite
        }
        if (m[4] == 0.0)
            m[4] = s;
        break;
    }
    case RANK1:
    {
        double v[3];
        const int kind = (int)(gen() % 3);
        for (int k = 0; k < 3; ++k)
            v[k] = kind == 1 ? (double)((int)(gen() % 19) - 9) : kind == 2 ? normal(gen) * decades(-2, 2) : normal(gen);
        m[0] = v[0] * v[0]; m[1] = v[1] * v[0]; m[2] = v[1] * v[1]; m[3] = v[2] * v[0]; m[4] = v[2] * v[1]; m[5] = v[2] * v[2];
        break;
    }
    case TINY_M20:
    {
        sym_normal(m);
        double scale = 0;
        for (int k = 0; k < 6; ++k)
            if (k != 3)
                scale = std::fmax(scale, std::fabs(m[k]));
        m[3] = sign() * scale * decades(-170, -140);
        break;
    }
    case NEAR_ISOTROPIC:
        sym_normal(m);
        for (int k = 0; k < 6; ++k)
            m[k] = 1e-8 * m[k] + ((k == 0 || k == 2 || k == 5) ? 1.0 : 0.0);
        break;
    case SCALE_LO:
    case SCALE_HI:
        sym_normal(m);
        for (int k = 0; k < 6; ++k)
            m[k] *= family == SCALE_LO ? 1e-300 : 1e300;
        break;
    case REPEATED:
    {
        const double s = decades(-6, 6), a = (c / N_SOLVER) % 9 == 0 ? 0.0 : s * normal(gen), b = s * normal(gen);
        const int kind = (int)(gen() % 4);
        m[1] = m[3] = m[4] = 0.0;
        m[0] = a; m[2] = kind == 0 || kind == 1 ? a : b; m[5] = kind == 0 || kind == 3 ? a : b;
        break;
    }
    case SHIFT_UNDERFLOW:
    {
        // |e| < 1.5e-162: e * e == 0 ; |a| < (e / eps)^2: the deflation test keeps e
        const double e = decades(-166, -163), t = e / DBL_EPSILON, a = sign() * t * t * decades(-3, -0.5);
        for (int k = 0; k < 6; ++k)
            m[k] = 0.0;
        if (gen() % 2)
        {
            m[0] = 1.0; m[2] = a; m[4] = sign() * e; // block [1,2]
        }
        else
        {
            m[0] = a; m[1] = sign() * e; m[5] = 1.0; // block [0,1]
        }
        break;
    }
    case TD_ZERO:
        m[0] = normal(gen); m[1] = 0.0; m[3] = 0.0;
        m[2] = m[5] = normal(gen) * decades(-3, 3);
        m[4] = (1.0 + uni(gen)) * sign() * decades(-3, 3);
        break;
    default:
    {
        static const double specials[3] = {std::nan(""), INFINITY, -INFINITY};
        sym_normal(m);
        m[gen() % 6] = specials[gen() % 3];
    }
    }
}

struct Sums
{
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // Sx Sy Sz Sxs Sys Szs Sxy Syz Szx
    uint32_t n = 0;
    void add(double x, double y, double z)
    {
        S[0] += x; S[1] += y; S[2] += z; S[3] += x * x; S[4] += y * y; S[5] += z * z; S[6] += x * y; S[7] += y * z; S[8] += x * z;
        ++n;
    }
    void covariance(double xx, double xy, double yy, double xz, double yz, double zz)
    {
        // Sx = Sy = Sz = 0 and n = 1: fit_plane's covariance is exactly this matrix
        S[3] = xx; S[4] = yy; S[5] = zz; S[6] = xy; S[7] = yz; S[8] = xz;
        n = 1;
    }
};

static long irand(long lo, long hi) { return lo + (long)(gen() % (uint64_t)(hi - lo + 1)); }

enum { NOISY_PLANE, DET_EDGE, HUYGENS_CLAMP, D_SIGN, SCORE_CLAMP, MIRRORED_X, N_FIT };
static const char* const fitNames[N_FIT] = {"noisy_plane", "det_edge", "huygens_clamp", "d_sign", "score_clamp", "mirrored_x"};

static void fit_case(int family, Sums& s)
{
    switch (family)
    {
    case NOISY_PLANE:
    {
        static const uint32_t counts[7] = {1, 2, 3, 200, 280, 400, 307200};
        const uint32_t want = counts[gen() % 7], k = want > 400 ? 400 : want;
        const double a = uni(gen) - 0.5, b = uni(gen) - 0.5, z0 = 800 + 2200 * uni(gen), noise = 0.5 + 4.5 * uni(gen);
        for (uint32_t p = 0; p < k; ++p)
        {
            // float32 points, float32 products widened to double, like stage A1's sums
            const float x = (float)(400 * uni(gen) - 200), y = (float)(400 * uni(gen) - 200), z = (float)(a * x + b * y + z0 + noise * normal(gen));
            s.S[0] += x; s.S[1] += y; s.S[2] += z; s.S[3] += x * x; s.S[4] += y * y; s.S[5] += z * z; s.S[6] += x * y; s.S[7] += y * z; s.S[8] += x * z;
        }
        s.n = want;
        if (want > 400)
            for (double& v : s.S)
                v *= 768.0;
        break;
    }
    case DET_EDGE:
    {
        const int kind = (int)(gen() % 5);
        const double v = gen() % 8 == 0 ? 1.0 : std::pow(2.0, 4 * uni(gen) - 2); // |det| = v eps
        if (kind == 0)
            s.covariance(1, 0, 1, 0, 0, v * DBL_EPSILON);
        else if (kind == 1)
            s.covariance(1, 0, 1, 0, std::ldexp(std::sqrt(v), -26), 0); // det = -(yz * yz)
        else if (kind == 2)
        {
            const double f = std::pow(v * DBL_EPSILON / 500.0, 1.0 / 6.0); // eight points of a box, shrunk: det of the order of eps
            for (int i = 0; i < 8; ++i)
                s.add(f * ((i & 1 ? 2 : -3) + (double)irand(-1, 1)), f * ((i & 2 ? 4 : -1) + (double)irand(-1, 1)), f * ((i & 4 ? 1 : -2) + (double)irand(-1, 1)));
        }
        else
        {
            const int k = 1 << irand(2, 6);
            const long z = irand(-1000, 1000), dir[3] = {irand(-5, 5), irand(-5, 5), irand(-5, 5)}, org[3] = {irand(-100, 100), irand(-100, 100), irand(-100, 100)};
            for (int p = 0; p < k; ++p)
            {
                const long t = irand(-60, 60);
                if (kind == 3)
                    s.add((double)irand(-60, 60), (double)irand(-60, 60), (double)z); // coplanar: zz == 0 exactly
                else
                    s.add((double)(org[0] + t * dir[0]), (double)(org[1] + t * dir[1]), (double)(org[2] + t * dir[2])); // collinear
            }
        }
        break;
    }
    case HUYGENS_CLAMP:
    {
        const int k = (int)irand(3, 400), axis = (int)(gen() % 3);
        const double big = 1e7 + (double)irand(0, 999);
        for (int p = 0; p < k; ++p)
        {
            double q[3] = {(double)irand(-50, 50), (double)irand(-50, 50), (double)irand(-50, 50)};
            q[axis] = big;
            s.add(q[0], q[1], q[2]);
        }
        break;
    }
    case D_SIGN:
    {
        const int kind = (int)(gen() % 4);
        const double a = 0.8 * uni(gen) - 0.4, b = 0.8 * uni(gen) - 0.4;
        for (int p = 0; p < 64; ++p)
        {
            const double x = (double)irand(-100, 100), y = (double)irand(-100, 100), z = std::rint(a * x + b * y + (double)irand(-3, 3));
            if (kind < 2)
                s.add(x, y, z + (kind == 0 ? 1500.0 : -1500.0));
            else
            {
                s.add(x, y, z);
                s.add(-x, -y, -z); // mirrored through the origin: Sx = Sy = Sz = 0
            }
        }
        if (kind == 3)
            for (int k = 0; k < 3; ++k)
                s.S[k] = gen() % 2 ? 0.0 : -0.0;
        break;
    }
    case SCORE_CLAMP:
    {
        // R diag(ev0, ev1, ev2) R^T, R from two plane rotations ; ev0 from 1e-7 to 1e-5
        const double ev[3] = {decades(-7, -5), 1 + 9 * uni(gen), 10 + 990 * uni(gen)};
        double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int rot = 0; rot < 3; ++rot)
        {
            const double th = 6.283185307179586 * uni(gen), cs = std::cos(th), sn = std::sin(th);
            const int i = rot % 3, j = (rot + 1) % 3;
            for (int r = 0; r < 3; ++r)
            {
                const double u = R[r][i], w = R[r][j];
                R[r][i] = cs * u - sn * w;
                R[r][j] = sn * u + cs * w;
            }
        }
        double C[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j <= i; ++j)
                C[i][j] = R[i][0] * ev[0] * R[j][0] + R[i][1] * ev[1] * R[j][1] + R[i][2] * ev[2] * R[j][2];
        s.covariance(C[0][0], C[1][0], C[1][1], C[2][0], C[2][1], C[2][2]);
        break;
    }
    default:
    {
        const int k = (int)irand(20, 199);
        const double a = uni(gen) - 0.5;
        const long z0 = irand(800, 3000);
        for (int p = 0; p < k; ++p)
        {
            const double x = (double)irand(1, 101), y = (double)irand(-100, 100), z = std::rint(a * y + (double)z0 + (double)irand(-3, 3));
            s.add(x, y, z);
            s.add(-x, y, z); // Sx = Sxy = Szx = 0 exactly: the solver works in block [1,2]
        }
    }
    }
}

int main()
{
    long bad = 0;

    const long nSolver = 2200000;
    long perFamily[N_SOLVER] = {0}, bits[N_SOLVER][8] = {{0}};
    for (long c = 0; c < nSolver; ++c)
    {
        const int family = (int)(c % N_SOLVER);
        double m[6];
        solver_case(family, c, m);
        const double lower[3][3] = {{m[0], 0, 0}, {m[1], m[2], 0}, {m[3], m[4], m[5]}};
        double ref[12], evecs[3][3];
        int iters = 0;
        unsigned trace = 0;
        co::self_adjoint_eigen3_trace(lower, ref, evecs, &iters, &trace);
        std::memcpy(ref + 3, evecs, sizeof(evecs));
        ++perFamily[family];
        for (int b = 0; b < 8; ++b)
            bits[family][b] += (trace >> b) & 1u;
        for (int forced = 0; forced < 2; ++forced)
        {
            g_force_any = forced != 0;
            cape::Eig3 e;
            cape::self_adjoint_eigen3(m[0], m[1], m[2], m[3], m[4], m[5], e);
            double got[12];
            std::memcpy(got, e.val, sizeof(e.val));
            std::memcpy(got + 3, e.q, sizeof(e.q));
            if (!same(got, ref, 12))
            {
                if (++bad <= 10)
                    std::printf("solver %s differs (vote forced: %d): %.17g %.17g %.17g %.17g %.17g %.17g\n", solverNames[family], forced, m[0], m[1], m[2], m[3], m[4], m[5]);
            }
        }
    }
    std::printf("self_adjoint_eigen3: %ld matrices, each with the vote as cast and forced\n", nSolver);
    std::printf("%-16s %8s %8s %8s %8s %8s %8s %8s %8s %8s\n", "family", "n", "[0,1]", "[0,2]", "[1,2]", "skipped", "reflect", "e2==0", "td==0", "cap");
    for (int f = 0; f < N_SOLVER; ++f)
    {
        std::printf("%-16s %8ld", solverNames[f], perFamily[f]);
        for (int b = 0; b < 8; ++b)
            std::printf(" %8ld", bits[f][b]);
        std::printf("\n");
    }
    // the families reach what they are named for (dense, of 24 points here and not of 400, enters block [1,2] now and then)
    const bool reached = bits[X_DECOUPLED][2] == perFamily[X_DECOUPLED] && bits[TD_ZERO][6] == perFamily[TD_ZERO] &&
                         bits[RANK1][2] > 0 && bits[SHIFT_UNDERFLOW][5] == perFamily[SHIFT_UNDERFLOW] && bits[TINY_M20][3] > 0 &&
                         bits[TINY_M20][4] > 0 && bits[NON_FINITE][7] > 0;
    if (!reached)
        std::printf("a family misses its branch\n");

    const long nFit = 540000;
    long fitCount[N_FIT] = {0}, planarCount[N_FIT] = {0}, block12[N_FIT] = {0};
    for (long c = 0; c < nFit; ++c)
    {
        const int family = (int)(c % N_FIT);
        Sums s;
        fit_case(family, s);
        co::PlaneSeg seg;
        seg.n = s.n;
        seg.Sx = s.S[0]; seg.Sy = s.S[1]; seg.Sz = s.S[2]; seg.Sxs = s.S[3]; seg.Sys = s.S[4]; seg.Szs = s.S[5];
        seg.Sxy = s.S[6]; seg.Syz = s.S[7]; seg.Szx = s.S[8];
        co::fit_plane(seg);
        const double ref[10] = {seg.normal[0], seg.normal[1], seg.normal[2], seg.d, seg.centroid[0], seg.centroid[1], seg.centroid[2], seg.mse, seg.score, seg.planar ? 1.0 : 0.0};
        ++fitCount[family];
        planarCount[family] += seg.planar;
        block12[family] += seg.planar && s.S[0] == 0.0 && s.S[6] == 0.0 && s.S[8] == 0.0 && s.S[7] != 0.0;
        for (int forced = 0; forced < 2; ++forced)
        {
            g_force_any = forced != 0;
            cape::PlaneFit f;
            cape::fit_plane(s.S, s.n, f);
            const double got[10] = {f.nx, f.ny, f.nz, f.d, f.cx, f.cy, f.cz, f.mse, f.score, f.planar ? 1.0 : 0.0};
            if (!same(got, ref, 10))
            {
                if (++bad <= 10)
                    std::printf("fit_plane %s differs (vote forced: %d), n = %u\n", fitNames[family], forced, s.n);
            }
        }
    }
    std::printf("fit_plane: %ld rows, each with the vote as cast and forced\n", nFit);
    for (int f = 0; f < N_FIT; ++f)
        std::printf("%-16s %8ld planar %8ld, with Sx = Sxy = Szx = 0 %8ld\n", fitNames[f], fitCount[f], planarCount[f], block12[f]);
    const bool fitReached = planarCount[DET_EDGE] > 0 && planarCount[DET_EDGE] < fitCount[DET_EDGE] && planarCount[MIRRORED_X] == fitCount[MIRRORED_X] &&
                            block12[MIRRORED_X] == fitCount[MIRRORED_X];
    if (!fitReached)
        std::printf("a fit_plane family misses its branch\n");

    std::printf("cases that differ from the oracle in a bit: %ld\n", bad);
    return bad == 0 && reached && fitReached ? 0 : 1;
}

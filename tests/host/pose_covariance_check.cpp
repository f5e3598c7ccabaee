// The rules of csrc/cape_pose_covariance.h in a stand-alone host program, for a sanitizer build (tests/test_pose_covariance_host.py
// compiles it with -fsanitize=address,undefined and runs it): the Philox known answers, the uniforms' range, the variation and its two
// edges, the Euler angles' rebuild on both sides of the fold, and whole frames -- vary into the slab layout of the device, a sample per
// iteration through pose_solve_problem on PoseVariedRows, the reduction with is_covariance_valid of host/map_tracking.cpp -- at 1, 2, 3, 64
// and 257 iterations of 3, 39 and 128 pairs, with failing samples, a refused frame and a refit row that carries its refusal.  Prints one
// line per frame; the exit status is the number of expectations missed.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "boundary_polygon.hpp"
#include "map_tracking.hpp"
#include "../../rgb-d-slam_amd/csrc/cape_pose_covariance.h"

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

uint64_t state = 0x9E3779B97F4A7C15ull;
double uniform(double lo, double hi) // (a 64-bit LCG: the same problems on every machine)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (hi - lo) * (double)(state >> 11) / 9007199254740992.0;
}

int missed = 0;
void expect(bool ok, const char* what)
{
    if (!ok)
    {
        std::printf("MISSED: %s\n", what);
        ++missed;
    }
}

constexpr int N = 128;
std::vector<double> planes((size_t)N * 8), stddevs((size_t)N * 4);
std::vector<int> kept((size_t)N);

// one frame as the twin runs it; failAt: the iteration whose first pair gets a distance deviate of 1e200 (-1: none)
cape_pose_covariance frame(int nIterations, unsigned long long lo, unsigned long long hi, const double x[6], uint64_t seed, int failFrom = -1,
                           const cape_pose_solution* solution = nullptr, double scale = 1.0, int nInvalid = 0)
{
    cape::PoseSolveSettings S;
    expect(cape::pose_solve_settings(nullptr, S), "the default parameters are accepted");
    cape::PoseSolveRows frameRows;
    frameRows.planes = planes.data(), frameRows.kept = kept.data(), frameRows.nPairs = N, frameRows.subsetLo = frameRows.subsetHi = 0ull;
    const uint32_t words[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    cape_pose_selection selection = {};
    std::memcpy(selection.inlier_words, words, sizeof words);
    const cape::PoseCovFrame F = cape::pose_cov_frame(frameRows, nInvalid, 0u, x, words, solution, solution ? &selection : nullptr);
    const size_t n = (size_t)nIterations;
    std::vector<cape::PoseCovSample> samples(n);
    std::memset(samples.data(), 0, n * sizeof(cape::PoseCovSample));
    if (F.refusal == 0)
    {
        cape::PoseVariedRows rows;
        static_cast<cape::PoseSolveRows&>(rows) = frameRows;
        rows.subsetLo = lo, rows.subsetHi = hi;
        std::vector<double> slab((size_t)N * 4 * n); // exactly the device's bytes per frame: an index past them is the sanitizer's to find
        bool first = true;
        for (size_t i = 0; i < n; ++i)
        {
            first = true;
            for (int k = 0; k < N; ++k)
            {
                if (!cape::pose_solve_takes(rows, k))
                    continue;
                double u[4], z[4], varied[4], sd[4];
                cape::pose_deviate_uniforms(seed, 3u, (uint32_t)i, (uint32_t)k, u);
                cape::pose_deviate_normals(u, z);
                for (int c = 0; c < 4; ++c)
                {
                    expect(u[c] > 0.0 && u[c] <= 1.0 && std::isfinite(z[c]), "a uniform lies in (0, 1] and its deviate is finite");
                    sd[c] = stddevs[4 * (size_t)k + c] * scale;
                }
                if (first && failFrom >= 0 && (int)i >= failFrom)
                    z[3] = 1e200;
                first = false;
                cape::pose_vary_plane(planes.data() + 8 * (size_t)k + 4, sd, z, varied);
                for (int c = 0; c < 4; ++c)
                    slab[(size_t)(4 * k + c) * n + i] = varied[c];
            }
        }
        rows.stride = n;
        for (size_t i = 0; i < n; ++i)
        {
            rows.varied = slab.data() + i;
            double T[12];
            samples[i] = cape::pose_cov_sample(cape::pose_solve_problem(rows, F.nInvalid, F.frameFlags, F.x, S, HostPlaneToCamera{}, T));
        }
    }
    const cape_pose_covariance row = cape::pose_cov_row_serial(F, samples.data(), nIterations, HostCovarianceValid{});
    std::printf("iterations %3d  status %3d  n_ok %3d  nfev %d..%d  diagonal %.6g %.6g %.6g %.6g %.6g %.6g\n", nIterations, row.status, row.n_ok,
                row.nfev_min, row.nfev_max, row.covariance[0], row.covariance[7], row.covariance[14], row.covariance[21], row.covariance[28],
                row.covariance[35]);
    return row;
}

} // namespace

int main()
{
    // ---- Philox4x32-10: the known answers
    const uint32_t kat[3][10] = {
        {0u, 0u, 0u, 0u, 0u, 0u, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
        {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
        {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
    for (const auto& row : kat)
    {
        uint32_t out[4];
        cape::philox4x32_10(row, row + 4, out);
        expect(std::memcmp(out, row + 6, sizeof out) == 0, "a Philox4x32-10 known answer");
    }
    // ---- the variation: stddev = 0 normalises and nothing else; a normal varied to 0 stays 0
    const double plane[4] = {0.6, 0.0, 0.8, 1500.0}, zero[4] = {0, 0, 0, 0}, z1[4] = {0.3, -1.2, 2.0, -0.7};
    double out[4];
    cape::pose_vary_plane(plane, zero, z1, out);
    const double norm = std::sqrt((0.6 * 0.6 + 0.0 * 0.0) + 0.8 * 0.8);
    expect(out[0] == 0.6 / norm && out[1] == 0.0 && out[2] == 0.8 / norm && out[3] == 1500.0, "stddev = 0: the plane after the normalise");
    const double up[4] = {0.0, 0.0, 1.0, 800.0}, half[4] = {0.5, 0.5, 0.5, 2.0}, back[4] = {0.0, 0.0, -2.0, 1.0};
    cape::pose_vary_plane(up, half, back, out);
    expect(out[0] == 0.0 && out[1] == 0.0 && out[2] == 0.0 && out[3] == 802.0, "a normal varied to 0 is left as it is");
    // ---- the Euler angles: Rx(a) Ry(b) Rz(c) gives the matrix back, the first angle lies in [0, pi]
    double worst = 0.0;
    for (int t = 0; t < 2000; ++t)
    {
        const double spread = t % 3 == 0 ? 0.01 : (t % 3 == 1 ? 1.0 : 30.0);
        const double x[6] = {0, 0, 0, uniform(-spread, spread), uniform(-spread, spread), uniform(-spread, spread)};
        double v[6], R[9];
        cape::pose_vector(x, v);
        cape::pose_rotation_from_coefficients(x, R);
        const double ca = std::cos(v[3]), sa = std::sin(v[3]), cb = std::cos(v[4]), sb = std::sin(v[4]), cc = std::cos(v[5]), sc = std::sin(v[5]);
        const double B[9] = {cb * cc, -cb * sc, sb, sa * sb * cc + ca * sc, -sa * sb * sc + ca * cc, -sa * cb, -ca * sb * cc + sa * sc, ca * sb * sc + sa * cc, ca * cb};
        for (int c = 0; c < 9; ++c)
            worst = std::fmax(worst, std::fabs(B[c] - R[c]));
        expect(v[3] >= 0.0 && v[3] <= 3.141592653589793, "the first angle lies in [0, pi]");
    }
    std::printf("Euler rebuild: at most %.3g\n", worst);
    expect(worst <= 1e-12, "Rx Ry Rz of the angles is the matrix");
    // ---- whole frames
    const double C[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double xTrue[6] = {120.0, -80.0, 45.0, 0.6, 0.5, -0.3};
    double Ttrue[12];
    cape::pose_from_coefficients(xTrue, C, Ttrue);
    for (int k = 0; k < N; ++k)
    {
        double n[3] = {uniform(-1, 1), uniform(-1, 1), uniform(-1, 1)};
        const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        for (double& v : n)
            v /= len;
        const double d = uniform(500.0, 4000.0);
        double qn[3], qd;
        rgbd_slam::utils::plane_to_camera(n, d, Ttrue, qn, &qd);
        double* row = planes.data() + 8 * (size_t)k;
        row[0] = qn[0], row[1] = qn[1], row[2] = qn[2], row[3] = qd + uniform(-2.0, 2.0);
        row[4] = n[0], row[5] = n[1], row[6] = n[2], row[7] = d;
        kept[k] = N - 1 - k; // (the pair order is not the kept planes')
        for (int c = 0; c < 3; ++c)
            stddevs[4 * (size_t)k + c] = uniform(1e-4, 1e-3);
        stddevs[4 * (size_t)k + 3] = uniform(0.1, 2.0);
    }
    const unsigned long long all = ~0ull, some = 0x0000007FFFFFFFFFull; // 39 pairs
    cape_pose_covariance r = frame(257, all, all, xTrue, 11);
    expect(r.status == CAPE_POSE_COVARIANCE_VALID && r.n_ok == 257 && r.covariance[0] > 0.001 && r.nfev_sum >= 257 * (int64_t)r.nfev_min, "128 pairs, 257 iterations: valid");
    r = frame(64, some, 0ull, xTrue, 12);
    expect(r.status == CAPE_POSE_COVARIANCE_VALID && r.n_ok == 64, "39 pairs, 64 iterations: valid");
    r = frame(3, 0x7ull, 0ull, xTrue, 13, 2);
    expect(r.status == CAPE_POSE_COVARIANCE_VALID && r.n_ok == 2, "three iterations, two successes: valid");
    r = frame(2, some, 0ull, xTrue, 14, 1);
    expect(r.status == CAPE_POSE_COVARIANCE_INVALID && r.n_ok == 1 && std::isnan(r.covariance[0]), "two iterations, one success: 0 / 0, invalid");
    r = frame(1, some, 0ull, xTrue, 15);
    expect(r.status == CAPE_POSE_COVARIANCE_INVALID && r.n_ok == 1, "one iteration: invalid");
    r = frame(10, some, 0ull, xTrue, 16, 4);
    expect(r.status == CAPE_POSE_COVARIANCE_TOO_MANY_FAILED && r.n_ok == 4 && r.covariance[0] == 0.0, "four successes of ten: too many failed");
    r = frame(10, some, 0ull, xTrue, 16, 5);
    expect(r.status == CAPE_POSE_COVARIANCE_VALID && r.n_ok == 5, "five successes of ten: valid");
    r = frame(2, some, 0ull, xTrue, 17, -1, nullptr, 0.0);
    bool exact = r.status == CAPE_POSE_COVARIANCE_VALID;
    for (int c = 0; c < 36; ++c)
        exact = exact && r.covariance[c] == (c % 7 == 0 ? 0.001 : 0.0);
    expect(exact, "stddev = 0, two iterations: exactly 0.001 I and valid");
    r = frame(5, 0x3ull, 0ull, xTrue, 18);
    expect(r.status == CAPE_POSE_SOLVE_TOO_FEW_PAIRS && r.n_ok == 0 && r.nfev_sum == 0, "two pairs: the frame's refusal, no sample");
    r = frame(5, some, 0ull, xTrue, 18, -1, nullptr, 1.0, 1);
    expect(r.status == CAPE_POSE_SOLVE_INVALID_FEATURE && (r.flags & CAPE_POSE_SCORE_INVALID_FEATURE), "an invalid feature refuses the frame");
    cape_pose_solution refit = {};
    std::memcpy(refit.x, xTrue, sizeof xTrue);
    refit.status = CAPE_POSE_SOLVE_NO_SELECTION;
    r = frame(5, some, 0ull, nullptr, 19, -1, &refit);
    expect(r.status == CAPE_POSE_SOLVE_NO_SELECTION, "a refit without a selection carries its refusal");
    refit.status = 0;
    r = frame(5, some, 0ull, nullptr, 19, -1, &refit);
    expect(r.status == CAPE_POSE_COVARIANCE_NO_SOLUTION, "a refit row with status 0: no solution");
    refit.status = 2;
    r = frame(5, some, 0ull, nullptr, 19, -1, &refit);
    expect(r.status == CAPE_POSE_COVARIANCE_VALID && r.n_ok == 5, "a refit row that converged: its x and the selection's words");
    std::printf("%d expectations missed\n", missed);
    return missed;
}

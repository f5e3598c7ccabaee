// The rules of csrc/cape_pose_solve.h in a stand-alone host program, for a sanitizer build (tests/test_pose_solve_host.py compiles it
// with -fsanitize=address,undefined and runs it): problems of 3, 44 and 128 pairs, the rank-deficient one that takes the pivoted qrfac
// branch and its tilted neighbour that leaves the degenerate configuration, a camera basis that is not the identity, mode = 2, the
// refusals, a NaN start and a start whose first evaluation overflows, through pose_solve_problem with utils::plane_to_camera of the
// host class, and the selection rule.  Prints one line per problem; the exit status is the number of expectations missed.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "boundary_polygon.hpp"
#include "../../rgb-d-slam_amd/csrc/cape_pose_solve.h"

namespace {

struct HostPlaneToCamera
{
    void operator()(const double* T, const double* normal, double d, double qn[3], double& qd) const
    {
        rgbd_slam::utils::plane_to_camera(normal, d, T, qn, &qd);
    }
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

cape_pose_solution solve(const std::vector<double>& planes, const std::vector<int>& kept, int nPairs, unsigned long long lo, unsigned long long hi,
                         const double x0[6], int nInvalid = 0, uint32_t frameFlags = 0, int maxfev = 400, const cape_pose_solve_params* params = nullptr)
{
    cape::PoseSolveSettings S;
    expect(cape::pose_solve_settings(params, S), "the parameters are accepted");
    S.maxfev = maxfev;
    cape::PoseSolveRows rows;
    rows.planes = planes.data(), rows.kept = kept.data(), rows.nPairs = nPairs, rows.subsetLo = lo, rows.subsetHi = hi;
    double T[12];
    const cape_pose_solution r = cape::pose_solve_problem(rows, nInvalid, frameFlags, x0, S, HostPlaneToCamera{}, T);
    std::printf("pairs %3d  status %2d  nfev %3d  iterations %2d  fnorm %.6g -> %.6g  flags %u\n", r.n_pairs_used, r.status, r.nfev, r.iterations,
                r.fnorm0, r.fnorm, r.flags);
    return r;
}

} // namespace

int main()
{
    constexpr int N = 128;
    const double C[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double xTrue[6] = {120.0, -80.0, 45.0, 1.05, -0.1, 0.07};
    double Ttrue[12];
    cape::pose_from_coefficients(xTrue, C, Ttrue);
    std::vector<double> planes((size_t)N * 8);
    std::vector<int> kept((size_t)N);
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
    }
    const double x0[6] = {150.0, -110.0, 20.0, 1.06, -0.09, 0.055};
    const unsigned long long all = ~0ull;
    cape_pose_solution r = solve(planes, kept, N, 0x7ull, 0ull, x0);
    expect(r.status >= 1 && r.status <= 3 && r.n_pairs_used == 3 && r.fnorm < r.fnorm0, "three pairs converge");
    r = solve(planes, kept, N, 0x00000FFFFFFFFFFFull, 0ull, x0);
    expect(r.status >= 1 && r.status <= 3 && r.n_pairs_used == 44, "44 pairs converge");
    r = solve(planes, kept, N, all, all, x0);
    expect(r.status >= 1 && r.status <= 3 && r.n_pairs_used == N && std::fabs(r.x[0] - xTrue[0]) < 5.0, "128 pairs converge near the true pose");
    r = solve(planes, kept, N, all, all, x0, 0, 0, 7);
    expect(r.status == 5 && r.nfev == 8, "maxfev = 7 ends with info 5 after the first trial point");
    r = solve(planes, kept, N, 0x3ull, 0ull, x0);
    expect(r.status == CAPE_POSE_SOLVE_TOO_FEW_PAIRS && r.nfev == 0 && r.x[0] == x0[0], "two pairs are refused");
    r = solve(planes, kept, N, all, all, x0, 1);
    expect(r.status == CAPE_POSE_SOLVE_INVALID_FEATURE && (r.flags & CAPE_POSE_SCORE_INVALID_FEATURE), "an invalid feature refuses the frame");
    r = solve(planes, kept, 0, all, all, x0, 0, CAPE_MATCH_EXACT_OVERFLOW);
    expect(r.status == CAPE_POSE_SOLVE_OVERFLOW, "a flagged frame is refused");
    double xNan[6] = {150.0, -110.0, 20.0, 1.06, std::nan(""), 0.055};
    r = solve(planes, kept, N, all, all, xNan);
    expect(r.status == CAPE_POSE_SOLVE_BAD_START, "a NaN start is refused");
    // three parallel map planes seen under the identity rotation: two columns of the Jacobian are exactly 0
    std::vector<double> par = {0, 0, 1, 790.0, 0, 0, 1, 800.0, 0, 0, 1, 1492.0, 0, 0, 1, 1500.0, 0, 0, 1, 2589.0, 0, 0, 1, 2600.0};
    std::vector<int> parKept = {0, 1, 2};
    const double xPar[6] = {10.0, -20.0, 0.0, 1.0, 0.0, 0.0};
    r = solve(par, parKept, 3, 0x7ull, 0ull, xPar);
    bool finite = std::isfinite(r.fnorm);
    for (double v : r.x)
        finite = finite && std::isfinite(v);
    expect((r.flags & CAPE_POSE_SOLVE_RANK_DEFICIENT) && r.status > 0 && finite && r.fnorm < r.fnorm0, "parallel planes take the qrfac branch and end finite");
    // the tilted neighbour: the detections lean by about 0.01, each its own way, so the first step leaves the identity rotation; the two
    // in-plane coordinates stay unobservable and must not move
    const double tilt[3][2] = {{0.01, 0.0}, {0.0, 0.01}, {-0.007, -0.007}};
    for (int k = 0; k < 3; ++k)
    {
        const double len = std::sqrt((tilt[k][0] * tilt[k][0] + tilt[k][1] * tilt[k][1]) + 1.0);
        par[8 * k] = tilt[k][0] / len, par[8 * k + 1] = tilt[k][1] / len, par[8 * k + 2] = 1.0 / len;
    }
    r = solve(par, parKept, 3, 0x7ull, 0ull, xPar);
    expect((r.flags & CAPE_POSE_SOLVE_RANK_DEFICIENT) && r.status >= 1 && r.status <= 3 && r.fnorm < 0.8 * r.fnorm0 && r.x[0] == xPar[0] && r.x[1] == xPar[1] &&
               std::fabs(r.x[3] - 1.0) > 1e-3,
           "the tilted parallel planes turn, converge and leave x and y alone");
    // a camera basis that is not the identity: a signed permutation turned by 0.3 about z, the detections made under it
    cape_pose_solve_params rotated = {};
    rotated.ftol = rotated.xtol = std::sqrt(DBL_EPSILON), rotated.factor = 100.0, rotated.maxfev = 400, rotated.mode = 1;
    const double co = std::cos(0.3), si = std::sin(0.3);
    const double basis[9] = {si, 0.0, co, -co, 0.0, si, 0.0, -1.0, 0.0};
    for (int c = 0; c < 9; ++c)
        rotated.camera_basis[c] = basis[c];
    cape::pose_from_coefficients(xTrue, basis, Ttrue);
    std::vector<double> turned = planes;
    for (int k = 0; k < N; ++k)
    {
        double* row = turned.data() + 8 * (size_t)k;
        double qn[3], qd;
        rgbd_slam::utils::plane_to_camera(row + 4, row[7], Ttrue, qn, &qd);
        row[0] = qn[0], row[1] = qn[1], row[2] = qn[2], row[3] = qd + uniform(-2.0, 2.0);
    }
    r = solve(turned, kept, N, 0x7ull, 0ull, x0, 0, 0, 400, &rotated);
    expect(r.status >= 1 && r.status <= 3 && r.n_pairs_used == 3 && r.fnorm < r.fnorm0, "three pairs converge under the rotated basis");
    r = solve(turned, kept, N, all, all, x0, 0, 0, 400, &rotated);
    expect(r.status >= 1 && r.status <= 3 && std::fabs(r.x[0] - xTrue[0]) < 5.0 && std::fabs(r.x[1] - xTrue[1]) < 5.0 && std::fabs(r.x[2] - xTrue[2]) < 5.0,
           "128 pairs converge near the true pose under the rotated basis");
    r = solve(turned, kept, N, all, all, x0);
    expect(!(std::fabs(r.x[0] - xTrue[0]) < 5.0 && std::fabs(r.x[1] - xTrue[1]) < 5.0), "... and not under the identity basis: the basis is read");
    // mode = 2: the scaling stays 1.  With factor = 100 the step bound never binds here, par stays 0 and the scaling never reaches the
    // step; under factor = 0.01 it binds, and mode = 2 must give another iteration than mode = 1 at the same factor
    cape_pose_solve_params bound = rotated;
    bound.factor = 0.01;
    for (int c = 0; c < 9; ++c)
        bound.camera_basis[c] = C[c];
    cape_pose_solve_params unscaled = bound;
    unscaled.mode = 2;
    const cape_pose_solution scaled = solve(planes, kept, N, 0x00000FFFFFFFFFFFull, 0ull, x0, 0, 0, 400, &bound);
    r = solve(planes, kept, N, 0x00000FFFFFFFFFFFull, 0ull, x0, 0, 0, 400, &unscaled);
    expect(scaled.status >= 1 && scaled.status <= 3 && std::fabs(scaled.x[0] - xTrue[0]) < 5.0, "44 pairs converge under a step bound that binds");
    expect(r.status >= 1 && r.status <= 3 && r.n_pairs_used == 44 && std::fabs(r.x[0] - xTrue[0]) < 5.0, "44 pairs converge with mode = 2 under that bound");
    expect(r.nfev != scaled.nfev || r.x[0] != scaled.x[0], "mode = 2 is read: another iteration than mode = 1");
    // a finite start whose residuals' squares overflow at the first evaluation
    double xFar[6] = {1e160, -110.0, 20.0, 1.06, -0.09, 0.055};
    r = solve(planes, kept, N, 0x7ull, 0ull, xFar);
    bool same = true;
    for (int j = 0; j < 6; ++j)
        same = same && r.x[j] == xFar[j];
    expect(r.status == CAPE_POSE_SOLVE_NOT_FINITE && r.nfev == 1 && r.iterations == 0 && same && std::isinf(r.fnorm0), "a start of 1e160 ends not finite at once");
    // the selection rule
    cape_pose_score scores[5] = {};
    cape_pose_solution solutions[5] = {};
    for (int h = 0; h < 5; ++h)
        scores[h].n_pairs = 10, scores[h].n_inliers = 10, scores[h].score = 10.0 / 3, solutions[h].status = 1;
    const cape_pose_selection s = cape::pose_select_frame(scores, solutions, 5);
    expect(s.best == 0 && s.n_scanned == 4 && (s.flags & CAPE_POSE_SELECT_EARLY_STOP), "ten inliers of ten pairs stop the scan at h = 3");
    std::printf("%d expectations missed\n", missed);
    return missed;
}

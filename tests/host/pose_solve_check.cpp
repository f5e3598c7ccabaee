// The rules of csrc/cape_pose_solve.h in a stand-alone host program, for a sanitizer build (tests/test_pose_solve_host.py compiles it
// with -fsanitize=address,undefined and runs it): problems of 3, 44 and 128 pairs, the rank-deficient one that takes the pivoted qrfac
// branch, the refusals and a NaN start, through pose_solve_problem with utils::plane_to_camera of the host class, and the selection
// rule.  Prints one line per problem; the exit status is the number of expectations missed.
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
                         const double x0[6], int nInvalid = 0, uint32_t frameFlags = 0, int maxfev = 400)
{
    cape::PoseSolveSettings S;
    cape::pose_solve_settings(nullptr, S);
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

// The state half's algebra of csrc/cape_map_tracking.h (det44, inverse44, kalman_update, plane_coordinate_system) compiled for the
// HOST and compared bit for bit with host/map_tracking.cpp and get_plane_coordinate_system, under the address and undefined-behaviour
// sanitizers.  A stand-alone program: tests/host/hip_stub stands in for the HIP runtime header (qualifiers as nothing, vector types
// as structs), so the device header compiles as plain C++.  Build and run from rgb-d-slam_amd/csrc:
//
//   g++ -O2 -std=c++17 -ffp-contract=off -fsanitize=address,undefined -I../../tests/host/hip_stub -I. -I../host -I../host/compat \
//       -o ../lib/map_kalman_algebra.exe ../../tests/host/map_kalman_algebra.cpp ../host/map_tracking.cpp ../host/boundary_polygon.cpp \
//       && ../lib/map_kalman_algebra.exe
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>

#include "cape_map_tracking.h"

#include "boundary_polygon.hpp"
#include "map_tracking.hpp"

namespace mt = rgbd_slam::map_tracking;

static bool same_bits(const double* a, const double* b, int n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }

int main()
{
    std::mt19937_64 gen(12345);
    std::normal_distribution<double> normal(0.0, 1.0);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    auto spd = [&](double* M, double scale) {
        double A[16];
        for (double& v : A)
            v = normal(gen);
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j)
            {
                double s = i == j ? 4.0 : 0.0;
                for (int k = 0; k < 4; ++k)
                    s += A[i * 4 + k] * A[j * 4 + k];
                M[i * 4 + j] = scale * s;
            }
    };
    const double specials[3] = {std::nan(""), INFINITY, -INFINITY};
    long counts[4] = {0, 0, 0, 0}, bad = 0;
    const long nKalman = 300000;
    for (long c = 0; c < nKalman; ++c)
    {
        double x[4], z[4], P[16], R[16];
        double nn = 0;
        for (int k = 0; k < 3; ++k)
        {
            x[k] = normal(gen);
            nn += x[k] * x[k];
        }
        for (int k = 0; k < 3; ++k)
            x[k] /= std::sqrt(nn);
        x[3] = 8000 * uni(gen) - 4000;
        for (int k = 0; k < 3; ++k)
            z[k] = x[k] + 0.01 * normal(gen);
        z[3] = x[3] + 5 * normal(gen);
        const int kind = (int)(c % 10);
        if (kind < 6)
        {
            spd(P, std::pow(10.0, 10 * uni(gen) - 7));
            spd(R, std::pow(10.0, 10 * uni(gen) - 7));
        }
        else
        {
            // around the singular threshold: det(S) = DBL_EPSILON at S = 1.2e-4 I
            const double s = std::pow(10.0, 1.5 * uni(gen) - 5);
            const double fp = 0.9 + 0.2 * uni(gen), fr = 0.9 + 0.2 * uni(gen);
            for (int k = 0; k < 16; ++k)
                P[k] = R[k] = 0.0;
            for (int k = 0; k < 4; ++k)
                P[k * 5] = s * fp, R[k * 5] = s * fr;
        }
        if (kind == 8)
        {
            double* targets[4] = {x, P, z, R};
            const int t = (int)(gen() % 4);
            targets[t][gen() % (t % 2 ? 16 : 4)] = specials[gen() % 3];
        }
        if (kind == 9)
        {
            double* M = gen() % 2 ? P : R;
            if (gen() % 2)
                M[1] += 1e-3;
            else
                M[15] = -1.0;
        }
        double xh[4] = {0, 0, 0, 0}, Ph[16] = {0}, xd[4] = {0, 0, 0, 0}, Pd[16] = {0};
        const int sh = (int)mt::kalman_update(x, P, z, R, xh, Ph);
        const int sd = cape::kalman_update(x, P, z, R, xd, Pd);
        ++counts[sh & 3];
        if (sh != sd || !same_bits(xh, xd, 4) || !same_bits(Ph, Pd, 16))
            ++bad;
        // the determinant and the inverse on their own, singular or not
        double S[16], ih[16], id[16];
        for (int k = 0; k < 16; ++k)
            S[k] = P[k] + R[k];
        const double dh = mt::det44(S), dd = cape::det44(S);
        mt::inverse44(S, dh, ih);
        cape::inverse44(S, dd, id);
        if (!same_bits(&dh, &dd, 1) || !same_bits(ih, id, 16))
            ++bad;
    }
    long accepted = 0, branch[3] = {0, 0, 0};
    const long nFrames = 300000;
    for (long c = 0; c < nFrames; ++c)
    {
        double n[3];
        const int kind = (int)(c % 8);
        if (kind < 4)
        {
            double nn = 0;
            for (int k = 0; k < 3; ++k)
            {
                n[k] = normal(gen);
                nn += n[k] * n[k];
            }
            const double scale = kind == 3 ? 1 + (gen() % 2 ? 1 : -1) * std::pow(10.0, 2 * uni(gen) - 10) : 1.0; // the 1e-9 norm check
            for (int k = 0; k < 3; ++k)
                n[k] = n[k] / std::sqrt(nn) * scale;
        }
        else if (kind < 7)
        {
            // within 0.1 of a boundary of select_correct_transform, on either side
            const double a = 0.45 * uni(gen), b = a + 0.1 + (gen() % 2 ? 1 : -1) * std::pow(10.0, 16 * uni(gen) - 17);
            const double c2 = 1 - a * a - b * b;
            const int p = (int)(gen() % 6);
            static const int perms[6][3] = {{0, 1, 2}, {1, 0, 2}, {2, 0, 1}, {0, 2, 1}, {1, 2, 0}, {2, 1, 0}};
            n[perms[p][0]] = a * (gen() % 2 ? 1 : -1);
            n[perms[p][1]] = b * (gen() % 2 ? 1 : -1);
            n[perms[p][2]] = std::sqrt(c2 > 0 ? c2 : 0) * (gen() % 2 ? 1 : -1);
        }
        else
        {
            for (int k = 0; k < 3; ++k)
                n[k] = gen() % 4 == 0 ? specials[gen() % 3] : (double)(int)(gen() % 3) - 1.0;
        }
        double hx[6] = {0, 0, 0, 0, 0, 0}, dx[6] = {0, 0, 0, 0, 0, 0};
        bool hok = true;
        try
        {
            const auto axes = rgbd_slam::utils::get_plane_coordinate_system(rgbd_slam::vector3(n[0], n[1], n[2]));
            for (int k = 0; k < 3; ++k)
                hx[k] = axes.first[k], hx[3 + k] = axes.second[k];
        }
        catch (const std::invalid_argument&)
        {
            hok = false;
        }
        const bool dok = cape::plane_coordinate_system(n, dx, dx + 3);
        accepted += hok;
        if (hok)
            for (int k = 0; k < 3; ++k)
                branch[k] += hx[k] == 0.0;
        if (hok != dok || (hok && !same_bits(hx, dx, 6)))
            ++bad;
    }
    std::printf("kalman_update / det44 / inverse44: %ld cases, status OK %ld, INVALID_INPUT %ld, SINGULAR %ld, INVALID_OUTPUT %ld\n", nKalman, counts[0],
                counts[1], counts[2], counts[3]);
    std::printf("plane_coordinate_system: %ld normals, %ld accepted, x axis without component 0 / 1 / 2: %ld / %ld / %ld\n", nFrames, accepted, branch[0],
                branch[1], branch[2]);
    std::printf("cases that differ from the host in a bit: %ld\n", bad);
    return bad == 0 ? 0 : 1;
}

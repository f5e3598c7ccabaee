// The four MINPACK blocks of csrc/cape_pose_solve.h -- lm_rwupdt, lm_qrfac, lm_qrsolv, lm_lmpar -- behind extern "C" wrappers, so that
// tests/test_pose_lm_blocks_host.py can hand each of them inputs of its own and compare with numpy.  The test compiles this file with
// g++ into a shared object and loads it with ctypes.  Matrices are 6 x 6, row-major, as the header keeps them.
#include "../../rgb-d-slam_amd/csrc/cape_pose_solve.h"

extern "C" {

// fold the m rows of J (m x 6) with right-hand sides f into r (zeroed here) and qtf (zeroed here), row after row
void pose_lm_rwupdt(int m, const double* J, const double* f, double* r, double* qtf)
{
    for (int c = 0; c < 36; ++c)
        r[c] = 0.0;
    for (int j = 0; j < 6; ++j)
        qtf[j] = 0.0;
    for (int k = 0; k < m; ++k)
        cape::lm_rwupdt(r, J + 6 * k, qtf, f[k]);
}

void pose_lm_qrfac(double* a, int* ipvt, double* rdiag, double* acnorm) { cape::lm_qrfac(a, ipvt, rdiag, acnorm); }

void pose_lm_qrsolv(double* r, const double* pdiag, const double* qtb, double* z, double* sdiag) { cape::lm_qrsolv(r, pdiag, qtb, z, sdiag); }

// returns par; x in the variables' own order
double pose_lm_lmpar(double* r, const int* ipvt, const double* diag, const double* qtb, double delta, double par, double* x)
{
    cape::lm_lmpar(r, ipvt, diag, qtb, delta, par, x);
    return par;
}

// lm_gather and lm_scatter on their own: out[j] = v[ipvt[j]]; out[ipvt[j]] = v[j]
void pose_lm_gather(const double* v, const int* ipvt, double* out) { cape::lm_gather(v, ipvt, out); }
void pose_lm_scatter(const double* v, const int* ipvt, double* out) { cape::lm_scatter(v, ipvt, out); }
}

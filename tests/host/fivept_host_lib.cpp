// Host build of the sequential five-point statement (coloc_amd/csrc/fivept.h) as a tiny shared library for the tests: the
// checker for the wave-cooperative GPU form (coloc_amd/csrc/fivept_wave.h).  Test infrastructure only.
//
// fpt_host_solve_ws also hands the workspace back (the null-space basis, the action matrix, the eigenvalues as the iteration
// left them and whether each had stopped, every root's (x, y, z) as it left each stage, its candidate and its `valid`), which
// is what tools/fivept_attribution.py attributes a lost solution to a stage from; fpt_host_eig runs the eigenvalue stage alone.
#include <string.h>

struct FptTrace { double xyz[10][3][3]; int reached[10][3]; };
static thread_local FptTrace g_trace;
#define FPT_ROOT_HOOK(k, stage, x, y, z) \
    (g_trace.xyz[k][stage][0] = (x), g_trace.xyz[k][stage][1] = (y), g_trace.xyz[k][stage][2] = (z), g_trace.reached[k][stage] = 1)
#include "../../coloc_amd/csrc/fivept.h"

static thread_local FptWorkspace ws;

extern "C" int fpt_host_solve(const double* q1, const double* q2, double* E_out /* 90 */)
{
    double a[5][2], b[5][2];
    for (int p = 0; p < 5; ++p) for (int c = 0; c < 2; ++c) { a[p][c] = q1[2 * p + c]; b[p][c] = q2[2 * p + c]; }
    memset(&ws, 0, sizeof ws);
    memset(&g_trace, 0, sizeof g_trace);
    const int n = fivept_solve(a, b, E_out, ws);
    for (int i = 9 * n; i < 90; ++i) E_out[i] = 0.0;
    return n;
}

// the same solve, and: EE (36), Ax (100), zr, zi (10 each), zdone (10), xyz (10 roots x 3 stages x 3), reached (10 x 3),
// cand (10 x 9), valid (10)
extern "C" int fpt_host_solve_ws(const double* q1, const double* q2, double* E_out, double* EE, double* Ax, double* zr, double* zi, int* zdone,
                                 double* xyz, int* reached, double* cand, int* valid)
{
    const int n = fpt_host_solve(q1, q2, E_out);
    memcpy(EE, ws.EE, sizeof ws.EE);
    memcpy(Ax, ws.Ax, sizeof ws.Ax);
    memcpy(zr, ws.zr, sizeof ws.zr);
    memcpy(zi, ws.zi, sizeof ws.zi);
    memcpy(zdone, ws.zdone, sizeof ws.zdone);
    memcpy(xyz, g_trace.xyz, sizeof g_trace.xyz);
    memcpy(reached, g_trace.reached, sizeof g_trace.reached);
    for (int k = 0; k < 10; ++k) { memcpy(cand + 9 * k, ws.root[k].cand, 9 * sizeof(double)); valid[k] = ws.root[k].valid; }
    return n;
}

// The eigenvalue stage alone: Hessenberg form, balancing and the Ehrlich-Aberth iteration on a 10 x 10 matrix (row-major), as
// fivept_solve runs them.  Returns 0 where the solver would give up (a zero matrix).
extern "C" int fpt_host_eig(const double* A, double* zr, double* zi, int* zdone)
{
    memset(&ws, 0, sizeof ws);
    for (int i = 0; i < 100; ++i) ws.hr[i / 10][i % 10] = A[i];
    if (!fpt_eigenvalues10_seq(ws)) return 0;
    memcpy(zr, ws.zr, sizeof ws.zr);
    memcpy(zi, ws.zi, sizeof ws.zi);
    memcpy(zdone, ws.zdone, sizeof ws.zdone);
    return 1;
}

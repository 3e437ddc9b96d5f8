// Host build of the SO(3) helpers and the 6x6 solve of the pose refinement (coloc_amd/csrc/so3.h) as a tiny shared library for the
// tests (tests/so3_host.py, tests/test_so3_host.py): the statements pnp_refine_kernel runs, compiled by g++ without contraction.  libm's
// sincos / atan2 stand in for the device's, so results agree with the device to rounding, not bit for bit.  Test infrastructure only.
#include <cmath>
#include "../../coloc_amd/csrc/so3.h"

extern "C" {

void so3_host_rodrigues(const double* w, double* R) { clc::rodrigues(w, R); }

void so3_host_log(const double* R, double* w) { clc::log_so3(R, w); }

// dR: 3 x 9 (dR/dw_k row-major); R = rodrigues(w) as the kernel passes it
void so3_host_d_rodrigues(const double* w, const double* R, double* dR) { clc::d_rodrigues(w, R, reinterpret_cast<double (*)[9]>(dR)); }

double so3_host_d_rodrigues_entry(const double* w, const double* R, int k, int e) { return clc::d_rodrigues_entry(w, R, k, e); }

int so3_host_packed6(int i, int j) { return clc::packed6(i, j); }

// Ap: packed upper triangle (21); returns 1 when the damped matrix was accepted as SPD
int so3_host_solve6(const double* Ap, const double* g, double lambda, double* d) { return clc::solve6(Ap, g, lambda, d) ? 1 : 0; }

// inv: 6 x 6 row-major, column c written on success only
int so3_host_invert6_column(const double* Ap, int c, double* inv) { return clc::invert6_column(Ap, c, inv) ? 1 : 0; }

}

// so3.h -- rotation helpers and the 6x6 solve of the single-pose refinement (pose_lm.h: pnp_refine_kernel, pose_prior_kernel), host + device inline
// so that the tests can run the very statements of the kernel on the CPU (tests/host/so3_host_lib.cpp) against a 50-digit
// reference (tests/pose_mp.py).  fp64 throughout, contraction off: an expression is the IEEE operations written here, in this order.
//
//   rodrigues / log_so3        exp and log of SO(3), angle-axis w <-> row-major R
//   d_rodrigues(_entry)        dR/dw_k, all 27 entries or one of them (27 lanes in parallel)
//   packed6 / solve6 / invert6_column   damped 6x6 Cholesky solve on the packed upper triangle; columns of the inverse
#ifndef CLC_SO3_H
#define CLC_SO3_H

#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define SO3_HD __host__ __device__ __forceinline__
#else
#define SO3_HD static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace clc {

SO3_HD void rodrigues(const double* w, double* R)
{
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (th2 < 1e-24) {
        R[0] = 1; R[1] = -w[2]; R[2] = w[1]; R[3] = w[2]; R[4] = 1; R[5] = -w[0]; R[6] = -w[1]; R[7] = w[0]; R[8] = 1;
        return;
    }
    const double th = sqrt(th2), ith = 1.0 / th;
    double s, c;
    sincos(th, &s, &c);                 // one shared range reduction
    const double k0 = w[0] * ith, k1 = w[1] * ith, k2 = w[2] * ith, v = 1.0 - c;
    R[0] = c + k0 * k0 * v;      R[1] = k0 * k1 * v - k2 * s; R[2] = k0 * k2 * v + k1 * s;
    R[3] = k1 * k0 * v + k2 * s; R[4] = c + k1 * k1 * v;      R[5] = k1 * k2 * v - k0 * s;
    R[6] = k2 * k0 * v - k1 * s; R[7] = k2 * k1 * v + k0 * s; R[8] = c + k2 * k2 * v;
}

// angle-axis of a rotation matrix (row-major).  With a = vee(R - R^T) = 2 sin(th) k and c = (tr R - 1) / 2 = cos(th):
//   angle  th = atan2(|a| / 2, c)   -- well conditioned on all of [0, pi] (acos(c) loses half the digits next to 0 and pi);
//   axis   from a while cos(th) >= -1/2 (|a| >= sqrt(3): no cancellation worth speaking of), beyond that from the symmetric
//          part S = (R + R^T) / 2 = c I + (1 - c) k k^T: row p of S - c I, p the largest diagonal entry, is (1 - c) k_p k -- a
//          multiple of k with |k_p| >= 1/sqrt(3) -- and its sign is the one that agrees with a.  At an exact half turn a = 0 and
//          both signs are the same rotation.
SO3_HD void log_so3(const double* R, double* w)
{
    const double ax = R[7] - R[5], ay = R[2] - R[6], az = R[3] - R[1];
    const double c = 0.5 * ((R[0] + R[4] + R[8]) - 1.0);
    const double s2 = ax * ax + ay * ay + az * az;
    if (c >= -0.5) {
        if (s2 < 1e-280) { w[0] = 0.5 * ax; w[1] = 0.5 * ay; w[2] = 0.5 * az; return; }     // th / sin(th) = 1 to the last bit
        const double n = sqrt(s2);
        const double f = atan2(0.5 * n, c) / n;
        w[0] = f * ax; w[1] = f * ay; w[2] = f * az;
        return;
    }
    const double th = atan2(0.5 * sqrt(s2), c);
    const int p = (R[0] >= R[4] && R[0] >= R[8]) ? 0 : (R[4] >= R[8] ? 1 : 2);
    double v0 = 0.5 * (R[3 * p] + R[p]), v1 = 0.5 * (R[3 * p + 1] + R[3 + p]), v2 = 0.5 * (R[3 * p + 2] + R[6 + p]);
    if (p == 0) v0 -= c; else if (p == 1) v1 -= c; else v2 -= c;
    double f = th / sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    if (v0 * ax + v1 * ay + v2 * az < 0.0) f = -f;
    w[0] = f * v0; w[1] = f * v1; w[2] = f * v2;
}

// The four scalar functions of th^2 that dR/dw is made of, R = I + a [w]x + b [w]x^2:
//   a = sin(th) / th, b = (1 - cos(th)) / th^2, a1 = (da/dth) / th = (th cos(th) - sin(th)) / th^3,
//   b1 = (db/dth) / th = (th sin(th) - 2 (1 - cos(th))) / th^4.
// Below th = 1/2 the closed forms cancel (a1 loses 2 log10(1/th) digits, b1 twice that), so the Taylor series are summed instead
// (alternating; the first term left out is below 1e-17 of the sum at th = 1/2).
SO3_HD void so3_coefficients(const double th2, double* a, double* b, double* a1, double* b1)
{
    if (th2 < 0.25) {
        const double x = th2;
        *a = 1.0 + x * (-1.0 / 6 + x * (1.0 / 120 + x * (-1.0 / 5040 + x * (1.0 / 362880 + x * (-1.0 / 39916800 + x * (1.0 / 6227020800.0 + x * (-1.0 / 1307674368000.0)))))));
        *b = 0.5 + x * (-1.0 / 24 + x * (1.0 / 720 + x * (-1.0 / 40320 + x * (1.0 / 3628800 + x * (-1.0 / 479001600 + x * (1.0 / 87178291200.0 + x * (-1.0 / 20922789888000.0)))))));
        *a1 = -1.0 / 3 + x * (1.0 / 30 + x * (-1.0 / 840 + x * (1.0 / 45360 + x * (-1.0 / 3991680 + x * (1.0 / 518918400 + x * (-1.0 / 93405312000.0))))));
        *b1 = -1.0 / 12 + x * (1.0 / 180 + x * (-1.0 / 6720 + x * (1.0 / 453600 + x * (-1.0 / 47900160 + x * (1.0 / 7264857600.0 + x * (-1.0 / 1494484992000.0))))));
        return;
    }
    const double th = sqrt(th2);
    double s, c;
    sincos(th, &s, &c);
    const double v = 1.0 - c;
    *a = s / th;
    *b = v / th2;
    *a1 = (th * c - s) / (th * th2);
    *b1 = (th * s - 2.0 * v) / (th2 * th2);
}

// Entry (i, j) of dR/dw_k from the coefficients above:
//   dR/dw_k = a G_k + a1 w_k [w]x + b (e_k w^T + w e_k^T - 2 w_k I) + b1 w_k (w w^T - th^2 I),     G_k = [e_k]x.
// No division by th^2 and no difference I - R: the form  (w_k [w]x + [w x (I - R) e_k]x) R / th^2  (Gallego & Yezzi 2015) that stood
// here is the same function, but it carries the rounding of R divided by th (1e-8 at th = 1e-8) and needed a th -> 0 branch that is
// itself only first order (G_k, off by th).  tests/test_so3_host.py holds this one to the 50-digit derivative.
SO3_HD double so3_d_entry(const double* w, const double th2, const double a, const double b, const double a1, const double b1,
                          const int k, const int i, const int j)
{
    // [v]x entry (i, j): 0 on the diagonal, else +-v_m with m the third index
    const int m = 3 - i - j;                                                  // the third index when i != j
    const double sgn = (i == j) ? 0.0 : (((j - i + 3) % 3 == 1) ? -1.0 : 1.0);    // [v]x(0,1) = -v2, (1,2) = -v0, (2,0) = -v1
    const double Wij = (i == j) ? 0.0 : sgn * w[m];
    const double Gij = (i == j || m != k) ? 0.0 : sgn;
    const double dij = (i == j) ? 1.0 : 0.0;
    const double sym = (i == k ? w[j] : 0.0) + (j == k ? w[i] : 0.0) - 2.0 * w[k] * dij;
    return ((a * Gij + a1 * w[k] * Wij) + b * sym) + b1 * w[k] * (w[i] * w[j] - th2 * dij);
}

// dR/dw_k, k = 0..2 (R is not needed by this form; the parameter stays for the call sites)
SO3_HD void d_rodrigues(const double* w, const double* R, double (*dR)[9])
{
    (void)R;
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double a, b, a1, b1;
    so3_coefficients(th2, &a, &b, &a1, &b1);
    for (int k = 0; k < 3; ++k)
        for (int e = 0; e < 9; ++e) dR[k][e] = so3_d_entry(w, th2, a, b, a1, b1, k, e / 3, e - 3 * (e / 3));
}

// One entry of the same derivative: element e (0..8) of dR/dw_k, for 27 lanes working in parallel.
SO3_HD double d_rodrigues_entry(const double* w, const double* R, const int k, const int e)
{
    (void)R;
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double a, b, a1, b1;
    so3_coefficients(th2, &a, &b, &a1, &b1);
    const int i = e / 3;
    return so3_d_entry(w, th2, a, b, a1, b1, k, i, e - 3 * i);
}

// index of entry (i, j), j >= i, in the packed upper triangle the normal-equation sums are kept in (row-major: 00 01 .. 05 11 ..)
SO3_HD constexpr int packed6(const int i, const int j) { return i <= j ? i * 6 - i * (i - 1) / 2 + (j - i) : j * 6 - j * (j - 1) / 2 + (i - j); }

// Cholesky solve of the damped 6x6 system (A + lambda diag(A)) d = g, A given as its PACKED upper triangle (21 values, read
// where they lie -- LDS: a 6 x 6 register copy costs 72 VGPRs in the one lane that runs this); returns false if not SPD.
// "Not SPD" is RELATIVE: a pivot that is not above 64 ulp of the diagonal entry it was subtracted from is rounding, not
// curvature -- a rank-deficient matrix (one or two points) otherwise passes with a pivot of 1e-18 and an inverse of 1e18.
SO3_HD bool solve6(const double* Ap, const double* g, double lambda, double* d)
{
    // fully unrolled (compile-time indices) so that L, y stay in registers instead of scratch
    double L[36], Linv[6];    // Linv[i] = 1 / L[i][i]: six divisions instead of twenty-seven
    bool spd = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double aij = Ap[packed6(i, j)];
            const double diag = aij + (i == j ? lambda * (aij > 1e-12 ? aij : 1e-12) : 0.0);
            double sum = diag;
#pragma unroll
            for (int k = 0; k < j; ++k) sum -= L[6 * i + k] * L[6 * j + k];
            if (i == j) {
                const bool pos = sum > 0.0 && sum > 7.105427357601002e-15 * diag;      // 64 * 2^-53
                spd = spd && pos;
                L[6 * i + i] = sqrt(pos ? sum : 1.0);
                Linv[i] = 1.0 / L[6 * i + i];
            }
            else L[6 * i + j] = sum * Linv[j];
        }
    }
    if (!spd) return false;
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double sum = g[i];
#pragma unroll
        for (int k = 0; k < i; ++k) sum -= L[6 * i + k] * y[k];
        y[i] = sum * Linv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double sum = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) sum -= L[6 * k + i] * d[k];
        d[i] = sum * Linv[i];
    }
    return true;
}

// column c of A^-1 (A SPD, packed upper triangle): called by six lanes in parallel, one column each
SO3_HD bool invert6_column(const double* A, int c, double* inv)
{
    double e[6], col[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) e[r] = r == c ? 1.0 : 0.0;
    if (!solve6(A, e, 0.0, col)) return false;
#pragma unroll
    for (int r = 0; r < 6; ++r) inv[6 * r + c] = col[r];
    return true;
}

} // namespace clc

#endif

// ba_math.h -- the fp64 statements of the map's bundle adjustment (include/coloc_hip.h: clc_ba_dev and the _grow_ba_ compositions;
// reference include/coloc/Refiner.hpp:47-239 under intrinsics NONE, extrinsics ADJUST_ALL, structure ADJUST_ALL), host + device inline
// and written ONCE, as map_math.h is: the kernels of map_ba.hip and the host build the tests hold them to (tests/host/ba_lib.cpp) run
// the very same statements.  Contraction off: an expression is the IEEE operations written here, in this order.
//
//   cost        1/2 sum rho(|r|^2) over the observations, r = x_ud - (f hnormalized(R X + t) + pp), rho / w of pnp_refine_kernel (pnp.hip)
//   parameters  per camera [angle-axis | t] (so3.h), per landmark X; nothing is held constant
//   step        Levenberg-Marquardt through the Schur complement on the landmarks:
//                 per point  V = sum w Jp^T Jp (3 x 3), g_t = sum w Jp^T r, W_c = w Jc^T Jp (6 x 3 per observing camera)
//                 per camera U = sum w Jc^T Jc, g_c = sum w Jc^T r
//                 S = U + lambda diag(U) - sum_t W (V + lambda diag V)^-1 W^T,  S d_c = g_c - sum_t W (V + lambda diag V)^-1 g_t
//                 d_X = (V + lambda diag V)^-1 (g_t - sum_c W_c^T d_c)
//   J is the Jacobian of the PROJECTION (the residual's is -J), so the right-hand sides above are descent directions.
#ifndef CLC_BA_MATH_H
#define CLC_BA_MATH_H

#include <math.h>
#include <stdint.h>

#include "so3.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define BA_HD __host__ __device__ __forceinline__
#else
#define BA_HD static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace clc {

constexpr int kBaCams = 8;                   // CLC_MAX_BATCH
constexpr int kBaDim = 6 * kBaCams;          // the reduced system's unknowns at most
constexpr int kBaRec = 21;                   // one observation's record: Ju 6 | Jv 6 | Pu 3 | Pv 3 | w | r0 | r1
constexpr int kBaPoint = 9;                  // one point's record: (V + lambda diag V)^-1 packed 00 01 02 11 12 22 | that times g_t
constexpr int kBaChunk = 128;                // points (in compacted order) whose sums one workgroup forms; the chunks are added in order
constexpr double kBaLambda0 = 1e-4, kBaLambdaFloor = 1e-12, kBaLambdaStop = 1e10;

// The cameras at one iterate: K = { focal, ppx, ppy }, R = exp(w) row-major, t, dR/dw_k, and the slot of a masked camera in the reduced
// system (its rank among the masked cameras; -1: not adjusted, its observations do not count).
struct BaCams {
    double K[kBaCams][3], par[kBaCams][6], R[kBaCams][9], dR[kBaCams][3][9];
    int32_t slot[kBaCams];
    int32_t n_cams, n_slots;
};

// par -> R, dR of camera c
BA_HD void ba_camera_update(BaCams& cams, const int c)
{
    rodrigues(cams.par[c], cams.R[c]);
    d_rodrigues(cams.par[c], cams.R[c], cams.dR[c]);
}

// [R|t] (3 x 4 row-major) -> par
BA_HD void ba_camera_from_Rt(const double* Rt, double* par)
{
    const double R[9] = { Rt[0], Rt[1], Rt[2], Rt[4], Rt[5], Rt[6], Rt[8], Rt[9], Rt[10] };
    log_so3(R, par);
    par[3] = Rt[3]; par[4] = Rt[7]; par[5] = Rt[11];
}

BA_HD void ba_camera_to_Rt(const double* R, const double* par, double* Rt)
{
    for (int i = 0; i < 3; ++i) { Rt[4 * i] = R[3 * i]; Rt[4 * i + 1] = R[3 * i + 1]; Rt[4 * i + 2] = R[3 * i + 2]; Rt[4 * i + 3] = par[3 + i]; }
}

// the bits of obs that count: cameras below n_cams with a slot
BA_HD uint32_t ba_obs_bits(const BaCams& cams, const uint32_t obs)
{
    uint32_t b = 0;
    for (int c = 0; c < cams.n_cams; ++c)
        if (((obs >> c) & 1u) && cams.slot[c] >= 0) b |= 1u << c;
    return b;
}

// rho(s) and the weight rho'(s): s inside a^2, 2 a sqrt(s) - a^2 and a / sqrt(s) in the tail
BA_HD void ba_huber(const double sq, const double a, double* rho, double* w)
{
    *rho = sq; *w = 1.0;
    if (sq > a * a) {
        const double r = sqrt(sq);
        *rho = 2.0 * a * r - a * a;
        *w = a / r;
    }
}

// Xc = R X + t and r = x - (f Xc.hnormalized() + pp).  false: the depth is not positive (r is not written)
BA_HD bool ba_residual(const double* K, const double* R, const double* par, const double* X, const double* x, double* Xc, double* r)
{
    for (int i = 0; i < 3; ++i) Xc[i] = ((R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2]) + par[3 + i];
    if (!(Xc[2] > 0.0)) return false;
    const double iz = 1.0 / Xc[2];
    r[0] = x[0] - (K[0] * (Xc[0] * iz) + K[1]);
    r[1] = x[1] - (K[0] * (Xc[1] * iz) + K[2]);
    return true;
}

// One point's cost 1/2 sum rho over the cameras of `bits` in ascending order; +inf where a depth is not positive
BA_HD double ba_point_cost(const BaCams& cams, const uint32_t bits, const double* X, const double* x, const double a)
{
    double cost = 0.0;
    for (int c = 0; c < cams.n_cams; ++c) {
        if (!((bits >> c) & 1u)) continue;
        double Xc[3], r[2], rho, w;
        if (!ba_residual(cams.K[c], cams.R[c], cams.par[c], X, x + 2 * c, Xc, r)) return INFINITY;
        ba_huber(r[0] * r[0] + r[1] * r[1], a, &rho, &w);
        cost += 0.5 * rho;
    }
    return cost;
}

// The record of one observation: the projection's Jacobians in the camera's six parameters (Ju, Jv) and in X (Pu, Pv), weight, residual
BA_HD bool ba_observation(const double* K, const double* R, const double (*dR)[9], const double* par, const double* X, const double* x, const double a,
                          double* rec)
{
    double Xc[3], r[2], rho, w;
    if (!ba_residual(K, R, par, X, x, Xc, r)) return false;
    ba_huber(r[0] * r[0] + r[1] * r[1], a, &rho, &w);
    const double iz = 1.0 / Xc[2], xn = Xc[0] * iz, yn = Xc[1] * iz;
    const double pu0 = K[0] * iz, pu2 = -(K[0] * xn) * iz, pv1 = K[0] * iz, pv2 = -(K[0] * yn) * iz;      // d(pixel) / d(Xc)
    double* Ju = rec; double* Jv = rec + 6; double* Pu = rec + 12; double* Pv = rec + 15;
    for (int k = 0; k < 3; ++k) {
        const double d0 = (dR[k][0] * X[0] + dR[k][1] * X[1]) + dR[k][2] * X[2];
        const double d2 = (dR[k][6] * X[0] + dR[k][7] * X[1]) + dR[k][8] * X[2];
        const double d1 = (dR[k][3] * X[0] + dR[k][4] * X[1]) + dR[k][5] * X[2];
        Ju[k] = pu0 * d0 + pu2 * d2;
        Jv[k] = pv1 * d1 + pv2 * d2;
        Pu[k] = pu0 * R[k] + pu2 * R[6 + k];
        Pv[k] = pv1 * R[3 + k] + pv2 * R[6 + k];
    }
    Ju[3] = pu0; Ju[4] = 0.0; Ju[5] = pu2;
    Jv[3] = 0.0; Jv[4] = pv1; Jv[5] = pv2;
    rec[18] = w; rec[19] = r[0]; rec[20] = r[1];
    return true;
}

// W[i][a] = w (Ju[i] Pu[a] + Jv[i] Pv[a]); U[i][j] = w (Ju[i] Ju[j] + Jv[i] Jv[j]); g_c[i] = w (Ju[i] r0 + Jv[i] r1)
BA_HD double ba_W(const double* rec, const int i, const int a) { return rec[18] * (rec[i] * rec[12 + a] + rec[6 + i] * rec[15 + a]); }
BA_HD double ba_U(const double* rec, const int i, const int j) { return rec[18] * (rec[i] * rec[j] + rec[6 + i] * rec[6 + j]); }
BA_HD double ba_gc(const double* rec, const int i) { return rec[18] * (rec[i] * rec[19] + rec[6 + i] * rec[20]); }

// packed symmetric 3 x 3: 00 01 02 11 12 22
BA_HD constexpr int ba_p3(const int i, const int j) { return i <= j ? (i == 0 ? j : (i == 1 ? 2 + j : 5)) : (j == 0 ? i : (j == 1 ? 2 + i : 5)); }

// (V + lambda diag V)^-1 by Cholesky, packed.  false: not positive definite by solve6's RELATIVE rule (a pivot not above 64 ulp of the
// diagonal entry it was subtracted from is rounding).  A point seen once has a V of rank 2: only the damping makes it invertible.
BA_HD bool ba_invert3(const double* V, const double lambda, double* inv)
{
    const double d0 = V[0] + lambda * (V[0] > 1e-12 ? V[0] : 1e-12), d1 = V[3] + lambda * (V[3] > 1e-12 ? V[3] : 1e-12),
                 d2 = V[5] + lambda * (V[5] > 1e-12 ? V[5] : 1e-12);
    const double tiny = 7.105427357601002e-15;                       // 64 * 2^-53
    if (!(d0 > 0.0)) return false;
    const double l00 = sqrt(d0), i00 = 1.0 / l00;
    const double l10 = V[1] * i00, l20 = V[2] * i00;
    const double p1 = d1 - l10 * l10;
    if (!(p1 > 0.0 && p1 > tiny * d1)) return false;
    const double l11 = sqrt(p1), i11 = 1.0 / l11;
    const double l21 = (V[4] - l20 * l10) * i11;
    const double p2 = (d2 - l20 * l20) - l21 * l21;
    if (!(p2 > 0.0 && p2 > tiny * d2)) return false;
    const double l22 = sqrt(p2), i22 = 1.0 / l22;
    // M = L^-1 (lower), inverse = M^T M
    const double m10 = -(l10 * i00) * i11, m21 = -(l21 * i11) * i22, m20 = -(l20 * i00 + l21 * m10) * i22;
    inv[0] = (i00 * i00 + m10 * m10) + m20 * m20;
    inv[1] = m10 * i11 + m20 * m21;
    inv[2] = m20 * i22;
    inv[3] = i11 * i11 + m21 * m21;
    inv[4] = m21 * i22;
    inv[5] = i22 * i22;
    return true;
}

// The build of one point at the current iterate: the records of its observations (rec: n_cams x kBaRec, written where the bit is set),
// and pt = { (V + lambda diag V)^-1, that times g_t }.  *gmax: the largest |g_t| component.  false: a depth that is not positive, or a V
// that the damping does not make positive definite (pt is zeros then; the step counts as a failed factorisation).
BA_HD bool ba_point_build(const BaCams& cams, const uint32_t bits, const double* X, const double* x, const double a, const double lambda,
                          double* rec, double* pt, double* gmax)
{
    double V[6] = { 0, 0, 0, 0, 0, 0 }, g[3] = { 0, 0, 0 };
    bool ok = true;
    for (int c = 0; c < cams.n_cams; ++c) {
        if (!((bits >> c) & 1u)) continue;
        double* rc = rec + (size_t)kBaRec * c;
        if (!ba_observation(cams.K[c], cams.R[c], cams.dR[c], cams.par[c], X, x + 2 * c, a, rc)) {
            for (int i = 0; i < kBaRec; ++i) rc[i] = 0.0;
            ok = false;
            continue;
        }
        const double w = rc[18];
        const double* Pu = rc + 12; const double* Pv = rc + 15;
        for (int i = 0; i < 3; ++i) {
            for (int j = i; j < 3; ++j) V[ba_p3(i, j)] += w * (Pu[i] * Pu[j] + Pv[i] * Pv[j]);
            g[i] += w * (Pu[i] * rc[19] + Pv[i] * rc[20]);
        }
    }
    *gmax = fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2])));
    ok = ok && ba_invert3(V, lambda, pt);
    if (!ok) { for (int i = 0; i < kBaPoint; ++i) pt[i] = 0.0; return false; }
    for (int i = 0; i < 3; ++i) pt[6 + i] = (pt[ba_p3(i, 0)] * g[0] + pt[ba_p3(i, 1)] * g[1]) + pt[ba_p3(i, 2)] * g[2];
    return true;
}

// ---- the reduced system's entries ---------------------------------------------------------------------------------------------------
// The sums a chunk of points leaves, n = 6 n_slots: [ upper triangle of U - sum W Vd^-1 W^T, row-major, n (n + 1) / 2 | right-hand side
// n | diag(U) n | g_c n | failed points | largest |g_t| ]
BA_HD constexpr int ba_tri(const int n) { return n * (n + 1) / 2; }
BA_HD constexpr int ba_entries(const int n) { return ba_tri(n) + 3 * n + 2; }
BA_HD int ba_tri_index(const int n, const int a, const int b) { return a * n - a * (a - 1) / 2 + (b - a); }      // a <= b

// entry e of the triangle -> (row a, column b), a <= b
BA_HD void ba_tri_entry(const int n, const int e, int* a, int* b)
{
    int row = 0, left = e;
    while (left >= n - row) { left -= n - row; ++row; }
    *a = row; *b = row + left;
}

// sum_ab W_A[i][a] inv[a][b] W_B[j][b]
BA_HD double ba_schur_term(const double* recA, const int i, const double* recB, const int j, const double* inv)
{
    const double w0 = ba_W(recA, i, 0), w1 = ba_W(recA, i, 1), w2 = ba_W(recA, i, 2);
    const double y0 = (w0 * inv[0] + w1 * inv[1]) + w2 * inv[2], y1 = (w0 * inv[1] + w1 * inv[3]) + w2 * inv[4],
                 y2 = (w0 * inv[2] + w1 * inv[4]) + w2 * inv[5];
    return (y0 * ba_W(recB, j, 0) + y1 * ba_W(recB, j, 1)) + y2 * ba_W(recB, j, 2);
}

// Entry e < ba_tri(n) + 3 n (the two tail entries are not sums of this kind) named once: kind 0 the triangle's (row a of camera ca,
// column b of camera cb), 1 the right-hand side, 2 diag(U), 3 g_c (row a of camera ca).  cam_of_slot: slot -> camera.
struct BaEntry { int32_t kind, ca, cb, i, j; };
BA_HD BaEntry ba_entry(const int n, const int e, const int32_t* cam_of_slot)
{
    const int tri = ba_tri(n);
    if (e < tri) {
        int a, b;
        ba_tri_entry(n, e, &a, &b);
        return BaEntry{ 0, cam_of_slot[a / 6], cam_of_slot[b / 6], a % 6, b % 6 };
    }
    const int a = (e - tri) % n;
    return BaEntry{ 1 + (e - tri) / n, cam_of_slot[a / 6], cam_of_slot[a / 6], a % 6, a % 6 };
}
// what ONE point adds to it
BA_HD double ba_entry_term(const BaEntry& en, const uint32_t bits, const double* rec, const double* pt)
{
    if (!((bits >> en.ca) & 1u) || !((bits >> en.cb) & 1u)) return 0.0;
    const double* ra = rec + (size_t)kBaRec * en.ca; const double* rb = rec + (size_t)kBaRec * en.cb;
    if (en.kind == 0) {
        const double s = ba_schur_term(ra, en.i, rb, en.j, pt);
        return en.ca == en.cb ? ba_U(ra, en.i, en.j) - s : -s;
    }
    if (en.kind == 2) return ba_U(ra, en.i, en.i);
    const double g = ba_gc(ra, en.i);
    if (en.kind == 3) return g;
    return g - ((ba_W(ra, en.i, 0) * pt[6] + ba_W(ra, en.i, 1) * pt[7]) + ba_W(ra, en.i, 2) * pt[8]);
}

// d_X of one point from the cameras' steps dc (slot-major, 6 each): Vd^-1 g_t - Vd^-1 sum_c W_c^T d_c, the cameras in ascending order
BA_HD void ba_point_delta(const BaCams& cams, const uint32_t bits, const double* rec, const double* pt, const double* dc, double* dX)
{
    double s[3] = { 0, 0, 0 };
    for (int c = 0; c < cams.n_cams; ++c) {
        if (!((bits >> c) & 1u)) continue;
        const double* rc = rec + (size_t)kBaRec * c; const double* d = dc + 6 * cams.slot[c];
        for (int a = 0; a < 3; ++a) {
            double v = 0.0;
            for (int i = 0; i < 6; ++i) v += ba_W(rc, i, a) * d[i];
            s[a] += v;
        }
    }
    for (int a = 0; a < 3; ++a) dX[a] = pt[6 + a] - ((pt[ba_p3(a, 0)] * s[0] + pt[ba_p3(a, 1)] * s[1]) + pt[ba_p3(a, 2)] * s[2]);
}

// ---- the dense solve of the reduced system, S full row-major with leading dimension kBaDim, the LOWER triangle in and L out ----------
// A[i][j] - sum_{k<j} L[i][k] L[j][k], k ascending: the one statement of an entry (the device runs the rows of a column side by side)
BA_HD double ba_chol_sum(const double* S, const int i, const int j)
{
    double sum = S[i * kBaDim + j];
    for (int k = 0; k < j; ++k) sum -= S[i * kBaDim + k] * S[j * kBaDim + k];
    return sum;
}
// the pivot of column j from its sum: > 0 and above 64 ulp of the diagonal entry, else 0 (not positive definite)
BA_HD double ba_chol_pivot(const double sum, const double diag) { return (sum > 0.0 && sum > 7.105427357601002e-15 * diag) ? sqrt(sum) : 0.0; }

// L y = g, L^T d = y by one lane
BA_HD void ba_chol_substitute(const double* L, const int n, const double* g, double* d)
{
    double y[kBaDim];
    for (int i = 0; i < n; ++i) {
        double sum = g[i];
        for (int k = 0; k < i; ++k) sum -= L[i * kBaDim + k] * y[k];
        y[i] = sum / L[i * kBaDim + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double sum = y[i];
        for (int k = i + 1; k < n; ++k) sum -= L[k * kBaDim + i] * d[k];
        d[i] = sum / L[i * kBaDim + i];
    }
}

// The whole solve in one thread (the host statement): sys = the summed entries of ba_entries(n); S: kBaDim x kBaDim scratch.
// false: not positive definite.
BA_HD void ba_system_fill(const double* sys, const int n, const double lambda, double* S)
{
    for (int a = 0; a < n; ++a)
        for (int b = a; b < n; ++b) {
            double v = sys[ba_tri_index(n, a, b)];
            if (a == b) { const double u = sys[ba_tri(n) + n + a]; v += lambda * (u > 1e-12 ? u : 1e-12); }
            S[b * kBaDim + a] = v;
        }
}
static inline bool ba_system_solve(const double* sys, const int n, const double lambda, double* S, double* d)
{
    ba_system_fill(sys, n, lambda, S);
    for (int j = 0; j < n; ++j) {
        const double diag = S[j * kBaDim + j];
        const double p = ba_chol_pivot(ba_chol_sum(S, j, j), diag);
        if (p == 0.0) return false;
        S[j * kBaDim + j] = p;
        for (int i = j + 1; i < n; ++i) S[i * kBaDim + j] = ba_chol_sum(S, i, j) / p;
    }
    ba_chol_substitute(S, n, sys + ba_tri(n), d);
    return true;
}

// ---- Levenberg-Marquardt's bookkeeping, pnp_refine_kernel's schedule ------------------------------------------------------------------
struct BaLm {
    double lambda, cost, cost_initial;
    int32_t it, max_it, status, n_accepted;        // status -1: running
    double ftol;
};
enum { BA_RUNNING = -1, BA_OK = 0, BA_MAX_ITERATIONS = 1, BA_STALLED = 2, BA_BAD_START = 3, BA_EMPTY = 4 };

// before a step: 1 = go on, 0 = the run has ended
BA_HD bool ba_lm_may_step(BaLm& lm)
{
    if (lm.status != BA_RUNNING) return false;
    if (!(lm.it < lm.max_it)) { lm.status = BA_MAX_ITERATIONS; return false; }
    return true;
}
// the gradient test at the current iterate (gradient tolerance 1e-8, as pnp_refine_kernel)
BA_HD bool ba_lm_gradient_small(const BaLm& lm, const double gmax) { return gmax < 1e-8 * fmax(1.0, lm.cost); }
// a factorisation that failed: reject
BA_HD void ba_lm_failed(BaLm& lm)
{
    lm.lambda *= 10.0;
    if (lm.lambda > kBaLambdaStop) { lm.status = BA_STALLED; return; }
    ++lm.it;
}
// a trial evaluated: dn = |step|^2, pn = |parameters|^2.  true: the trial is the new iterate
BA_HD bool ba_lm_trial(BaLm& lm, const double new_cost, const double dn, const double pn)
{
    if (sqrt(dn) < 1e-8 * (sqrt(pn) + 1e-8)) { lm.status = BA_OK; return false; }      // parameter tolerance: the step is not taken
    if (new_cost < lm.cost) {                        // (false for a cost that is not finite: +inf behind a camera, NaN)
        const double rel = (lm.cost - new_cost) / fmax(lm.cost, 1e-300);
        lm.cost = new_cost;
        lm.lambda = fmax(lm.lambda * 0.1, kBaLambdaFloor);
        ++lm.it; ++lm.n_accepted;
        if (rel < lm.ftol) lm.status = BA_OK;
        return true;
    }
    lm.lambda *= 10.0;
    if (lm.lambda > kBaLambdaStop) { lm.status = BA_STALLED; return false; }
    ++lm.it;
    return false;
}

} // namespace clc

#endif

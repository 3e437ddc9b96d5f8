// sim3_math.h -- the fp64 statements of the 3-D similarity that aligns a replaced map to the old one, host + device inline and written
// ONCE, as map_math.h and guided_math.h are: the a-contrario round (acransac.hip, kAcrSimilarity), the refit launch behind it and the host build
// the tests hold them to (tests/host/sim3_host_lib.cpp) run the very same statements, so the device has the host's bits by construction.
// IEEE +, -, *, / and sqrt only, contraction off: an expression is the operations written here, in this order.
//
// Convention throughout: the similarity maps NEW to OLD, X_old ~ s R X_new + t.  A model is A = [sR | t], 12 doubles, 3 x 4 row-major
// (the resection's model stride).  This is the project's own statement: the reference's matchMaps keeps every match
// (RobustMatcher.hpp:348-362, its homography filter commented out, :247-293) and colocUtils.hpp:184-211 averages distance ratios.
#ifndef CLC_SIM3_MATH_H
#define CLC_SIM3_MATH_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define SIM3_HD __host__ __device__ __forceinline__
#else
#define SIM3_HD static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace clc {

// the one literal of the degeneracy guard of a minimal sample, and the refit's rank guard
#define CLC_SIM3_DEGENERATE 1e-12
#define CLC_SIM3_RANK 1e-12
// inliers per partial sum of the refit
static constexpr int kSim3Chunk = 128;

SIM3_HD bool sim3_finite(const double v) { return v - v == 0.0; }
// the NaN that marks an empty slot: one bit pattern on host and device (0.0 / 0.0 has the sign bit set on x86)
SIM3_HD double sim3_nan() { const uint64_t u = 0x7ff8000000000000ull; double d; memcpy(&d, &u, 8); return d; }
SIM3_HD double sim3_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
SIM3_HD void sim3_cross(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// One cloud of a minimal sample: the orthonormal triad F = [u1 u2 u3] (columns) of e1 = p1 - p0 and e1 x e2, e2 = p2 - p0 (e1 and
// e1 x e2 are orthogonal as they stand: Gram-Schmidt on them is their normalisation; u2 = u3 x u1), the centroid ((p0 + p1) + p2) / 3
// and S = sum |p_i - centroid|^2.  false: |e1 x e2|^2 <= 1e-12 |e1|^2 |e2|^2, the three points are (nearly) collinear or coincide.
SIM3_HD bool sim3_triad(const double* p0, const double* p1, const double* p2, double* u1, double* u2, double* u3, double* mean, double* S)
{
    double e1[3], e2[3], c[3];
    for (int q = 0; q < 3; ++q) { e1[q] = p1[q] - p0[q]; e2[q] = p2[q] - p0[q]; }
    sim3_cross(e1, e2, c);
    const double n1 = sim3_dot(e1, e1), n2 = sim3_dot(e2, e2), cc = sim3_dot(c, c);
    if (!(cc > (CLC_SIM3_DEGENERATE * n1) * n2)) return false;
    const double l1 = sqrt(n1), lc = sqrt(cc);
    for (int q = 0; q < 3; ++q) { u1[q] = e1[q] / l1; u3[q] = c[q] / lc; }
    sim3_cross(u3, u1, u2);
    double acc = 0.0;
    for (int q = 0; q < 3; ++q) mean[q] = ((p0[q] + p1[q]) + p2[q]) / 3.0;
    const double* p[3] = { p0, p1, p2 };
    for (int i = 0; i < 3; ++i) {
        const double d0 = p[i][0] - mean[0], d1 = p[i][1] - mean[1], d2 = p[i][2] - mean[2];
        const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
        acc = i == 0 ? dd : acc + dd;
    }
    *S = acc;
    return true;
}

// A = [sR | t] from s, R (3 x 3 row-major) and the two centroids: A = s R, t = ybar - (s R) xbar
SIM3_HD void sim3_compose(const double s, const double* R, const double* xbar, const double* ybar, double* A)
{
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) A[4 * r + q] = s * R[3 * r + q];
        A[4 * r + 3] = ybar[r] - ((A[4 * r] * xbar[0] + A[4 * r + 1] * xbar[1]) + A[4 * r + 2] * xbar[2]);
    }
}

// The minimal solver: three correspondences x[i] (new) -> y[i] (old), 3 doubles each.  R = F_y F_x^T, s = sqrt(S_y / S_x),
// t = ybar - s R xbar.  A degenerate sample (either cloud) fills the slot with NaNs, as the other solvers mark an empty root.
SIM3_HD bool sim3_minimal(const double* x0, const double* x1, const double* x2, const double* y0, const double* y1, const double* y2, double* A)
{
    double ux[3][3], uy[3][3], mx[3], my[3], Sx = 0.0, Sy = 0.0;
    const bool okx = sim3_triad(x0, x1, x2, ux[0], ux[1], ux[2], mx, &Sx);
    const bool oky = sim3_triad(y0, y1, y2, uy[0], uy[1], uy[2], my, &Sy);
    if (!okx || !oky) {
        for (int e = 0; e < 12; ++e) A[e] = sim3_nan();
        return false;
    }
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) R[3 * r + q] = (uy[0][r] * ux[0][q] + uy[1][r] * ux[1][q]) + uy[2][r] * ux[2][q];
    sim3_compose(sqrt(Sy / Sx), R, mx, my, A);
    return true;
}

// |y - A [x; 1]|^2, every row ((A0 X + A1 Y) + A2 Z) + A3 (the style of the resection's residual)
SIM3_HD double sim3_residual(const double* A, const double* x, const double* y)
{
    const double d0 = y[0] - (((A[0] * x[0] + A[1] * x[1]) + A[2] * x[2]) + A[3]);
    const double d1 = y[1] - (((A[4] * x[0] + A[5] * x[1]) + A[6] * x[2]) + A[7]);
    const double d2 = y[2] - (((A[8] * x[0] + A[9] * x[1]) + A[10] * x[2]) + A[11]);
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// s, R, t of a minimal model: s = sqrt((A00^2 + A10^2) + A20^2), R = A[:, :3] / s, t = A[:, 3]
SIM3_HD void sim3_from_model(const double* A, double* s, double* R, double* t)
{
    const double sc = sqrt((A[0] * A[0] + A[4] * A[4]) + A[8] * A[8]);
    *s = sc;
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) R[3 * r + q] = A[4 * r + q] / sc;
        t[r] = A[4 * r + 3];
    }
}

// The a-contrario alpha of a residual that is a squared distance in R^3: the unit ball over the bounding box of the old points,
// ((4 / 3) pi) / V with V = (ex ey) ez.  box: { min x, y, z, max x, y, z }.
SIM3_HD double sim3_box_volume(const double* box) { return ((box[3] - box[0]) * (box[4] - box[1])) * (box[5] - box[2]); }
SIM3_HD bool sim3_volume_ok(const double V) { return V > 0.0 && sim3_finite(V); }
SIM3_HD double sim3_alpha0(const double V) { return ((4.0 / 3.0) * 3.14159265358979323846) / V; }
// the acceptance rule of HIP_SfM_Localizer::Localize: a meaningful model with more than 2.5 x 3 inliers
SIM3_HD bool sim3_accepted(const int valid, const int n_inliers) { return valid >= 0 && 2 * n_inliers > 15; }

// ---- the refit: Umeyama's least-squares similarity over an inlier list -----------------------------------------------------------------
// The inliers are taken in ascending correspondence index (list: the indices, null = 0 .. n - 1); entries [b, e) of the list are ONE
// partial sum, added left to right.  First pass: the six coordinate sums; second: the 3 x 3 sum of (y - ybar)(x - xbar)^T (row = y) and
// sum |x - xbar|^2 behind it.  A partial is kSim3Chunk consecutive inliers; the partials are then added left to right (sim3_add).
SIM3_HD void sim3_sum_points(const double* x, const double* y, const int32_t* list, const int b, const int e, double* out6)
{
    for (int q = 0; q < 6; ++q) out6[q] = 0.0;
    for (int i = b; i < e; ++i) {
        const int k = list ? list[i] : i;
        for (int q = 0; q < 3; ++q) { out6[q] += x[3 * k + q]; out6[3 + q] += y[3 * k + q]; }
    }
}
SIM3_HD void sim3_sum_cov(const double* x, const double* y, const int32_t* list, const int b, const int e, const double* xbar, const double* ybar,
                          double* out10)
{
    for (int q = 0; q < 10; ++q) out10[q] = 0.0;
    for (int i = b; i < e; ++i) {
        const int k = list ? list[i] : i;
        double dx[3], dy[3];
        for (int q = 0; q < 3; ++q) { dx[q] = x[3 * k + q] - xbar[q]; dy[q] = y[3 * k + q] - ybar[q]; }
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) out10[3 * r + q] += dy[r] * dx[q];
        out10[9] += (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2];
    }
}
// acc (+)= part over `len` entries; first: acc = part
SIM3_HD void sim3_add(double* acc, const double* part, const int len, const bool first)
{
    for (int q = 0; q < len; ++q) acc[q] = first ? part[q] : acc[q] + part[q];
}

// The 3 x 3 SVD M = U diag(sigma) V^T by a one-sided (Hestenes) Jacobi on M's columns with the sweep rule of map_math.h's null_vector4:
// at most 30 cyclic sweeps, a pair is rotated unless gamma == 0 or |gamma| <= 1e-16 sqrt(alpha beta), a sweep that rotates nothing ends
// it.  M (row-major) is overwritten by U diag(sigma); the columns are then ordered by descending norm (compare-exchanges (0,1), (0,2),
// (1,2), strict '<').  sigma[j] = the column norms.
SIM3_HD void sim3_svd3(double* M, double* V, double* sigma)
{
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int k = 0; k < 3; ++k) {
                    alpha += M[3 * k + p] * M[3 * k + p];
                    beta += M[3 * k + q] * M[3 * k + q];
                    gamma += M[3 * k + p] * M[3 * k + q];
                }
                if (gamma == 0.0 || fabs(gamma) <= 1e-16 * sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < 3; ++k) {
                    const double mp = M[3 * k + p], mq = M[3 * k + q];
                    M[3 * k + p] = c * mp - s * mq;
                    M[3 * k + q] = s * mp + c * mq;
                    const double vp = V[3 * k + p], vq = V[3 * k + q];
                    V[3 * k + p] = c * vp - s * vq;
                    V[3 * k + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double n2[3];
    for (int j = 0; j < 3; ++j) n2[j] = (M[j] * M[j] + M[3 + j] * M[3 + j]) + M[6 + j] * M[6 + j];
    const int pa[3] = { 0, 0, 1 }, pb[3] = { 1, 2, 2 };
    for (int w = 0; w < 3; ++w) {
        const int a = pa[w], b = pb[w];
        if (n2[a] < n2[b]) {
            const double tn = n2[a]; n2[a] = n2[b]; n2[b] = tn;
            for (int k = 0; k < 3; ++k) {
                const double tm = M[3 * k + a]; M[3 * k + a] = M[3 * k + b]; M[3 * k + b] = tm;
                const double tv = V[3 * k + a]; V[3 * k + a] = V[3 * k + b]; V[3 * k + b] = tv;
            }
        }
    }
    for (int j = 0; j < 3; ++j) sigma[j] = sqrt(n2[j]);
}
SIM3_HD double sim3_det3(const double* M)
{
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Umeyama's solution from the sums of n inliers: sum6 = { sum x, sum y }; cov10 = the second pass's sums about xbar = sum x / n,
// ybar = sum y / n.  M = cov / n = U diag(sigma) V^T; R = U diag(1, 1, d) V^T, d = sign(det U det V); s = ((sigma1 + sigma2) + d sigma3)
// / (S_x / n); t = ybar - s R xbar.  The third column of U is taken as u1 x u2 (the normalised third column of U diag(sigma) is noise
// where sigma3 is small -- a planar cloud); the sign of det U is the sign of that column against u1 x u2, + where it vanishes.
// false (the refit is refused, outputs untouched): sigma2 <= 1e-12 sigma1, or an output that is not finite.
SIM3_HD bool sim3_umeyama(const int n, const double* xbar, const double* ybar, const double* cov10, double* s, double* R, double* t, double* A)
{
    const double dn = (double)n;
    double M[9], V[9], sg[3];
    for (int q = 0; q < 9; ++q) M[q] = cov10[q] / dn;
    const double var_x = cov10[9] / dn;
    sim3_svd3(M, V, sg);
    if (!(sg[1] > CLC_SIM3_RANK * sg[0])) return false;
    double u1[3], u2[3], u3[3], m3[3];
    for (int k = 0; k < 3; ++k) { u1[k] = M[3 * k] / sg[0]; u2[k] = M[3 * k + 1] / sg[1]; m3[k] = M[3 * k + 2]; }
    sim3_cross(u1, u2, u3);
    const double sdU = sim3_dot(m3, u3) < 0.0 ? -1.0 : 1.0, sdV = sim3_det3(V) < 0.0 ? -1.0 : 1.0;
    const double d = sdU * sdV;
    double Rr[9], tr[3], Ar[12];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) Rr[3 * r + q] = (u1[r] * V[3 * q] + u2[r] * V[3 * q + 1]) + (sdV * u3[r]) * V[3 * q + 2];
    const double sr = ((sg[0] + sg[1]) + d * sg[2]) / var_x;
    sim3_compose(sr, Rr, xbar, ybar, Ar);
    for (int r = 0; r < 3; ++r) tr[r] = Ar[4 * r + 3];
    bool fin = sim3_finite(sr) && sr > 0.0;
    for (int q = 0; q < 12; ++q) fin = fin && sim3_finite(Ar[q]);
    for (int q = 0; q < 9; ++q) fin = fin && sim3_finite(Rr[q]);
    if (!fin) return false;
    *s = sr;
    for (int q = 0; q < 9; ++q) R[q] = Rr[q];
    for (int q = 0; q < 3; ++q) t[q] = tr[q];
    for (int q = 0; q < 12; ++q) A[q] = Ar[q];
    return true;
}

// the whole refit, sequentially: what the refit launch computes with one thread per partial sum.  n >= 1 inliers.
SIM3_HD bool sim3_refit(const double* x, const double* y, const int32_t* list, const int n, double* s, double* R, double* t, double* A)
{
    double sum6[6], part[10], cov10[10], xbar[3], ybar[3];
    for (int b = 0; b < n; b += kSim3Chunk) {
        sim3_sum_points(x, y, list, b, b + kSim3Chunk < n ? b + kSim3Chunk : n, part);
        sim3_add(sum6, part, 6, b == 0);
    }
    for (int q = 0; q < 3; ++q) { xbar[q] = sum6[q] / (double)n; ybar[q] = sum6[3 + q] / (double)n; }
    for (int b = 0; b < n; b += kSim3Chunk) {
        sim3_sum_cov(x, y, list, b, b + kSim3Chunk < n ? b + kSim3Chunk : n, xbar, ybar, part);
        sim3_add(cov10, part, 10, b == 0);
    }
    return sim3_umeyama(n, xbar, ybar, cov10, s, R, t, A);
}

// ---- applying the similarity -----------------------------------------------------------------------------------------------------------
// a point of the new frame in the old one: s R X + t, rows as in sim3_residual (A = [sR | t])
SIM3_HD void sim3_apply_point(const double* A, const double* X, double* out)
{
    const double o0 = ((A[0] * X[0] + A[1] * X[1]) + A[2] * X[2]) + A[3];
    const double o1 = ((A[4] * X[0] + A[5] * X[1]) + A[6] * X[2]) + A[7];
    const double o2 = ((A[8] * X[0] + A[9] * X[1]) + A[10] * X[2]) + A[11];
    out[0] = o0; out[1] = o1; out[2] = o2;
}
// a camera [R_c | t_c] (3 x 4 row-major, rewritten) of the new frame in the old one: R_c' = R_c R^T, t_c' = s t_c - R_c' t; its centre
// moves to s R C + t
SIM3_HD void sim3_apply_pose(const double s, const double* R, const double* t, double* Rt)
{
    double Rc[9];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) Rc[3 * r + q] = (Rt[4 * r] * R[3 * q] + Rt[4 * r + 1] * R[3 * q + 1]) + Rt[4 * r + 2] * R[3 * q + 2];
    for (int r = 0; r < 3; ++r) {
        const double tc = s * Rt[4 * r + 3] - ((Rc[3 * r] * t[0] + Rc[3 * r + 1] * t[1]) + Rc[3 * r + 2] * t[2]);
        for (int q = 0; q < 3; ++q) Rt[4 * r + q] = Rc[3 * r + q];
        Rt[4 * r + 3] = tc;
    }
}

} // namespace clc

#endif

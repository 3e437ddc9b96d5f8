// inter_math.h -- the per-element fp64 statements of the inter-camera step (reference include/coloc/coloc.hpp:296-340), host + device
// inline and written ONCE: inter_geometry.cpp (clc_inter_pose_batch) and the kernels of inter_dev.hip (clc_inter_pose_batch_dev) call the
// very same statements, so the device has the host's bits by construction, and tests/test_inter_geometry_host.py pins the host build
// (tests/host/inter_geometry_lib.cpp) bit for bit on the CPU.  Contraction off: an expression is the IEEE operations written here, in this
// order.  What differs between the callers -- containers, loop order, sort against radix select, the vote by ballot, who sums -- is theirs.
#ifndef CLC_INTER_MATH_H
#define CLC_INTER_MATH_H

#include <math.h>
#include "../../include/coloc_hip.h"         // CLC_INTER_OK / CLC_INTER_NO_SCALE

#if defined(__HIPCC__) || defined(__HIP__)
#define INTER_HD __host__ __device__ __forceinline__
#else
#define INTER_HD static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace clc {

// pixel -> normalised camera plane for K = { fx, skew, cx; 0, fy, cy; 0, 0, 1 }.  The device's cameras have skew = 0: the product stays.
INTER_HD void normalise_px(const double fx, const double skew, const double cx, const double fy, const double cy, const double x, const double y, double* n)
{
    n[1] = (y - cy) / fy;
    n[0] = (x - cx - skew * n[1]) / fx;
}

// The depths along the two rays of correspondence (n1, n2) under motion Rt = [R|t] (3 x 4 row-major) that bring them closest,
// min | l1 R n1 - l2 n2 + t |^2 in closed form (OpenMVG's TriangulateDLT differs from it by less than the measurement noise).
// *depth1 = l1; true: the point lies in front of both cameras.
INTER_HD bool two_ray_depths(const double* Rt, const double* n1, const double* n2, double* depth1)
{
    const double p[3] = { n1[0], n1[1], 1.0 }, b[3] = { n2[0], n2[1], 1.0 };
    const double t[3] = { Rt[3], Rt[7], Rt[11] };
    double a[3];
    for (int r = 0; r < 3; ++r) a[r] = Rt[4 * r] * p[0] + Rt[4 * r + 1] * p[1] + Rt[4 * r + 2] * p[2];
    const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
    const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
    const double at = a[0] * t[0] + a[1] * t[1] + a[2] * t[2], bt = b[0] * t[0] + b[1] * t[1] + b[2] * t[2];
    double det = aa * bb - ab * ab;
    if (fabs(det) < 1e-18) det = 1e-18;
    const double d1 = (-at * bb + bt * ab) / det, d2 = (-at * ab + bt * aa) / det;
    *depth1 = d1;
    return d1 > 0.0 && d2 > 0.0;
}

// The depth-ratio screen's number for one common feature: |R_s X_g + t_s| / |X_t|, global map point X_g seen from the source camera
// (Rs = its [R|t]) against temporary map point Xt_k (source camera's frame, unit baseline).
INTER_HD double depth_ratio(const double* Rs, const double* Xg, const double* Xt_k)
{
    double xs[3];
    for (int r = 0; r < 3; ++r) xs[r] = Rs[4 * r] * Xg[0] + Rs[4 * r + 1] * Xg[1] + Rs[4 * r + 2] * Xg[2] + Rs[4 * r + 3];
    const double ng = sqrt(xs[0] * xs[0] + xs[1] * xs[1] + xs[2] * xs[2]);
    const double nt = sqrt(Xt_k[0] * Xt_k[0] + Xt_k[1] * Xt_k[1] + Xt_k[2] * Xt_k[2]);
    return ng / (nt > 1e-12 ? nt : 1e-12);
}

// One term of the scale rule over consecutive common features (colocUtils.hpp:201-204: float dist1 = (X12 - X11).norm(); float dist2 =
// (X22 - X21).norm(); scale += dist1 / dist2), g = global map points, t = temporary map points.  A term the d2 > 1e-9f guard drops comes
// back as -1 (a ratio of norms is never negative): the sum skips terms < 0.
INTER_HD double scale_term(const double* g0, const double* g1, const double* t0, const double* t1)
{
    const float d1 = (float)sqrt((g1[0] - g0[0]) * (g1[0] - g0[0]) + (g1[1] - g0[1]) * (g1[1] - g0[1]) + (g1[2] - g0[2]) * (g1[2] - g0[2]));
    const float d2 = (float)sqrt((t1[0] - t0[0]) * (t1[0] - t0[0]) + (t1[1] - t0[1]) * (t1[1] - t0[1]) + (t1[2] - t0[2]) * (t1[2] - t0[2]));
    return d2 > 1e-9f ? (double)(d1 / d2) : -1.0;
}

// the mean of the `good` terms that were summed (in list order: the bits depend on it); *scale = 0 unless CLC_INTER_OK comes back
INTER_HD int scale_from_sum(const double sum, const unsigned good, double* scale)
{
    *scale = 0.0;
    if (good == 0) return CLC_INTER_NO_SCALE;
    const double s = sum / (double)good;
    if (!(s > 0.0) || !isfinite(s)) return CLC_INTER_NO_SCALE;
    *scale = s;
    return CLC_INTER_OK;
}

// Entry (r, q) of the destination's [R|t] through the source: X_d = R_rel X_s + s t_rel, X_s = R_s X_w + t_s (Rb, tb: the relative
// pose the chirality vote chose; Rs: the source's [R|t], 3 x 4)
INTER_HD double compose_pose_entry(const double* Rb, const double* tb, const double* Rs, const double scale, const int r, const int q)
{
    const double v = Rb[3 * r] * Rs[q] + Rb[3 * r + 1] * Rs[4 + q] + Rb[3 * r + 2] * Rs[8 + q];
    return q < 3 ? v : v + scale * tb[r];
}

// a temporary map point in world coordinates: X_w = R_s^T (s X_tmp - t_s)
INTER_HD void world_point(const double* Rs, const double scale, const double* Xt_k, double* out)
{
    const double v[3] = { scale * Xt_k[0] - Rs[3], scale * Xt_k[1] - Rs[7], scale * Xt_k[2] - Rs[11] };
    for (int q = 0; q < 3; ++q) out[q] = Rs[q] * v[0] + Rs[4 + q] * v[1] + Rs[8 + q] * v[2];
}

} // namespace clc

#endif

// map_math.h -- the per-point fp64 statements of the map's seed triangulation (reference include/coloc/Reconstructor.hpp:185-257) and of
// the grow step behind it (:329-414), host + device inline and written ONCE, as inter_math.h is: seed_triangulate_kernel (map_build.hip),
// grow_kernel (map_grow.hip) and the host builds the tests hold them to (tests/host/map_math_lib.cpp, tests/host/map_grow_lib.cpp) run
// the very same statements, so the device has the host's bits by construction.  Contraction off: an
// expression is the IEEE operations written here, in this order.
#ifndef CLC_MAP_MATH_H
#define CLC_MAP_MATH_H

#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MAP_HD __host__ __device__ __forceinline__
#else
#define MAP_HD static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace clc {

// P = K [R|t] (3 x 4 row-major) for K = { focal, 0, ppx; 0, focal, ppy; 0, 0, 1 } (Pinhole_Intrinsic::get_projective_equivalent,
// Reconstructor.hpp:241-245)
MAP_HD void projective_equivalent(const double focal, const double ppx, const double ppy, const double* Rt, double* P)
{
    for (int j = 0; j < 4; ++j) {
        P[j] = focal * Rt[j] + ppx * Rt[8 + j];
        P[4 + j] = focal * Rt[4 + j] + ppy * Rt[8 + j];
        P[8 + j] = Rt[8 + j];
    }
}

// The design matrix of TriangulateDLT(P1, x1.homogeneous(), P2, x2.homogeneous(), &X) (Reconstructor.hpp:223-225), 4 x 4 row-major:
// rows x[0] P.row(2) - x[2] P.row(0), x[1] P.row(2) - x[2] P.row(1) of either view with x[2] = 1 -- the matrix hipgeom::triangulate_dlt
// forms (host/HIPRobustMatcher.hpp:139-162) with projective matrices in place of [I|0] / [R|t].
MAP_HD void dlt_design(const double* P1, const double* x1, const double* P2, const double* x2, double* D)
{
    for (int j = 0; j < 4; ++j) {
        D[j] = x1[0] * P1[8 + j] - P1[j];
        D[4 + j] = x1[1] * P1[8 + j] - P1[4 + j];
        D[8 + j] = x2[0] * P2[8 + j] - P2[j];
        D[12 + j] = x2[1] * P2[8 + j] - P2[4 + j];
    }
}

// The right singular vector of D's smallest singular value by a one-sided (Hestenes) Jacobi on D itself: pairs of COLUMNS are rotated
// until they are orthogonal, the rotations accumulate in V, the singular values are the column norms.  Working on D -- not on D^T D --
// keeps the condition number unsquared: near-degenerate points (short baseline, far away) are where it matters.  At most 30 cyclic
// sweeps; a sweep that rotates nothing ends the iteration.  D is overwritten.
MAP_HD void null_vector4(double* D, double* v)
{
    double V[16];
    for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int k = 0; k < 4; ++k) {
                    alpha += D[4 * k + p] * D[4 * k + p];
                    beta += D[4 * k + q] * D[4 * k + q];
                    gamma += D[4 * k + p] * D[4 * k + q];
                }
                if (gamma == 0.0 || fabs(gamma) <= 1e-16 * sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < 4; ++k) {
                    const double dp = D[4 * k + p], dq = D[4 * k + q];
                    D[4 * k + p] = c * dp - s * dq;
                    D[4 * k + q] = s * dp + c * dq;
                    const double vp = V[4 * k + p], vq = V[4 * k + q];
                    V[4 * k + p] = c * vp - s * vq;
                    V[4 * k + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    int m = 0;
    double least = 0.0;
    for (int j = 0; j < 4; ++j) {
        double n2 = 0.0;
        for (int k = 0; k < 4; ++k) n2 += D[4 * k + j] * D[4 * k + j];
        if (j == 0 || n2 < least) { least = n2; m = j; }
    }
    for (int k = 0; k < 4; ++k) v[k] = V[4 * k + m];
}

// TriangulateDLT: X = hnormalized(null vector of the design matrix).  false: the point lies at infinity or is not finite (the reference
// divides all the same and keeps what comes out; a landmark without finite coordinates serves nobody, so it is dropped here).
MAP_HD bool triangulate_dlt(const double* P1, const double* x1, const double* P2, const double* x2, double* X)
{
    double D[16], v[4];
    dlt_design(P1, x1, P2, x2, D);
    null_vector4(D, v);
    if (!(fabs(v[3]) >= 1e-300)) return false;
    X[0] = v[0] / v[3]; X[1] = v[1] / v[3]; X[2] = v[2] / v[3];
    return isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
}

// Pose3::depth: (R X + t)[2]
MAP_HD double pose_depth(const double* Rt, const double* X) { return Rt[8] * X[0] + Rt[9] * X[1] + Rt[10] * X[2] + Rt[11]; }

// The reference's acceptance rule as written (Reconstructor.hpp:227-231): a point is dropped iff it lies behind BOTH cameras, or iff
// |X[2]| > 100.
MAP_HD bool seed_point_accepted(const double* Rt_i, const double* Rt_j, const double* X)
{
    if (pose_depth(Rt_i, X) < 0.0 && pose_depth(Rt_j, X) < 0.0) return false;
    if (fabs(X[2]) > 100.0) return false;
    return true;
}

// One seed landmark: undistorted pixels of the two seed cameras -> X.  false: dropped.
MAP_HD bool seed_point(const double* P_i, const double* P_j, const double* Rt_i, const double* Rt_j, const double* x_i, const double* x_j, double* X)
{
    return triangulate_dlt(P_i, x_i, P_j, x_j, X) && seed_point_accepted(Rt_i, Rt_j, X);
}

// ---- the grow step (Reconstructor::resectionCamera, Reconstructor.hpp:329-414; map_grow.hip) -----------------------------------------
// The bearing of an UNDISTORTED pixel under K = { focal, 0, ppx; 0, focal, ppy; 0, 0, 1 }.
MAP_HD void pixel_bearing(const double focal, const double ppx, const double ppy, const double* x_ud, double* b)
{
    b[0] = (x_ud[0] - ppx) / focal; b[1] = (x_ud[1] - ppy) / focal; b[2] = 1.0;
}

// R^T b of [R|t]: the bearing in world axes
MAP_HD void world_ray(const double* Rt, const double* b, double* r)
{
    for (int q = 0; q < 3; ++q) r[q] = Rt[q] * b[0] + Rt[4 + q] * b[1] + Rt[8 + q] * b[2];
}

// cos(2 degrees) to 17 digits
#define CLC_MAP_COS_2DEG 0.99939082701909573

// AngleBetweenRay(...) > 2 degrees (Reconstructor.hpp:383) without acos: dot < cos(2 deg) * sqrt(n_I * n_J), the plain sums below.
MAP_HD bool ray_angle_over_2deg(const double* r_i, const double* r_j)
{
    const double dot = r_i[0] * r_j[0] + r_i[1] * r_j[1] + r_i[2] * r_j[2];
    const double n_i = r_i[0] * r_i[0] + r_i[1] * r_i[1] + r_i[2] * r_i[2];
    const double n_j = r_j[0] * r_j[0] + r_j[1] * r_j[1] + r_j[2] * r_j[2];
    return dot < CLC_MAP_COS_2DEG * sqrt(n_i * n_j);
}

// A landmark is observed by a camera iff it lies in front of it and |X[2]| < 1000 (Reconstructor.hpp:402-411).
MAP_HD bool observation_ok(const double* Rt, const double* X) { return pose_depth(Rt, X) > 0.0 && fabs(X[2]) < 1000.0; }

// One new landmark from the resected camera I and a valid camera J: cam = { focal, ppx, ppy }, undistorted pixels -> X.  Accepted iff the
// ray angle is over 2 degrees, X is finite, both depths are positive and |X[2]| < 1000 (:383).  false: X is not to be used.
MAP_HD bool grow_point(const double* cam_i, const double* cam_j, const double* P_i, const double* P_j, const double* Rt_i, const double* Rt_j,
                       const double* x_i, const double* x_j, double* X)
{
    double b_i[3], b_j[3], r_i[3], r_j[3];
    pixel_bearing(cam_i[0], cam_i[1], cam_i[2], x_i, b_i);
    pixel_bearing(cam_j[0], cam_j[1], cam_j[2], x_j, b_j);
    world_ray(Rt_i, b_i, r_i);
    world_ray(Rt_j, b_j, r_j);
    if (!ray_angle_over_2deg(r_i, r_j)) return false;
    if (!triangulate_dlt(P_i, x_i, P_j, x_j, X)) return false;
    return pose_depth(Rt_i, X) > 0.0 && pose_depth(Rt_j, X) > 0.0 && fabs(X[2]) < 1000.0;
}

// Pose3::center of [R|t]: C = -R^T t
static inline void pose_center(const double* R9, const double* t, double* C)
{
    for (int q = 0; q < 3; ++q) C[q] = -(R9[q] * t[0] + R9[3 + q] * t[1] + R9[6 + q] * t[2]);
}

// rescaleMap on a pose (colocUtils.hpp:213-223 multiplies the CENTRE): C = pose_center(R, t), C' = C * s, t' = -R C'.  Rt: [R|t], 3 x 4
// row-major, t rewritten.  Host helper, as seed_poses below.
static inline void rescale_pose(double* Rt, const double s)
{
    const double R[9] = { Rt[0], Rt[1], Rt[2], Rt[4], Rt[5], Rt[6], Rt[8], Rt[9], Rt[10] }, t[3] = { Rt[3], Rt[7], Rt[11] };
    double C[3];
    pose_center(R, t, C);
    for (int q = 0; q < 3; ++q) C[q] = C[q] * s;
    for (int r = 0; r < 3; ++r) Rt[4 * r + 3] = -(R[3 * r] * C[0] + R[3 * r + 1] * C[1] + R[3 * r + 2] * C[2]);
}

// The two seed cameras' [R|t] (3 x 4 row-major each): camera I = the origin pose (R_o, centre C_o), camera J = relativePoseToAbsolute
// of the origin and Pose3(R_rel, scale * C_rel) (Reconstructor.hpp:215-221, 247-257) -- as odd as it is: R = R_rel R_o, C = C_o + scale
// C_rel, t = -R C.  Host helper: the device receives the two [R|t].
static inline void seed_poses(const double* Ro, const double* Co, const double* Rrel, const double* Crel, const double scale, double* Rt_i, double* Rt_j)
{
    double R[9], C[3];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) R[3 * r + q] = Rrel[3 * r] * Ro[q] + Rrel[3 * r + 1] * Ro[3 + q] + Rrel[3 * r + 2] * Ro[6 + q];
    for (int q = 0; q < 3; ++q) C[q] = Co[q] + scale * Crel[q];
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) { Rt_i[4 * r + q] = Ro[3 * r + q]; Rt_j[4 * r + q] = R[3 * r + q]; }
        Rt_i[4 * r + 3] = -(Ro[3 * r] * Co[0] + Ro[3 * r + 1] * Co[1] + Ro[3 * r + 2] * Co[2]);
        Rt_j[4 * r + 3] = -(R[3 * r] * C[0] + R[3 * r + 1] * C[1] + R[3 * r + 2] * C[2]);
    }
}

} // namespace clc

#endif

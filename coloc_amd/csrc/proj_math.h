// proj_math.h -- the two statements of the map match guided by a predicted pose (include/coloc_hip.h, clc_match_map_guided_dev), host +
// device inline and written ONCE, as guided_math.h is: the kernels of k2nn_guided.hip and the host build the tests hold them to
// (tests/host/proj_lib.cpp) run the very same lines.
//
//   proj_point      [R|t] (12 doubles, row-major 3 x 4, world to camera), the camera's focal and principal point, a landmark X -> the
//                   UNDISTORTED pixel of X, each coordinate rounded ONCE to float; or "none"
//   proj_in_radius  is train point (xt, yt) within sqrt(r2) pixels of query point (xq, yq)
//
// The fp64 part is + - x / in source order (every build that includes this has -ffp-contract=off); the fp32 part is a subtraction pair, ONE
// product and ONE explicit fused multiply-add, so it does not depend on that flag and is the same under g++ and on the device.  A landmark
// without a projection carries two quiet NaNs (guided_none()): the comparison of proj_in_radius is then false, and the sweep needs no flag
// beside the point.
#ifndef CLC_PROJ_MATH_H
#define CLC_PROJ_MATH_H

#include "guided_math.h"

namespace clc {

struct ProjCamera { double focal, ppx, ppy; };                    // what a projection reads of clc_camera_k3: no distortion is applied

// Xc = R X + t, each row ((R0 X0 + R1 X1) + R2 X2) + t; u = focal * (Xc0 / Xc2) + ppx, v = focal * (Xc1 / Xc2) + ppy, each rounded once
// to float.  false ("none": xy = two guided_none()) unless Xc2 > 0 and both floats are finite.
GUIDED_HD bool proj_point(const double* Rt, const ProjCamera& cam, const double* X, float* xy)
{
    const double xc = ((Rt[0] * X[0] + Rt[1] * X[1]) + Rt[2] * X[2]) + Rt[3];
    const double yc = ((Rt[4] * X[0] + Rt[5] * X[1]) + Rt[6] * X[2]) + Rt[7];
    const double zc = ((Rt[8] * X[0] + Rt[9] * X[1]) + Rt[10] * X[2]) + Rt[11];
    const float u = (float)(cam.focal * (xc / zc) + cam.ppx), v = (float)(cam.focal * (yc / zc) + cam.ppy);
    const bool ok = zc > 0.0 && __builtin_isfinite(u) && __builtin_isfinite(v);
    xy[0] = ok ? u : guided_none();
    xy[1] = ok ? v : guided_none();
    return ok;
}

// dx = xt - xq, dy = yt - yq, d2 = fma(dx, dx, dy * dy); candidate iff d2 <= r2 (r2 = radius * radius, formed once by the caller)
GUIDED_HD bool proj_in_radius(const float xq, const float yq, const float xt, const float yt, const float r2)
{
    const float dx = xt - xq, dy = yt - yq;
    const float d2 = __builtin_fmaf(dx, dx, dy * dy);
    return d2 <= r2;
}

} // namespace clc

#endif

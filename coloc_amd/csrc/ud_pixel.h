// ud_pixel.h -- Pinhole_Intrinsic_Radial_K3::get_ud_pixel (coloc_hip_geometry.hpp:97-135; OpenMVG's Pinhole_Intrinsic_Radial_K3) on the
// device, the ONE copy the track kernel and the pair kernel (gather.hip) share: + - x / sqrt only, in the host's order, and the
// library is built with -ffp-contract=off: the host's bits.
#pragma once

#include <hip/hip_runtime.h>

#include "clc_internal.h"

namespace clc {

__device__ __forceinline__ double ud_disto(const double r2, const double k1, const double k2, const double k3)
{
    const double t = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    return r2 * t * t;
}
__device__ inline double ud_radius_solve(const double r2, const double k1, const double k2, const double k3)
{
    double lowerbound = r2, upbound = r2;
    while (ud_disto(lowerbound, k1, k2, k3) > r2) lowerbound /= 1.05;
    while (ud_disto(upbound, k1, k2, k3) < r2) upbound *= 1.05;
    // (the step cap: a bracket whose width cannot fall below 1e-10 -- coefficients far outside any lens, a keypoint 10^5 focal lengths
    // out -- spins for ever on the host; a workgroup must not.  A bracket of finite doubles halves to below 1e-10 in < 1 100 steps.)
    for (int it = 0; it < 4096 && 1e-10 < upbound - lowerbound; ++it) {
        const double mid = .5 * (lowerbound + upbound);
        if (ud_disto(mid, k1, k2, k3) > r2) upbound = mid;
        else lowerbound = mid;
    }
    return .5 * (lowerbound + upbound);
}
// the feature position of row q: the detector's level-local keypoint, scale * (float)x in float with the host's table of
// (float) pow((double) 1.2f, level) (clc_keypoints_to_features), or a block of float positions already scaled
__device__ __forceinline__ void feature_position(const clc_keypoint* kps, const float* feat, const int feat_stride, const uint32_t q,
                                                 const float* scale, float* fx, float* fy)
{
    if (kps) {
        const clc_keypoint kp = kps[q];
        const float s = scale[kp.scale < CLC_MAX_LEVELS ? kp.scale : CLC_MAX_LEVELS - 1];
        *fx = s * (float)kp.x;
        *fy = s * (float)kp.y;
    } else {
        const float* f = feat + (size_t)q * (size_t)feat_stride;
        *fx = f[0];
        *fy = f[1];
    }
}
// get_ud_pixel of the float feature position (fx, fy), widened to double: ima2cam, radius by bisection, cam2ima
__device__ inline void ud_pixel(const float fx, const float fy, const UdCamera& c, double* out)
{
    const double c0 = ((double)fx - c.ppx) / c.focal, c1 = ((double)fy - c.ppy) / c.focal;
    const double r2 = c0 * c0 + c1 * c1;
    const double radius = (r2 == 0.0) ? 1.0 : sqrt(ud_radius_solve(r2, c.k1, c.k2, c.k3) / r2);
    out[0] = c.focal * (radius * c0) + c.ppx;
    out[1] = c.focal * (radius * c1) + c.ppy;
}

} // namespace clc

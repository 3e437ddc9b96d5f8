// guided_math.h -- the two statements of the guided match (include/coloc_hip.h, clc_match_guided_dev), host + device inline and written
// ONCE, as k2nn_top2.h and map_math.h are: the kernels of k2nn_guided.hip and the host build the tests hold them to
// (tests/host/guided_lib.cpp) run the very same lines.
//
//   guided_line     F (9 doubles, row-major, x_b^T F x_a = 0) and the undistorted pixel (u, v) of a query row -> the epipolar line of the
//                   query in image B, normalised so that |L . (x, y, 1)| is the distance of (x, y) from it in pixels, rounded ONCE to
//                   float; or "none"
//   guided_in_band  is train point (x, y) within `band` pixels of that line
//
// The fp64 part is + - x / sqrt in source order (every build that includes this has -ffp-contract=off); the fp32 part is two EXPLICIT fused
// multiply-adds, so it does not depend on that flag and is the same under g++ and on the device.  A query without a line carries three
// quiet NaNs: every comparison of guided_in_band is then false, and the sweep needs no flag beside the line.
#ifndef CLC_GUIDED_MATH_H
#define CLC_GUIDED_MATH_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define GUIDED_HD __host__ __device__ __forceinline__
#else
#define GUIDED_HD static inline
#endif

namespace clc {

static constexpr uint32_t kGuidedNoneBits = 0x7FC00000u;          // the component of a "none" line, and of a row past a device-side count

GUIDED_HD float guided_none()
{
    const uint32_t b = kGuidedNoneBits;
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

// l = F (u, v, 1), n = sqrt(l0^2 + l1^2), L = l / n.  false ("none": L = three guided_none()) when n is zero or not finite or a
// component of L is not finite.
GUIDED_HD bool guided_line(const double* F, const double u, const double v, float* L)
{
    const double l0 = F[0] * u + F[1] * v + F[2];
    const double l1 = F[3] * u + F[4] * v + F[5];
    const double l2 = F[6] * u + F[7] * v + F[8];
    const double n = __builtin_sqrt(l0 * l0 + l1 * l1);
    const float a = (float)(l0 / n), b = (float)(l1 / n), c = (float)(l2 / n);
    const bool ok = n > 0.0 && __builtin_isfinite(n) && __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(c);
    L[0] = ok ? a : guided_none();
    L[1] = ok ? b : guided_none();
    L[2] = ok ? c : guided_none();
    return ok;
}

// e = fma(L0, x, fma(L1, y, L2)); candidate iff |e| <= band
GUIDED_HD bool guided_in_band(const float L0, const float L1, const float L2, const float x, const float y, const float band)
{
    const float e = __builtin_fmaf(L0, x, __builtin_fmaf(L1, y, L2));
    return __builtin_fabsf(e) <= band;
}

} // namespace clc

#endif

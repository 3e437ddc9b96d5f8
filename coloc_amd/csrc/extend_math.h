// extend_math.h -- the statements of the map extension (include/coloc_hip.h, clc_map_extend_dev) that no other header holds, host + device
// inline and written ONCE, as map_math.h and unique_math.h are: the entry and the kernels of map_extend.hip and the host build the tests
// hold them to (tests/host/map_extend_lib.cpp) run the very same lines.  The step's other rules are used as they stand: the guided match
// (guided_math.h), the one-to-one filter (unique_math.h), get_ud_pixel (ud_pixel.h) and grow_point (map_math.h).
//
//   fundamental_from_poses   F of two posed views, x_b^T F x_a = 0 in undistorted pixels: clc_guided_job.F's orientation and units
//   extend_keeps             the mask behind the guided sweep: may entry q -> t become a new landmark at all
//
// fp64, + - x / in source order, no contraction (map_math.h switches it off for every build that includes this).
#ifndef CLC_EXTEND_MATH_H
#define CLC_EXTEND_MATH_H

#include "guided_math.h"
#include "map_math.h"
#include "unique_math.h"

namespace clc {

static constexpr int32_t kExtendMaxDistance = (int32_t)kUniqueMaxDist;      // max_distance lies in [0, 512]

// cam = { focal, ppx, ppy }, Rt = [R|t] 3 x 4 row-major, world to camera.  In this order:
//   R = R_b R_a^T            every entry (r0 c0 + r1 c1) + r2 c2
//   t = t_b - R t_a          the product summed the same way, then ONE subtraction
//   E = [t]x R               every entry one difference of two products
//   G = E K_a^-1             columns 0, 1 divided by focal_a; column 2: E2 - (E0 ppx_a + E1 ppy_a) / focal_a
//   F = K_b^-T G             rows 0, 1 divided by focal_b;    row 2:    G2 - (G0 ppx_b + G1 ppy_b) / focal_b
// Two views with one centre have t = 0 and F = 0: no query has a line (guided_line), so nothing is matched.
MAP_HD void fundamental_from_poses(const double* cam_a, const double* Rt_a, const double* cam_b, const double* Rt_b, double* F)
{
    double R[9], t[3], E[9], G[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (Rt_b[4 * r] * Rt_a[4 * c] + Rt_b[4 * r + 1] * Rt_a[4 * c + 1]) + Rt_b[4 * r + 2] * Rt_a[4 * c + 2];
    for (int r = 0; r < 3; ++r) t[r] = Rt_b[4 * r + 3] - ((R[3 * r] * Rt_a[3] + R[3 * r + 1] * Rt_a[7]) + R[3 * r + 2] * Rt_a[11]);
    for (int c = 0; c < 3; ++c) {
        E[c] = t[1] * R[6 + c] - t[2] * R[3 + c];
        E[3 + c] = t[2] * R[c] - t[0] * R[6 + c];
        E[6 + c] = t[0] * R[3 + c] - t[1] * R[c];
    }
    for (int r = 0; r < 3; ++r) {
        G[3 * r] = E[3 * r] / cam_a[0];
        G[3 * r + 1] = E[3 * r + 1] / cam_a[0];
        G[3 * r + 2] = E[3 * r + 2] - (E[3 * r] * cam_a[1] + E[3 * r + 1] * cam_a[2]) / cam_a[0];
    }
    for (int c = 0; c < 3; ++c) {
        F[c] = G[c] / cam_b[0];
        F[3 + c] = G[3 + c] / cam_b[0];
        F[6 + c] = G[6 + c] - (G[c] * cam_b[1] + G[3 + c] * cam_b[2]) / cam_b[0];
    }
}

// Entry q of the guided list names train row t, 0 <= t < nt, at distance `best`.  track_a = A's map match of q, track_b = B's of t (-1
// where the view has no list).  It stays iff neither keypoint is a landmark already and the distance is within the cap: the guided rule
// accepts a lone candidate at ANY distance.  The caller reads track_b only for a row inside the train set.
GUIDED_HD bool extend_keeps(const int32_t track_a, const int32_t track_b, const uint32_t best, const int32_t max_distance)
{
    return track_a < 0 && track_b < 0 && best <= (uint32_t)max_distance;
}

} // namespace clc

#endif

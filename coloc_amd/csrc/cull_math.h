// cull_math.h -- the statements of the map's observation statistics and of the cull (include/coloc_hip.h, clc_map_observe_dev and
// clc_map_cull_dev) that no other header holds, host + device inline and written ONCE, as extend_math.h and unique_math.h are: the
// kernels of map_cull.hip and the host build the tests hold them to (tests/host/map_cull_lib.cpp) run the very same lines.  The projection
// of a landmark and the gate of a hit are used as they stand (proj_point, proj_in_radius: proj_math.h), a keypoint's undistorted pixel too
// (ud_pixel.h, on the device).
//
//   cull_in_view       is the float pixel (u, v) inside the rectangle [lo, hi_x] x [lo, hi_y]; NaN is outside
//   cull_bounds        lo, hi_x, hi_y of an image and a margin, formed once by the host
//   cull_clause        which clause of the rule drops a row: 0 none (the row stays), 1 flagged, 2 the found / visible ratio, 3 idle --
//                      the FIRST that fires in this order
//   cull_drops         cull_clause != 0
//   cull_remap_entry   a track-list entry under a remap
//   cull_remap         the remap of a drop list on the host: kept rows in ascending old order (the device: wg_compact.h)
//
// The rectangle test is three float comparisons a side, everything else integers: nothing here depends on a floating-point flag.
#ifndef CLC_CULL_MATH_H
#define CLC_CULL_MATH_H

#include "proj_math.h"

namespace clc {

enum { kCullKept = 0, kCullFlagged = 1, kCullRatio = 2, kCullIdle = 3 };

// the customary rule -- a row seen in at least 8 frames and found in fewer than a quarter of them goes, idleness is not judged --: UNTUNED
static constexpr int32_t kCullMinVisible = 8, kCullNum = 1, kCullDen = 4;
static constexpr uint32_t kCullMaxIdle = 0u;

// true iff u >= lo && u <= hi_x && v >= lo && v <= hi_y: a landmark without a projection (two guided_none()) is never in view
GUIDED_HD bool cull_in_view(const float u, const float v, const float lo, const float hi_x, const float hi_y)
{
    return u >= lo && u <= hi_x && v >= lo && v <= hi_y;
}

// lo = margin, hi_x = (float)(width - 1) - margin, hi_y = (float)(height - 1) - margin, in UNDISTORTED pixels (the projection gate's deviation)
GUIDED_HD void cull_bounds(const int width, const int height, const float margin, float* lo, float* hi_x, float* hi_y)
{
    *lo = margin;
    *hi_x = (float)(width - 1) - margin;
    *hi_y = (float)(height - 1) - margin;
}

// A row with visible < min_visible is too young for the ratio test; the products are 64-bit (the counters run to 2^32 - 1); the idle
// time is the difference of two 32-bit epochs modulo 2^32, and max_idle == 0 switches the test off.
GUIDED_HD int cull_clause(const uint32_t visible, const uint32_t found, const uint32_t last_view, const uint32_t epoch, const bool flagged,
                          const uint32_t min_visible, const uint32_t num, const uint32_t den, const uint32_t max_idle)
{
    if (flagged) return kCullFlagged;
    if (visible >= min_visible && (uint64_t)found * den < (uint64_t)num * visible) return kCullRatio;
    if (max_idle > 0 && (uint32_t)(epoch - last_view) > max_idle) return kCullIdle;
    return kCullKept;
}

GUIDED_HD bool cull_drops(const uint32_t visible, const uint32_t found, const uint32_t last_view, const uint32_t epoch, const bool flagged,
                          const uint32_t min_visible, const uint32_t num, const uint32_t den, const uint32_t max_idle)
{
    return cull_clause(visible, found, last_view, epoch, flagged, min_visible, num, den, max_idle) != kCullKept;
}

// entry e of a list that names map rows, after a cull of a map of n_before rows: the row's new index, or -1 for a dropped row and for
// whatever named no row before
GUIDED_HD int32_t cull_remap_entry(const int32_t e, const int32_t n_before, const int32_t* remap)
{
    return e >= 0 && e < n_before ? remap[e] : -1;
}

// remap[r] = the number of kept rows below r where row r is kept, -1 otherwise; returns the number of kept rows
static inline int32_t cull_remap(const uint8_t* drops, const int32_t n, int32_t* remap)
{
    int32_t kept = 0;
    for (int32_t r = 0; r < n; ++r) remap[r] = drops[r] ? -1 : kept++;
    return kept;
}

// true iff a host remap of n entries is one a cull can have produced: every entry -1 or the count of kept entries below it
static inline bool cull_remap_valid(const int32_t* remap, const int32_t n, int32_t* kept_out)
{
    int32_t kept = 0;
    for (int32_t r = 0; r < n; ++r) {
        if (remap[r] == -1) continue;
        if (remap[r] != kept) return false;
        ++kept;
    }
    *kept_out = kept;
    return true;
}

} // namespace clc

#endif

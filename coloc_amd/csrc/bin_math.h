// bin_math.h -- the cell rule of the map match by projection through a cell grid (include/coloc_hip.h, clc_match_map_binned_dev), host +
// device inline and written ONCE, as proj_math.h is: the kernels of k2nn_binned.hip, the host plan of the entry and the host build the
// tests hold them to (tests/host/bin_lib.cpp) run the very same lines.
//
//   rw    = (double)radius * (1.0 + 0x1p-10)             the window's half-width
//   W     = 2.0 * max(ppx, ppy)                          the grid's extent on both axes, origin (0, 0)
//   c     = max(rw, W / 64.0)                            the cell's side: never below rw
//   k(v)  = (int)min(max(floor(v / c), -1.0), 64.0) + 1  1 .. 64 inside, 0 and 65 the ring; clamped BEFORE the conversion
//   cell(x, y) = k(y) * 66 + k(x)                        66 * 66 = 4356 cells, row-major
//
// Everything is fp64 + - x / and floor in source order (every build that includes this has -ffp-contract=off); max and min are the two
// comparisons written below, so a NaN falls to the lower clamp (k(NaN) = 0) under every compiler.  Why the window of a query --
// k(q - rw) .. k(q + rw) on either axis -- holds every row that passes proj_in_radius: DESIGN.md 4.1.
#ifndef CLC_BIN_MATH_H
#define CLC_BIN_MATH_H

#include "guided_math.h"

namespace clc {

static constexpr int kBinAxis = 66;                               // cells per axis: 64 inside and the ring on either side
static constexpr int kBinCells = kBinAxis * kBinAxis;             // 4356
static constexpr int kBinMaxRows = 65536;                         // map rows a BINNED plan takes
enum { BIN_PLAN_SWEEP = 0, BIN_PLAN_BINNED = 1 };

GUIDED_HD double bin_max(const double a, const double b) { return a > b ? a : b; }      // (a NaN in `a` gives b)
GUIDED_HD double bin_min(const double a, const double b) { return a < b ? a : b; }

GUIDED_HD double bin_half_width(const float radius) { return (double)radius * (1.0 + 0x1p-10); }
GUIDED_HD double bin_extent(const double ppx, const double ppy) { return 2.0 * bin_max(ppx, ppy); }
GUIDED_HD double bin_cell_side(const double rw, const double W) { return bin_max(rw, W / 64.0); }

GUIDED_HD int bin_k(const double v, const double c)
{
    return (int)bin_min(bin_max(__builtin_floor(v / c), -1.0), 64.0) + 1;
}
GUIDED_HD int bin_cell(const double x, const double y, const double c) { return bin_k(y, c) * kBinAxis + bin_k(x, c); }

// the window of a query coordinate: cells lo .. hi, at most three of them because c >= rw
GUIDED_HD void bin_window(const double q, const double rw, const double c, int* lo, int* hi)
{
    *lo = bin_k(q - rw, c);
    *hi = bin_k(q + rw, c);
}

// THE plan: BINNED iff radius >= 2^-10, 8 rw <= W, 0 < map_n <= 65 536 and ppx, ppy finite and positive; SWEEP otherwise
GUIDED_HD int bin_plan(const double ppx, const double ppy, const float radius, const long long map_n)
{
    const bool cam_ok = __builtin_isfinite(ppx) && __builtin_isfinite(ppy) && ppx > 0.0 && ppy > 0.0;
    if (!cam_ok || !(radius >= 0x1p-10f)) return BIN_PLAN_SWEEP;
    if (!(8.0 * bin_half_width(radius) <= bin_extent(ppx, ppy))) return BIN_PLAN_SWEEP;
    return map_n > 0 && map_n <= (long long)kBinMaxRows ? BIN_PLAN_BINNED : BIN_PLAN_SWEEP;
}

} // namespace clc

#endif

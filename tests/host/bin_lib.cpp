// Host build of the cell rule of the map match through a cell grid (coloc_amd/csrc/bin_math.h) as a tiny shared library for the tests
// (tests/bin_host.py): the grid of a job, k, the cell of a projection, the window of a query and the plan, compiled by g++ without
// contraction -- the lines the kernels of coloc_amd/csrc/k2nn_binned.hip and the entry's host plan run.  Test infrastructure only.
#include <cstdint>
#include "../../coloc_amd/csrc/bin_math.h"

using namespace clc;

extern "C" {

// out = { rw, W, c }
void bin_host_grid(double ppx, double ppy, float radius, double* out)
{
    out[0] = bin_half_width(radius);
    out[1] = bin_extent(ppx, ppy);
    out[2] = bin_cell_side(out[0], out[1]);
}

void bin_host_k(const double* v, int n, double c, int32_t* out)
{
    for (int i = 0; i < n; ++i) out[i] = bin_k(v[i], c);
}

// xy: n x 2 floats -> the cell of each point, or -1 for a row without a projection (a NaN coordinate)
void bin_host_cells(const float* xy, int n, double c, int32_t* out)
{
    for (int i = 0; i < n; ++i) {
        const float x = xy[2 * i], y = xy[2 * i + 1];
        out[i] = (x == x && y == y) ? bin_cell((double)x, (double)y, c) : -1;
    }
}

// q: n x 2 floats -> out: n x 4 = { kx0, kx1, ky0, ky1 }; a query whose point is NaN has no window: { 1, 0, 1, 0 }
void bin_host_windows(const float* q, int n, double rw, double c, int32_t* out)
{
    for (int i = 0; i < n; ++i) {
        const float x = q[2 * i], y = q[2 * i + 1];
        int32_t* o = out + 4 * i;
        if (x == x && y == y) {
            int lo, hi;
            bin_window((double)x, rw, c, &lo, &hi); o[0] = lo; o[1] = hi;
            bin_window((double)y, rw, c, &lo, &hi); o[2] = lo; o[3] = hi;
        } else {
            o[0] = 1; o[1] = 0; o[2] = 1; o[3] = 0;
        }
    }
}

int bin_host_plan(double ppx, double ppy, float radius, long long map_n) { return bin_plan(ppx, ppy, radius, map_n); }

int bin_host_cells_per_axis() { return kBinAxis; }
int bin_host_max_rows() { return kBinMaxRows; }

} // extern "C"

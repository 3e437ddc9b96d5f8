// Host build of the arithmetic behind coloc_amd/csrc/map_update.hip as a tiny shared library for the tests (tests/map_update_host.py,
// tests/test_map_update_host.py, tests/test_gpu_map_update.py): the statements of inter_math.h / map_math.h that map_align_kernel and
// clc_map_update_batch_dev run, compiled by g++ without contraction, in the order the kernel keeps -- the terms of consecutive common
// features summed sequentially in list order.  No GPU, no HIP headers.  Test infrastructure only.
#include <stdint.h>

#include "../../coloc_amd/csrc/inter_math.h"
#include "../../coloc_amd/csrc/map_math.h"

extern "C" {

// The scale of a common list: cq / ct = old / new row of the n_common common features, in list order; old_X / new_X the two maps' points.
// *scale = the mean of the kept terms, or 1.0 where there is none to be had; *n_terms = the kept terms; returns the status
// (0: CLC_MAP_ALIGN_OK, 1: CLC_MAP_ALIGN_NO_SCALE).
int map_update_host_scale(const double* old_X, const double* new_X, const int32_t* cq, const int32_t* ct, int n_common, double* scale, int* n_terms)
{
    double sum = 0.0;
    unsigned good = 0;
    for (int k = 0; k + 1 < n_common; ++k) {
        const double v = clc::scale_term(old_X + 3 * (size_t)cq[k], old_X + 3 * (size_t)cq[k + 1], new_X + 3 * (size_t)ct[k], new_X + 3 * (size_t)ct[k + 1]);
        if (!(v < 0.0)) { sum += v; ++good; }
    }
    *n_terms = (int)good;
    if (clc::scale_from_sum(sum, good, scale) != CLC_INTER_OK) { *scale = 1.0; return CLC_MAP_ALIGN_NO_SCALE; }
    return CLC_MAP_ALIGN_OK;
}

// rescaleMap on the points: every component one multiply
void map_update_host_rescale_points(const double* X, int n, double scale, double* out)
{
    for (int i = 0; i < 3 * n; ++i) out[i] = X[i] * scale;
}

// rescaleMap on a pose [R|t] (12 doubles, rewritten): the centre multiplied
void map_update_host_rescale_pose(double* Rt, double scale) { clc::rescale_pose(Rt, scale); }

}

// Host build of the two statements of the map match guided by a predicted pose (coloc_amd/csrc/proj_math.h) as a tiny shared library for
// the tests (tests/proj_host.py): the projection of a landmark and the radius gate, compiled by g++ without contraction -- the lines the
// kernels of coloc_amd/csrc/k2nn_guided.hip run, so results are compared bit for bit.  Test infrastructure only.
#include <cstdint>
#include "../../coloc_amd/csrc/proj_math.h"

using namespace clc;

extern "C" {

// Rt: 12 doubles; cam: focal, ppx, ppy; X: n x 3 landmarks -> xy: n x 2 floats, ok: n bytes (0: "none", xy = two quiet NaNs)
void proj_host_points(const double* Rt, const double* cam, const double* X, int n, float* xy, uint8_t* ok)
{
    const ProjCamera c{ cam[0], cam[1], cam[2] };
    for (int i = 0; i < n; ++i) ok[i] = proj_point(Rt, c, X + 3 * i, xy + 2 * i) ? 1 : 0;
}

// one query point against n train points (floats): in[i] = candidate or not
void proj_host_gate(const float* q, const float* xy, int n, float r2, uint8_t* in)
{
    for (int i = 0; i < n; ++i) in[i] = proj_in_radius(q[0], q[1], xy[2 * i], xy[2 * i + 1], r2) ? 1 : 0;
}

uint32_t proj_host_none_bits() { return kGuidedNoneBits; }

} // extern "C"

// Host build of the guided match's two statements (coloc_amd/csrc/guided_math.h) as a tiny shared library for the tests
// (tests/guided_host.py): the line of a query and the band gate, compiled by g++ without contraction -- the lines the kernels of
// coloc_amd/csrc/k2nn_guided.hip run, so results are compared bit for bit.  Test infrastructure only.
#include <cstdint>
#include "../../coloc_amd/csrc/guided_math.h"

using namespace clc;

extern "C" {

// uv: n x 2 undistorted pixels (fp64) -> L: n x 3 floats, ok: n bytes (0: "none", L = three quiet NaNs)
void guided_host_lines(const double* F, const double* uv, int n, float* L, uint8_t* ok)
{
    for (int i = 0; i < n; ++i) ok[i] = guided_line(F, uv[2 * i], uv[2 * i + 1], L + 3 * i) ? 1 : 0;
}

// one line against n train points (x, y as floats): in[i] = candidate or not
void guided_host_gate(const float* L, const float* xy, int n, float band, uint8_t* in)
{
    for (int i = 0; i < n; ++i) in[i] = guided_in_band(L[0], L[1], L[2], xy[2 * i], xy[2 * i + 1], band) ? 1 : 0;
}

uint32_t guided_host_none_bits() { return kGuidedNoneBits; }

} // extern "C"

// Host build of coloc_amd/csrc/cull_math.h as a tiny shared library for the tests (tests/map_cull_host.py, tests/test_map_cull_host.py,
// tests/test_gpu_map_cull.py): what the entries and the kernels of map_cull.hip run, compiled by g++.  No GPU, no HIP headers.  Test
// infrastructure only.
#include <stdint.h>

#include "../../coloc_amd/csrc/cull_math.h"

extern "C" {

// out = { lo, hi_x, hi_y }
void map_cull_host_bounds(int width, int height, float margin, float* out) { clc::cull_bounds(width, height, margin, out, out + 1, out + 2); }

// n float pixels (n x 2) against the rectangle: in[n]
void map_cull_host_in_view(const float* uv, int n, float lo, float hi_x, float hi_y, uint8_t* in)
{
    for (int i = 0; i < n; ++i) in[i] = clc::cull_in_view(uv[2 * i], uv[2 * i + 1], lo, hi_x, hi_y) ? 1 : 0;
}

// the rule on n rows (flagged nullable): clause[n] (0 kept, 1 flagged, 2 ratio, 3 idle) and drops[n]
void map_cull_host_rule(const uint32_t* visible, const uint32_t* found, const uint32_t* last_view, int n, uint32_t epoch, const uint8_t* flagged,
                        uint32_t min_visible, uint32_t num, uint32_t den, uint32_t max_idle, uint8_t* clause, uint8_t* drops)
{
    for (int i = 0; i < n; ++i) {
        const bool f = flagged && flagged[i] != 0;
        clause[i] = (uint8_t)clc::cull_clause(visible[i], found[i], last_view[i], epoch, f, min_visible, num, den, max_idle);
        drops[i] = clc::cull_drops(visible[i], found[i], last_view[i], epoch, f, min_visible, num, den, max_idle) ? 1 : 0;
    }
}

int32_t map_cull_host_remap(const uint8_t* drops, int32_t n, int32_t* remap) { return clc::cull_remap(drops, n, remap); }

// a list of m entries through the remap of a map of n_before rows, in place
void map_cull_host_remap_list(int32_t* list, int m, int32_t n_before, const int32_t* remap)
{
    for (int i = 0; i < m; ++i) list[i] = clc::cull_remap_entry(list[i], n_before, remap);
}

// -1: not a remap a cull can have produced; else the kept count
int32_t map_cull_host_remap_valid(const int32_t* remap, int32_t n)
{
    int32_t kept = 0;
    return clc::cull_remap_valid(remap, n, &kept) ? kept : -1;
}

// { min_visible, num, den, max_idle } of the customary rule
void map_cull_host_default_rule(int32_t* out)
{
    out[0] = clc::kCullMinVisible; out[1] = clc::kCullNum; out[2] = clc::kCullDen; out[3] = (int32_t)clc::kCullMaxIdle;
}

}

// Host build of coloc_amd/csrc/extend_math.h and of grow_point (map_math.h) as a tiny shared library for the tests
// (tests/map_extend_host.py, tests/test_map_extend_host.py, tests/test_map_extend_abi.py, tests/test_gpu_map_extend.py): what the entry
// and the kernels of map_extend.hip run, compiled by g++ without contraction.  No GPU, no HIP headers.  Test infrastructure only.
#include <stdint.h>

#include "../../coloc_amd/csrc/extend_math.h"

extern "C" {

// F of two posed views: cam = { focal, ppx, ppy }, Rt 12 doubles -> F 9
void map_extend_host_fundamental(const double* cam_a, const double* Rt_a, const double* cam_b, const double* Rt_b, double* F)
{
    clc::fundamental_from_poses(cam_a, Rt_a, cam_b, Rt_b, F);
}

// the mask on n entries: keeps[n]
void map_extend_host_keeps(const int32_t* track_a, const int32_t* track_b, const uint32_t* best, int n, int max_distance, uint8_t* keeps)
{
    for (int i = 0; i < n; ++i) keeps[i] = clc::extend_keeps(track_a[i], track_b[i], best[i], max_distance);
}

// grow_point of n pairs of undistorted pixels (n x 2 each) with camera A in the place of the resected camera: ok[n], X n x 3
void map_extend_host_points(const double* cam_a, const double* cam_b, const double* Rt_a, const double* Rt_b, const double* x_a, const double* x_b,
                            int n, uint8_t* ok, double* X)
{
    double P_a[12], P_b[12];
    clc::projective_equivalent(cam_a[0], cam_a[1], cam_a[2], Rt_a, P_a);
    clc::projective_equivalent(cam_b[0], cam_b[1], cam_b[2], Rt_b, P_b);
    for (int i = 0; i < n; ++i) {
        double Xi[3] = { 0.0, 0.0, 0.0 };
        ok[i] = clc::grow_point(cam_a, cam_b, P_a, P_b, Rt_a, Rt_b, x_a + 2 * i, x_b + 2 * i, Xi);
        X[3 * i] = Xi[0]; X[3 * i + 1] = Xi[1]; X[3 * i + 2] = Xi[2];
    }
}

int map_extend_host_max_distance(void) { return clc::kExtendMaxDistance; }

}

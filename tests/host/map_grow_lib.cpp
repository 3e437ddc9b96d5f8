// Host build of the grow statements of coloc_amd/csrc/map_math.h as a tiny shared library for the tests (tests/map_grow_host.py,
// tests/test_map_grow_host.py, tests/test_gpu_map_grow.py): what grow_kernel runs on the device, compiled by g++ without contraction.
// No GPU, no HIP headers.  Test infrastructure only.
#include <stdint.h>

#include "../../coloc_amd/csrc/map_math.h"

extern "C" {

// the world ray of an undistorted pixel: cam = { focal, ppx, ppy }, Rt 12 doubles -> r 3
void map_grow_host_ray(const double* cam, const double* Rt, const double* x_ud, double* r)
{
    double b[3];
    clc::pixel_bearing(cam[0], cam[1], cam[2], x_ud, b);
    clc::world_ray(Rt, b, r);
}

// the angle decision on n pairs of rays (n x 3 each): over[n]
void map_grow_host_angle(const double* r_i, const double* r_j, int n, uint8_t* over)
{
    for (int i = 0; i < n; ++i) over[i] = clc::ray_angle_over_2deg(r_i + 3 * i, r_j + 3 * i);
}

// grow_point of one track: -> accepted, X 3
int map_grow_host_point(const double* cam_i, const double* cam_j, const double* Rt_i, const double* Rt_j, const double* x_i, const double* x_j, double* X)
{
    double P_i[12], P_j[12];
    clc::projective_equivalent(cam_i[0], cam_i[1], cam_i[2], Rt_i, P_i);
    clc::projective_equivalent(cam_j[0], cam_j[1], cam_j[2], Rt_j, P_j);
    return clc::grow_point(cam_i, cam_j, P_i, P_j, Rt_i, Rt_j, x_i, x_j, X);
}

int map_grow_host_observation_ok(const double* Rt, const double* X) { return clc::observation_ok(Rt, X); }

double map_grow_host_cos_2deg(void) { return CLC_MAP_COS_2DEG; }

}

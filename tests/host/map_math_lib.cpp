// Host build of coloc_amd/csrc/map_math.h as a tiny shared library for the tests (tests/map_host.py, tests/test_map_host.py,
// tests/test_gpu_map_build.py): the statements seed_triangulate_kernel runs on the device, compiled by g++ without contraction.  No
// GPU, no HIP headers.  Test infrastructure only.
#include <stdint.h>

#include "../../coloc_amd/csrc/map_math.h"

extern "C" {

// the design matrix of one correspondence under P1 / P2 (3 x 4 each): D 16 doubles
void map_math_host_design(const double* P1, const double* x1, const double* P2, const double* x2, double* D) { clc::dlt_design(P1, x1, P2, x2, D); }

// TriangulateDLT of n correspondences (x1 / x2: n x 2 undistorted pixels) under P1 / P2: X n x 3, ok[n]
void map_math_host_triangulate(const double* P1, const double* P2, const double* x1, const double* x2, int n, double* X, uint8_t* ok)
{
    for (int i = 0; i < n; ++i) ok[i] = clc::triangulate_dlt(P1, x1 + 2 * i, P2, x2 + 2 * i, X + 3 * i);
}

// the seed kernel's statement: cam = { focal, ppx, ppy }, Rt 12 doubles each -> X n x 3, accepted[n]
void map_math_host_seed_points(const double* cam_i, const double* cam_j, const double* Rt_i, const double* Rt_j, const double* x_i, const double* x_j,
                               int n, double* X, uint8_t* accepted)
{
    double P_i[12], P_j[12];
    clc::projective_equivalent(cam_i[0], cam_i[1], cam_i[2], Rt_i, P_i);
    clc::projective_equivalent(cam_j[0], cam_j[1], cam_j[2], Rt_j, P_j);
    for (int i = 0; i < n; ++i) accepted[i] = clc::seed_point(P_i, P_j, Rt_i, Rt_j, x_i + 2 * i, x_j + 2 * i, X + 3 * i);
}

int map_math_host_accepted(const double* Rt_i, const double* Rt_j, const double* X) { return clc::seed_point_accepted(Rt_i, Rt_j, X); }

void map_math_host_pose_center(const double* R, const double* t, double* C) { clc::pose_center(R, t, C); }

void map_math_host_seed_poses(const double* Ro, const double* Co, const double* Rrel, const double* Crel, double scale, double* Rt_i, double* Rt_j)
{
    clc::seed_poses(Ro, Co, Rrel, Crel, scale, Rt_i, Rt_j);
}

}

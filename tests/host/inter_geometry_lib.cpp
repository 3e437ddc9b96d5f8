// Host build of the inter-camera geometry (coloc_amd/csrc/inter_geometry.cpp over inter_math.h: inter_relative, inter_scale_pose) as a
// tiny shared library for the tests (tests/inter_geometry_host.py, tests/test_inter_geometry_host.py): the statements clc_inter_pose_batch
// runs on the host and inter_front_kernel / inter_scale_kernel run on the device, compiled by g++ without contraction.  Built together
// with inter_geometry.cpp; no GPU, no HIP headers.  Test infrastructure only.
#include <algorithm>
#include <cstring>

#include "../../coloc_amd/csrc/inter_geometry.h"

extern "C" {

// inter_relative on n correspondences with E and the inlier list given.  Xt / x2f / corr: room for n_inliers points; R (9), t (3).
// Returns the stage; *n_front = points written.
int inter_geometry_host_relative(const double* x1, const double* x2, int n, const double* K1, const double* K2, const double* E,
                                 const int32_t* inliers, int n_inliers, double* Xt, double* x2f, int32_t* corr, double* R, double* t, int* n_front)
{
    clc_inter_pose_job jb{};
    double e[9];
    memcpy(e, E, sizeof e);
    jb.tv.x1 = x1; jb.tv.x2 = x2; jb.tv.n = n; jb.tv.K1 = K1; jb.tv.K2 = K2; jb.tv.E = e;
    jb.tv.inliers = const_cast<int32_t*>(inliers); jb.tv.n_inliers = n_inliers;
    clc::InterFront fr{};
    const int stage = clc::inter_relative(jb, fr);
    *n_front = jb.n_front;
    if (stage != CLC_INTER_OK) return stage;
    std::copy(fr.Xt.begin(), fr.Xt.end(), Xt); std::copy(fr.x2f.begin(), fr.x2f.end(), x2f); std::copy(fr.corr.begin(), fr.corr.end(), corr);
    memcpy(R, fr.R, sizeof fr.R); memcpy(t, fr.t, sizeof fr.t);
    return stage;
}

// inter_scale_pose on a temporary map of nf points (Xt, R, t as inter_relative left them) and n_common pairs (global map point,
// temporary map point) in the order the rule walks them.  Rt (12), Xw (3 nf).  Returns the stage.
int inter_geometry_host_scale_pose(const double* Xt, int nf, const double* R, const double* t, const int32_t* common, int n_pairs,
                                   const double* map_X, int map_n, const double* Rt_source, int* n_common, double* scale, double* Rt, double* Xw)
{
    clc_inter_pose_job jb{};
    jb.map_X = map_X; jb.map_n = map_n; jb.Rt_source = Rt_source;
    clc::InterFront fr{};
    fr.Xt.assign(Xt, Xt + 3 * (size_t)nf); fr.corr.assign((size_t)nf, 0);
    memcpy(fr.R, R, sizeof fr.R); memcpy(fr.t, t, sizeof fr.t);
    std::vector<std::pair<int32_t, int32_t>> com;
    for (int c = 0; c < n_pairs; ++c) com.emplace_back(common[2 * c], common[2 * c + 1]);
    std::vector<double> xw;
    const int stage = clc::inter_scale_pose(jb, fr, com, xw);
    *n_common = jb.n_common; *scale = jb.scale;
    if (stage != CLC_INTER_OK) return stage;
    memcpy(Rt, jb.Rt, sizeof jb.Rt);
    std::copy(xw.begin(), xw.end(), Xw);
    return stage;
}

}

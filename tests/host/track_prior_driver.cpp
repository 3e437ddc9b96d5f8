// track_prior_driver.cpp -- HIPLocalizer::localizeImagePriorDev (the pose from the prediction, clc_track_prior_dev) for
// tests/test_gpu_track_prior_policy.py, which runs the binding of the same entry on the same frame and compares.
// usage: track_prior_driver <dir>    reads <dir>/loc.bin (the layout of localizer_driver.cpp) and <dir>/prior.bin = [Rt_prior (12), gate];
// writes <dir>/prior_out.bin = [status, n_tracks, n_inliers, rmse, R (9, row-major), C (3), cov (36), the prior as the member read it (12), inliers ...].  The member is called
// twice: with the prior, and with a prior every landmark lies behind of (FEW: failure, the pose left as it came in); exit status 0 = the
// second call failed and left the pose alone.
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <fstream>
#include <string>
#include <vector>

#include "HIPLocalizer.hpp"

using namespace openMVG;

static std::vector<double> slurp(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    std::vector<double> v(static_cast<size_t>(f.tellg()) / 8);
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(v.size() * 8));
    return v;
}

// the two HIP runtime calls the driver needs, from the runtime libcoloc_hip.so already brought in (plain C++ host code, no HIP headers)
typedef int (*hip_malloc_t)(void**, size_t);
typedef int (*hip_memcpy_t)(void*, const void*, size_t, int);

static geometry::Pose3 pose_of(const double* Rt)
{
    Mat3 R;
    Vec3 C;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R(i, j) = Rt[4 * i + j];
    for (int i = 0; i < 3; ++i) C[i] = -(R(0, i) * Rt[3] + R(1, i) * Rt[7] + R(2, i) * Rt[11]);
    return geometry::Pose3(R, C);
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s dir\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const hip_malloc_t hip_malloc = reinterpret_cast<hip_malloc_t>(dlsym(RTLD_DEFAULT, "hipMalloc"));
    const hip_memcpy_t hip_memcpy = reinterpret_cast<hip_memcpy_t>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
    if (!hip_malloc || !hip_memcpy) { std::fprintf(stderr, "no HIP runtime in the process\n"); return 2; }
    const std::vector<double> in = slurp(dir + "/loc.bin");
    const std::vector<double> pr = slurp(dir + "/prior.bin");
    if (pr.size() < 13) { std::fprintf(stderr, "prior.bin\n"); return 2; }
    const int w = (int)in[0], h = (int)in[1];
    Mat3 K; K(0, 0) = in[2]; K(1, 1) = in[2]; K(0, 2) = in[3]; K(1, 2) = in[4]; K(2, 2) = 1.0;
    const Vec3 dist(in[5], in[6], in[7]);
    const size_t n_map = (size_t)in[8], n_feat = (size_t)in[9], n_match = (size_t)in[10];
    const double* p = in.data() + 11;
    coloc::colocParams params({ K }, { dist }, 'E', { (size_t)w, (size_t)h }, ".", coloc::DetectorOptions{}, coloc::MatcherOptions{});
    coloc::colocData data;
    for (size_t i = 0; i < n_map; ++i) {
        data.scene.structure[(IndexT)(1000 + i)].X = Vec3(p[3 * i], p[3 * i + 1], p[3 * i + 2]);     // landmark ids are not row numbers
        data.mapRegionIdx.push_back((IndexT)(1000 + i));
    }
    p += 3 * n_map;
    data.regions[0].reset(new features::AKAZE_Binary_Regions);
    std::vector<float> feat4(4 * n_feat);
    for (size_t i = 0; i < n_feat; ++i) {
        data.regions[0]->Features().emplace_back((float)p[2 * i], (float)p[2 * i + 1], 7.0f, 0.0f);
        feat4[4 * i] = (float)p[2 * i]; feat4[4 * i + 1] = (float)p[2 * i + 1]; feat4[4 * i + 2] = 7.0f; feat4[4 * i + 3] = 0.0f;
    }
    p += 2 * n_feat;
    std::vector<int32_t> match(n_feat, -1);
    for (size_t i = 0; i < n_match; ++i) match[(size_t)p[2 * i + 1]] = (int32_t)p[2 * i];

    void *d_match = nullptr, *d_feat = nullptr;
    if (hip_malloc(&d_match, n_feat * 4) != 0 || hip_malloc(&d_feat, n_feat * 16) != 0 ||
        hip_memcpy(d_match, match.data(), n_feat * 4, 1) != 0 || hip_memcpy(d_feat, feat4.data(), n_feat * 16, 1) != 0) {
        std::fprintf(stderr, "device buffers\n");
        return 2;
    }
    int idx = 0;
    coloc::HIPLocalizer loc(params);
    loc.seed = 5;
    if (loc.setMapPoints(data)) { std::fprintf(stderr, "setMapPoints failed\n"); return 2; }
    geometry::Pose3 pose = pose_of(pr.data());
    // the prior as the member reads it back from the Pose3 (R, C): t = pose.translation(), not bit for bit prior.bin's
    double prior_read[12];
    {
        const Vec3 t0 = pose.translation();
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) prior_read[4 * i + j] = pose.rotation()(i, j); prior_read[4 * i + 3] = t0[i]; }
    }
    coloc::Cov6 cov;
    float rmse = -2.0f;
    std::vector<uint32_t> inl;
    matching::IndMatches tracked;
    const bool st = loc.localizeImagePriorDev(idx, pose, pr[12], data, cov, rmse, tracked, inl, (const int32_t*)d_match, (int)n_feat, nullptr,
                                              nullptr, (const float*)d_feat, 4, nullptr);
    std::vector<double> out = { st ? 1.0 : 0.0, (double)tracked.size(), (double)inl.size(), (double)rmse };
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) out.push_back(pose.rotation()(i, j));
    for (int i = 0; i < 3; ++i) out.push_back(pose.center()[i]);
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) out.push_back(cov(i, j));
    for (int i = 0; i < 12; ++i) out.push_back(prior_read[i]);
    for (uint32_t c : inl) out.push_back((double)c);
    std::ofstream f(dir + "/prior_out.bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(out.data()), static_cast<std::streamsize>(out.size() * 8));

    // a prior that looks the other way (a half turn about the camera's x axis): FEW, reported as failure, the pose as it came in
    double back[12];
    for (int j = 0; j < 4; ++j) { back[j] = pr[j]; back[4 + j] = -pr[4 + j]; back[8 + j] = -pr[8 + j]; }
    geometry::Pose3 pose2 = pose_of(back);
    const geometry::Pose3 kept = pose2;
    const auto seed_before = loc.seed;
    const bool st2 = loc.localizeImagePriorDev(idx, pose2, pr[12], data, cov, rmse, tracked, inl, (const int32_t*)d_match, (int)n_feat, nullptr,
                                               nullptr, (const float*)d_feat, 4, nullptr);
    int bad = 0;
    if (!st2) { std::fprintf(stderr, "a prior behind the scene did not fail\n"); ++bad; }
    if (std::memcmp(pose2.rotation().m.data(), kept.rotation().m.data(), 72) != 0 || std::memcmp(pose2.center().v.data(), kept.center().v.data(), 24) != 0) {
        std::fprintf(stderr, "a failed call changed the pose\n");
        ++bad;
    }
    if (!inl.empty() || tracked.size() != n_match) { std::fprintf(stderr, "a failed call: inliers / trackedFeatures\n"); ++bad; }
    if (loc.seed != seed_before || loc.seed != 5) { std::fprintf(stderr, "the member drew a seed\n"); ++bad; }
    return bad == 0 ? 0 : 1;
}

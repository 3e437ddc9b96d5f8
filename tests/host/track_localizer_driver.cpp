// track_localizer_driver.cpp -- HIPLocalizer::localizeImageDev (tracks built on the device, clc_track_localize_dev) against
// setupTracks + localizeImage on the same frame and seed, for tests/test_gpu_track_policy.py.
// usage: track_localizer_driver <dir>    reads <dir>/loc.bin (the layout of localizer_driver.cpp); exit status 0 = every member the two
// calls leave behind (status, pose, covariance, rmse, trackedFeatures, inliers, the next seed) is identical; writes <dir>/track_out.bin
// = [status, n_tracks, n_inliers, rmse, C (3)].
#include <algorithm>
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

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s dir\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const hip_malloc_t hip_malloc = reinterpret_cast<hip_malloc_t>(dlsym(RTLD_DEFAULT, "hipMalloc"));
    const hip_memcpy_t hip_memcpy = reinterpret_cast<hip_memcpy_t>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
    if (!hip_malloc || !hip_memcpy) { std::fprintf(stderr, "no HIP runtime in the process\n"); return 2; }
    const std::vector<double> in = slurp(dir + "/loc.bin");
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
    // matchFeaturesWithMap's output: one map row per accepted query, ascending query (GPUMatcher.hpp:263-266)
    std::vector<int32_t> match(n_feat, -1);
    for (size_t i = 0; i < n_match; ++i) match[(size_t)p[2 * i + 1]] = (int32_t)p[2 * i];
    matching::IndMatches tracked;
    for (size_t q = 0; q < n_feat; ++q) if (match[q] >= 0) tracked.emplace_back((IndexT)match[q], (IndexT)q);

    int idx = 0;
    // (a) today: setupTracks on the host, inside localizeImage
    coloc::HIPLocalizer host(params);
    host.seed = 5;
    geometry::Pose3 pose_a;
    coloc::Cov6 cov_a;
    float rmse_a = -1.0f;
    std::vector<uint32_t> inl_a;
    matching::IndMatches tracked_a = tracked;
    const bool st_a = host.localizeImage(idx, pose_a, data, cov_a, rmse_a, tracked_a, inl_a);
    // (b) the tracks on the device
    void *d_match = nullptr, *d_feat = nullptr;
    if (hip_malloc(&d_match, n_feat * 4) != 0 || hip_malloc(&d_feat, n_feat * 16) != 0 ||
        hip_memcpy(d_match, match.data(), n_feat * 4, 1) != 0 || hip_memcpy(d_feat, feat4.data(), n_feat * 16, 1) != 0) {
        std::fprintf(stderr, "device buffers\n");
        return 2;
    }
    coloc::HIPLocalizer dev(params);
    dev.seed = 5;
    if (dev.setMapPoints(data)) { std::fprintf(stderr, "setMapPoints failed\n"); return 2; }
    geometry::Pose3 pose_b;
    coloc::Cov6 cov_b;
    float rmse_b = -2.0f;
    std::vector<uint32_t> inl_b;
    matching::IndMatches tracked_b;
    const bool st_b = dev.localizeImageDev(idx, pose_b, data, cov_b, rmse_b, tracked_b, inl_b, (const int32_t*)d_match, (int)n_feat, nullptr,
                                           nullptr, (const float*)d_feat, 4, nullptr);
    int bad = 0;
    auto differ = [&](const char* what) { std::fprintf(stderr, "differs: %s\n", what); ++bad; };
    if (st_a != st_b) differ("status");
    if (host.seed != dev.seed) differ("seed");
    if (std::memcmp(pose_a.rotation().m.data(), pose_b.rotation().m.data(), 72) != 0) differ("rotation");
    if (std::memcmp(pose_a.center().v.data(), pose_b.center().v.data(), 24) != 0) differ("center");
    if (std::memcmp(cov_a.m.data(), cov_b.m.data(), 288) != 0) differ("covariance");
    if (std::memcmp(&rmse_a, &rmse_b, 4) != 0) differ("rmse");
    if (inl_a != inl_b) differ("inliers");
    if (tracked_a.size() != tracked_b.size()) differ("trackedFeatures size");
    else
        for (size_t i = 0; i < tracked_a.size(); ++i)
            if (tracked_a[i].i_ != tracked_b[i].i_ || tracked_a[i].j_ != tracked_b[i].j_) { differ("trackedFeatures"); break; }
    const std::vector<double> out = { st_b ? 1.0 : 0.0, (double)tracked_b.size(), (double)inl_b.size(), (double)rmse_b, pose_b.center()[0],
                                      pose_b.center()[1], pose_b.center()[2] };
    std::ofstream f(dir + "/track_out.bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(out.data()), static_cast<std::streamsize>(out.size() * 8));
    return bad == 0 ? 0 : 1;
}

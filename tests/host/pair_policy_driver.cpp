// pair_policy_driver.cpp -- HIPRobustMatcher::filterMatchesPairDev (correspondences built on the device, clc_pair_filter_dev) against
// filterMatchesPair on the same matches and seed, for tests/test_gpu_pair_policy.py.
// usage: pair_policy_driver <dir>    reads <dir>/pair.bin = [w, h, camera A (focal, ppx, ppy, k1, k2, k3), camera B (6), model letter, nq, nt,
// features A (2 nq), features B (2 nt), match (nq)]; exit status 0 = everything the two members leave behind (status, lastStatus, the next
// seed, geometricMatches[pair], relativePoses[pair]: vec_inliers, essential_matrix, found_residual_precision, relativePose) is identical;
// writes <dir>/pair_out.bin = [status, n_putative, n_inliers, R (9), C (3), model matrix (9)].
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <fstream>
#include <string>
#include <vector>

#include "HIPRobustMatcher.hpp"

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
    const std::vector<double> in = slurp(dir + "/pair.bin");
    const int w = (int)in[0], h = (int)in[1];
    std::vector<Mat3> Ks(2);
    std::vector<Vec3> dists(2);
    for (int c = 0; c < 2; ++c) {
        const double* k = in.data() + 2 + 6 * c;
        Ks[c](0, 0) = k[0]; Ks[c](1, 1) = k[0]; Ks[c](0, 2) = k[1]; Ks[c](1, 2) = k[2]; Ks[c](2, 2) = 1.0;
        dists[c] = Vec3(k[3], k[4], k[5]);
    }
    const char model = (char)(int)in[14];
    const size_t nq = (size_t)in[15], nt = (size_t)in[16];
    const double* p = in.data() + 17;
    coloc::colocParams params(Ks, dists, model, { (size_t)w, (size_t)h }, ".", coloc::DetectorOptions{}, coloc::MatcherOptions{});
    coloc::FeatureMap regions;
    std::vector<float> featA(4 * nq), featB(4 * nt);
    regions[0].reset(new features::AKAZE_Binary_Regions);
    regions[1].reset(new features::AKAZE_Binary_Regions);
    for (size_t i = 0; i < nq; ++i) {
        regions[0]->Features().emplace_back((float)p[2 * i], (float)p[2 * i + 1], 7.0f, 0.0f);
        featA[4 * i] = (float)p[2 * i]; featA[4 * i + 1] = (float)p[2 * i + 1]; featA[4 * i + 2] = 7.0f; featA[4 * i + 3] = 0.0f;
    }
    p += 2 * nq;
    for (size_t i = 0; i < nt; ++i) {
        regions[1]->Features().emplace_back((float)p[2 * i], (float)p[2 * i + 1], 7.0f, 0.0f);
        featB[4 * i] = (float)p[2 * i]; featB[4 * i + 1] = (float)p[2 * i + 1]; featB[4 * i + 2] = 7.0f; featB[4 * i + 3] = 0.0f;
    }
    p += 2 * nt;
    std::vector<int32_t> match(nq);
    for (size_t i = 0; i < nq; ++i) match[i] = (int32_t)p[i];
    // GPUMatcher::computeMatches' output for the pair: IndMatch(i, h_matches[i]) for every accepted query, ascending (GPUMatcher.hpp:215-220)
    const Pair pr(0, 1);
    matching::PairWiseMatches putative;
    for (size_t q = 0; q < nq; ++q) if (match[q] >= 0 && (size_t)match[q] < nt) putative[pr].emplace_back((IndexT)q, (IndexT)match[q]);

    // (a) today: the host gather inside computeRelativePose
    coloc::HIPRobustMatcher host(params);
    host.seed = 5;
    matching::PairWiseMatches geo_a;
    coloc::InterPoseMap poses_a;
    const bool st_a = host.filterMatchesPair(pr, regions, putative, geo_a, poses_a);
    // (b) the correspondences on the device
    void *d_match = nullptr, *d_fa = nullptr, *d_fb = nullptr;
    if (hip_malloc(&d_match, nq * 4) != 0 || hip_malloc(&d_fa, nq * 16) != 0 || hip_malloc(&d_fb, nt * 16) != 0 ||
        hip_memcpy(d_match, match.data(), nq * 4, 1) != 0 || hip_memcpy(d_fa, featA.data(), nq * 16, 1) != 0 ||
        hip_memcpy(d_fb, featB.data(), nt * 16, 1) != 0) {
        std::fprintf(stderr, "device buffers\n");
        return 2;
    }
    coloc::HIPRobustMatcher dev(params);
    dev.seed = 5;
    matching::PairWiseMatches geo_b, putative_b;
    coloc::InterPoseMap poses_b;
    const coloc::HIPRobustMatcher::PairSideDev sa{ nullptr, (const float*)d_fa, 4, nullptr }, sb{ nullptr, (const float*)d_fb, 4, nullptr };
    const bool st_b = dev.filterMatchesPairDev(pr, (const int32_t*)d_match, (int)nq, (int)nt, sa, sb, nullptr, geo_b, poses_b, &putative_b);

    int bad = 0;
    auto differ = [&](const char* what) { std::fprintf(stderr, "differs: %s\n", what); ++bad; };
    auto same_matches = [](const matching::IndMatches& x, const matching::IndMatches& y) {
        if (x.size() != y.size()) return false;
        for (size_t i = 0; i < x.size(); ++i) if (x[i].i_ != y[i].i_ || x[i].j_ != y[i].j_) return false;
        return true;
    };
    if (st_a != st_b) differ("status");
    if (host.lastStatus() != dev.lastStatus()) differ("lastStatus");
    if (host.seed != dev.seed) differ("seed");
    if (!same_matches(putative[pr], putative_b[pr])) differ("putative matches");
    if (geo_a.count(pr) != geo_b.count(pr)) differ("geometricMatches entry");
    else if (geo_a.count(pr) && !same_matches(geo_a[pr], geo_b[pr])) differ("geometricMatches");
    if (poses_a.count(pr) != 1 || poses_b.count(pr) != 1) { differ("relativePoses entry"); return 1; }
    const sfm::RelativePose_Info &ra = poses_a[pr], &rb = poses_b[pr];
    if (ra.vec_inliers != rb.vec_inliers) differ("vec_inliers");
    if (std::memcmp(ra.essential_matrix.m.data(), rb.essential_matrix.m.data(), 72) != 0) differ("essential_matrix");
    if (std::memcmp(&ra.found_residual_precision, &rb.found_residual_precision, 8) != 0) differ("found_residual_precision");
    if (std::memcmp(ra.relativePose.rotation().m.data(), rb.relativePose.rotation().m.data(), 72) != 0) differ("relativePose rotation");
    if (std::memcmp(ra.relativePose.center().v.data(), rb.relativePose.center().v.data(), 24) != 0) differ("relativePose center");
    std::vector<double> out = { st_b ? 1.0 : 0.0, (double)putative_b[pr].size(), (double)rb.vec_inliers.size() };
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) out.push_back(rb.relativePose.rotation()(i, j));
    for (int i = 0; i < 3; ++i) out.push_back(rb.relativePose.center()[i]);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) out.push_back(rb.essential_matrix(i, j));
    std::ofstream f(dir + "/pair_out.bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(out.data()), static_cast<std::streamsize>(out.size() * 8));
    return bad == 0 ? 0 : 1;
}

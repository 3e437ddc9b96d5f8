// guided_policy_driver.cpp -- HIPRobustMatcher::guidedMatchesPairDev (the guided match behind the drop-in policy class) for
// tests/test_gpu_guided_match.py, which holds its d_match to clc_match_guided_dev's for the same pair.
// usage: guided_policy_driver <dir>    reads <dir>/guided.bin = doubles [w, h, camera A (focal, ppx, ppy, k1, k2, k3), camera B (6), model
// letter, nq, nt, band, threshold, the model matrix as filterMatchesPair leaves it in relativePoses[pair].essential_matrix (9), features A
// (2 nq), features B (2 nt)] and <dir>/desc.bin = the descriptor rows of A then B (64 bytes each); writes <dir>/guided_out.bin = int32
// d_match (nq).  Exit status 0 = the member returned EXIT_SUCCESS.
#include <cstdio>
#include <dlfcn.h>
#include <fstream>
#include <string>
#include <vector>

#include "HIPRobustMatcher.hpp"

using namespace openMVG;

template <class T> static std::vector<T> slurp(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    std::vector<T> v(static_cast<size_t>(f.tellg()) / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
    return v;
}

// the HIP runtime calls the driver needs, from the runtime libcoloc_hip.so already brought in (plain C++ host code, no HIP headers)
typedef int (*hip_malloc_t)(void**, size_t);
typedef int (*hip_memcpy_t)(void*, const void*, size_t, int);
typedef int (*hip_sync_t)(void);

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s dir\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const hip_malloc_t hip_malloc = reinterpret_cast<hip_malloc_t>(dlsym(RTLD_DEFAULT, "hipMalloc"));
    const hip_memcpy_t hip_memcpy = reinterpret_cast<hip_memcpy_t>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
    const hip_sync_t hip_sync = reinterpret_cast<hip_sync_t>(dlsym(RTLD_DEFAULT, "hipDeviceSynchronize"));
    if (!hip_malloc || !hip_memcpy || !hip_sync) { std::fprintf(stderr, "no HIP runtime in the process\n"); return 2; }
    const std::vector<double> in = slurp<double>(dir + "/guided.bin");
    const std::vector<unsigned char> desc = slurp<unsigned char>(dir + "/desc.bin");
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
    const float band = (float)in[17];
    const int threshold = (int)in[18];
    sfm::RelativePose_Info info;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) info.essential_matrix(i, j) = in[19 + 3 * i + j];
    const double* p = in.data() + 28;
    if (in.size() != 28 + 2 * nq + 2 * nt || desc.size() != 64 * (nq + nt)) { std::fprintf(stderr, "input sizes\n"); return 2; }
    std::vector<float> featA(2 * nq), featB(2 * nt);
    for (size_t i = 0; i < 2 * nq; ++i) featA[i] = (float)p[i];
    p += 2 * nq;
    for (size_t i = 0; i < 2 * nt; ++i) featB[i] = (float)p[i];
    coloc::colocParams params(Ks, dists, model, { (size_t)w, (size_t)h }, ".", coloc::DetectorOptions{}, coloc::MatcherOptions{ 0.8f, 60, 4096u });

    void *d_a = nullptr, *d_b = nullptr, *d_fa = nullptr, *d_fb = nullptr, *d_match = nullptr;
    if (hip_malloc(&d_a, 64 * nq) != 0 || hip_malloc(&d_b, 64 * nt) != 0 || hip_malloc(&d_fa, 8 * nq) != 0 || hip_malloc(&d_fb, 8 * nt) != 0 ||
        hip_malloc(&d_match, 4 * nq) != 0 || hip_memcpy(d_a, desc.data(), 64 * nq, 1) != 0 || hip_memcpy(d_b, desc.data() + 64 * nq, 64 * nt, 1) != 0 ||
        hip_memcpy(d_fa, featA.data(), 8 * nq, 1) != 0 || hip_memcpy(d_fb, featB.data(), 8 * nt, 1) != 0) {
        std::fprintf(stderr, "device buffers\n");
        return 2;
    }
    coloc::HIPRobustMatcher rm(params);
    const coloc::HIPRobustMatcher::PairSideDev sa{ nullptr, (const float*)d_fa, 2, nullptr }, sb{ nullptr, (const float*)d_fb, 2, nullptr };
    const bool st = rm.guidedMatchesPairDev(Pair(0, 1), d_a, (int)nq, d_b, (int)nt, sa, sb, info, band, threshold, (int32_t*)d_match, nullptr);
    std::vector<int32_t> match(nq, -7);
    if (hip_sync() != 0 || hip_memcpy(match.data(), d_match, 4 * nq, 2) != 0) { std::fprintf(stderr, "read back\n"); return 2; }
    std::ofstream f(dir + "/guided_out.bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(match.data()), static_cast<std::streamsize>(match.size() * 4));
    return st == static_cast<bool>(EXIT_SUCCESS) ? 0 : 1;
}

// match_unique_driver.cpp -- HIPMatcher::matchSceneWithMapBinnedUniqueDev and HIPMatcher::computeMatchesPairUnique (the one-to-one filter
// behind the drop-in policy class) for tests/test_gpu_match_unique_policy.py, which holds what they leave to the binding's result on the
// same data.
// usage: match_unique_driver <dir>    reads map_binned_policy_driver's three files -- <dir>/map_binned.bin = doubles [camera (focal, ppx,
// ppy, k1, k2, k3), R (9, row-major), C (3), nq, nm, radius, threshold, the landmarks of the map rows (3 nm)], <dir>/kps.bin = nq
// clc_keypoint rows, <dir>/desc.bin = the descriptor rows of the frame then of the map (64 bytes each) -- and <dir>/pair_a.bin,
// <dir>/pair_b.bin = the descriptor rows of the two cameras of a pair; writes <dir>/map_unique_out.bin = int32 d_match (nq) then d_owner
// (nm), and <dir>/pair_unique_out.bin = int32 (i_, j_) of every IndMatch in order.  Exit status 0 = the members returned EXIT_SUCCESS.
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <fstream>
#include <string>
#include <vector>

#include "HIPMatcher.hpp"

using namespace openMVG;

template <class T> static std::vector<T> slurp(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    std::vector<T> v(static_cast<size_t>(f.tellg()) / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
    return v;
}

static std::unique_ptr<features::AKAZE_Binary_Regions> regions_of(const std::vector<unsigned char>& rows)
{
    std::unique_ptr<features::AKAZE_Binary_Regions> r(new features::AKAZE_Binary_Regions());
    r->Features().resize(rows.size() / 64);
    r->Descriptors().resize(rows.size() / 64);
    if (!rows.empty()) std::memcpy(r->Descriptors().data(), rows.data(), rows.size());
    return r;
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
    const std::vector<double> in = slurp<double>(dir + "/map_binned.bin");
    const std::vector<unsigned char> kps = slurp<unsigned char>(dir + "/kps.bin");
    std::vector<unsigned char> desc = slurp<unsigned char>(dir + "/desc.bin");
    if (in.size() < 22) { std::fprintf(stderr, "input sizes\n"); return 2; }
    const clc_camera_k3 cam{ in[0], in[1], in[2], in[3], in[4], in[5] };
    Mat3 R;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R(i, j) = in[6 + 3 * i + j];
    const geometry::Pose3 predicted(R, Vec3(in[15], in[16], in[17]));
    const size_t nq = (size_t)in[18], nm = (size_t)in[19];
    const float radius = (float)in[20];
    const int threshold = (int)in[21];
    if (in.size() != 22 + 3 * nm || kps.size() != sizeof(clc_keypoint) * nq || desc.size() != 64 * (nq + nm)) { std::fprintf(stderr, "input sizes\n"); return 2; }
    coloc::colocData data;
    for (size_t i = 0; i < nm; ++i) {
        data.scene.structure[(IndexT)(1000 + i)].X = Vec3(in[22 + 3 * i], in[23 + 3 * i], in[24 + 3 * i]);     // landmark ids are not row numbers
        data.mapRegionIdx.push_back((IndexT)(1000 + i));
    }

    void *d_q = nullptr, *d_kps = nullptr, *d_match = nullptr, *d_owner = nullptr;
    if (hip_malloc(&d_q, 64 * nq) != 0 || hip_malloc(&d_kps, kps.size()) != 0 || hip_malloc(&d_match, 4 * nq) != 0 || hip_malloc(&d_owner, 4 * nm) != 0 ||
        hip_memcpy(d_q, desc.data(), 64 * nq, 1) != 0 || hip_memcpy(d_kps, kps.data(), kps.size(), 1) != 0) {
        std::fprintf(stderr, "device buffers\n");
        return 2;
    }
    coloc::HIPMatcher<bool> matcher(coloc::MatcherOptions{ 0.8f, threshold, 4096u });
    matcher.setMapData((int)nm, desc.data() + 64 * nq);
    const bool st_points = matcher.setMapPoints(data);
    const bool st = matcher.matchSceneWithMapBinnedUniqueDev(predicted, cam, d_q, (int)nq, (const clc_keypoint*)d_kps, nullptr, radius, (int32_t*)d_match,
                                                             nullptr, (int32_t*)d_owner);
    std::vector<int32_t> out(nq + nm, -7);
    if (hip_sync() != 0 || hip_memcpy(out.data(), d_match, 4 * nq, 2) != 0 || hip_memcpy(out.data() + nq, d_owner, 4 * nm, 2) != 0) {
        std::fprintf(stderr, "read back\n");
        return 2;
    }
    std::ofstream f(dir + "/map_unique_out.bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(out.data()), static_cast<std::streamsize>(out.size() * 4));

    coloc::FeatureMap regions;
    regions[0] = regions_of(slurp<unsigned char>(dir + "/pair_a.bin"));
    regions[1] = regions_of(slurp<unsigned char>(dir + "/pair_b.bin"));
    matching::IndMatches putative;
    putative.emplace_back((IndexT)5, (IndexT)5);                                    // (the member replaces the list)
    matcher.computeMatchesPairUnique(Pair(0, 1), regions, putative);
    std::vector<int32_t> pairs;
    for (const auto& m : putative) { pairs.push_back((int32_t)m.i_); pairs.push_back((int32_t)m.j_); }
    std::ofstream g(dir + "/pair_unique_out.bin", std::ios::binary);
    g.write(reinterpret_cast<const char*>(pairs.data()), static_cast<std::streamsize>(pairs.size() * 4));
    return (st_points == static_cast<bool>(EXIT_SUCCESS) && st == static_cast<bool>(EXIT_SUCCESS)) ? 0 : 1;
}

// map_binned_policy_driver.cpp -- HIPMatcher::setMapPoints + matchSceneWithMapBinnedDev (the map match around a predicted pose through a
// cell grid, behind the drop-in policy class) for tests/test_gpu_map_binned.py, which holds its d_match to clc_match_map_binned_dev's for
// the same map, pose and frame.
// usage: map_binned_policy_driver <dir>    reads <dir>/map_binned.bin = doubles [camera (focal, ppx, ppy, k1, k2, k3), R (9, row-major),
// C (3), nq, nm, radius, threshold, the landmarks of the map rows (3 nm)], <dir>/kps.bin = nq clc_keypoint rows and <dir>/desc.bin = the
// descriptor rows of the frame then of the map (64 bytes each); writes <dir>/map_binned_out.bin = int32 d_match (nq).  Exit status 0 = both
// members returned EXIT_SUCCESS.
#include <cstdio>
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

    void *d_q = nullptr, *d_kps = nullptr, *d_match = nullptr;
    if (hip_malloc(&d_q, 64 * nq) != 0 || hip_malloc(&d_kps, kps.size()) != 0 || hip_malloc(&d_match, 4 * nq) != 0 ||
        hip_memcpy(d_q, desc.data(), 64 * nq, 1) != 0 || hip_memcpy(d_kps, kps.data(), kps.size(), 1) != 0) {
        std::fprintf(stderr, "device buffers\n");
        return 2;
    }
    coloc::HIPMatcher<bool> matcher(coloc::MatcherOptions{ 0.8f, threshold, 4096u });
    matcher.setMapData((int)nm, desc.data() + 64 * nq);
    const bool st_points = matcher.setMapPoints(data);
    const bool st = matcher.matchSceneWithMapBinnedDev(predicted, cam, d_q, (int)nq, (const clc_keypoint*)d_kps, nullptr, radius, (int32_t*)d_match, nullptr);
    std::vector<int32_t> match(nq, -7);
    if (hip_sync() != 0 || hip_memcpy(match.data(), d_match, 4 * nq, 2) != 0) { std::fprintf(stderr, "read back\n"); return 2; }
    std::ofstream f(dir + "/map_binned_out.bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(match.data()), static_cast<std::streamsize>(match.size() * 4));
    return (st_points == static_cast<bool>(EXIT_SUCCESS) && st == static_cast<bool>(EXIT_SUCCESS)) ? 0 : 1;
}

// map_extend_policy_driver.cpp -- HIPMatcher::extendMapPairDev and HIPLocalizer::appendMapPoints (the map extended in place behind the
// drop-in policy classes) for tests/test_gpu_map_extend_policy.py, which holds what they leave in colocData to the binding's result on
// the same data.
// usage: map_extend_policy_driver <dir>    reads <dir>/extend.bin = doubles [camera A (focal, ppx, ppy, k1, k2, k3), R_a (9, row-major),
// C_a (3), camera B, R_b, C_b, na, nb, nm, band, threshold, max_distance, the landmarks of the map rows (3 nm)], <dir>/desc.bin = the
// descriptor rows of A, of B, then of the map (64 bytes each), <dir>/feat.bin = float positions of A (2 na) then B (2 nb),
// <dir>/track.bin = int32 map matches of A (na) then B (nb); writes <dir>/out.bin = int32 [n_added, n_dropped, rows of the map, then
// mapRegionIdx, then d_track of A and of B as the call left them], <dir>/rows_out.bin = the descriptors of mapRegions,
// <dir>/feat_out.bin = its features' (x, y) floats, <dir>/X_out.bin = the landmark of every mapRegionIdx entry (3 doubles each).
// Exit status 0 = every member returned EXIT_SUCCESS.
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <fstream>
#include <string>
#include <vector>

#include "HIPLocalizer.hpp"
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

template <class T> static void spill(const std::string& path, const std::vector<T>& v)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
}

// the HIP runtime calls the driver needs, from the runtime libcoloc_hip.so already brought in (plain C++ host code, no HIP headers)
typedef int (*hip_malloc_t)(void**, size_t);
typedef int (*hip_memcpy_t)(void*, const void*, size_t, int);
typedef int (*hip_sync_t)(void);

static geometry::Pose3 pose_of(const double* p)
{
    Mat3 R;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R(i, j) = p[3 * i + j];
    return geometry::Pose3(R, Vec3(p[9], p[10], p[11]));
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s dir\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const hip_malloc_t hip_malloc = reinterpret_cast<hip_malloc_t>(dlsym(RTLD_DEFAULT, "hipMalloc"));
    const hip_memcpy_t hip_memcpy = reinterpret_cast<hip_memcpy_t>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
    const hip_sync_t hip_sync = reinterpret_cast<hip_sync_t>(dlsym(RTLD_DEFAULT, "hipDeviceSynchronize"));
    if (!hip_malloc || !hip_memcpy || !hip_sync) { std::fprintf(stderr, "no HIP runtime in the process\n"); return 2; }
    const std::vector<double> in = slurp<double>(dir + "/extend.bin");
    std::vector<unsigned char> desc = slurp<unsigned char>(dir + "/desc.bin");
    const std::vector<float> feat = slurp<float>(dir + "/feat.bin");
    const std::vector<int32_t> track = slurp<int32_t>(dir + "/track.bin");
    if (in.size() < 42) { std::fprintf(stderr, "input sizes\n"); return 2; }
    const clc_camera_k3 cam_a{ in[0], in[1], in[2], in[3], in[4], in[5] }, cam_b{ in[18], in[19], in[20], in[21], in[22], in[23] };
    const geometry::Pose3 pose_a = pose_of(in.data() + 6), pose_b = pose_of(in.data() + 24);
    const size_t na = (size_t)in[36], nb = (size_t)in[37], nm = (size_t)in[38];
    const float band = (float)in[39];
    const int threshold = (int)in[40], max_distance = (int)in[41];
    if (in.size() != 42 + 3 * nm || desc.size() != 64 * (na + nb + nm) || feat.size() != 2 * (na + nb) || track.size() != na + nb || na == 0 || nb == 0) {
        std::fprintf(stderr, "input sizes\n");
        return 2;
    }
    coloc::colocData data;
    data.mapRegions.reset(new features::AKAZE_Binary_Regions());
    data.mapRegions->Features().resize(nm);
    data.mapRegions->Descriptors().resize(nm);
    if (nm) std::memcpy(data.mapRegions->Descriptors().data(), desc.data() + 64 * (na + nb), 64 * nm);
    for (size_t i = 0; i < nm; ++i) {
        data.scene.structure[(IndexT)(1000 + i)].X = Vec3(in[42 + 3 * i], in[43 + 3 * i], in[44 + 3 * i]);     // landmark ids are not row numbers
        data.mapRegionIdx.push_back((IndexT)(1000 + i));
    }
    // the host copy of view A's block: what HIPDetector leaves in data.regions
    data.regions[3].reset(new features::AKAZE_Binary_Regions());
    data.regions[3]->Descriptors().resize(na);
    std::memcpy(data.regions[3]->Descriptors().data(), desc.data(), 64 * na);
    for (size_t i = 0; i < na; ++i) data.regions[3]->Features().emplace_back(feat[2 * i], feat[2 * i + 1], 7.0f, 0.0f);

    void *d_a = nullptr, *d_b = nullptr, *d_fa = nullptr, *d_fb = nullptr, *d_ta = nullptr, *d_tb = nullptr;
    if (hip_malloc(&d_a, 64 * na) != 0 || hip_malloc(&d_b, 64 * nb) != 0 || hip_malloc(&d_fa, 8 * na) != 0 || hip_malloc(&d_fb, 8 * nb) != 0 ||
        hip_malloc(&d_ta, 4 * na) != 0 || hip_malloc(&d_tb, 4 * nb) != 0 ||
        hip_memcpy(d_a, desc.data(), 64 * na, 1) != 0 || hip_memcpy(d_b, desc.data() + 64 * na, 64 * nb, 1) != 0 ||
        hip_memcpy(d_fa, feat.data(), 8 * na, 1) != 0 || hip_memcpy(d_fb, feat.data() + 2 * na, 8 * nb, 1) != 0 ||
        hip_memcpy(d_ta, track.data(), 4 * na, 1) != 0 || hip_memcpy(d_tb, track.data() + na, 4 * nb, 1) != 0) {
        std::fprintf(stderr, "device buffers\n");
        return 2;
    }
    coloc::HIPMatcher<bool> matcher(coloc::MatcherOptions{ 0.8f, threshold, 4096u });
    matcher.setMapData((int)nm, desc.data() + 64 * (na + nb));
    const bool st_points = matcher.setMapPoints(data);

    Mat3 K; K(0, 0) = cam_a.focal; K(1, 1) = cam_a.focal; K(0, 2) = cam_a.ppx; K(1, 2) = cam_a.ppy; K(2, 2) = 1.0;
    coloc::colocParams params({ K }, { Vec3(cam_a.k1, cam_a.k2, cam_a.k3) }, 'E', { (size_t)640, (size_t)480 }, ".", coloc::DetectorOptions{}, coloc::MatcherOptions{});
    coloc::HIPLocalizer localizer(params);
    const bool st_loc = localizer.setMapPoints(data);

    const coloc::HIPMatcher<bool>::ExtendSideDev a{ nullptr, (const float*)d_fa, 2, nullptr, (int32_t*)d_ta }, b{ nullptr, (const float*)d_fb, 2, nullptr, (int32_t*)d_tb };
    int n_added = -1, n_dropped = -1;
    const bool st = matcher.extendMapPairDev(data, Pair(3, 5), d_a, (int)na, d_b, (int)nb, a, b, cam_a, cam_b, pose_a, pose_b, band, max_distance, nullptr,
                                             &n_added, &n_dropped);
    const bool st_append = localizer.appendMapPoints(data, nm);
    const bool st_past = localizer.appendMapPoints(data, data.mapRegionIdx.size() + 1);         // past the end: refused

    std::vector<int32_t> out{ n_added, n_dropped, (int32_t)data.mapRegionIdx.size() };
    for (const IndexT id : data.mapRegionIdx) out.push_back((int32_t)id);
    std::vector<int32_t> tr(na + nb, -7);
    if (hip_sync() != 0 || hip_memcpy(tr.data(), d_ta, 4 * na, 2) != 0 || hip_memcpy(tr.data() + na, d_tb, 4 * nb, 2) != 0) {
        std::fprintf(stderr, "read back\n");
        return 2;
    }
    out.insert(out.end(), tr.begin(), tr.end());
    spill(dir + "/out.bin", out);
    std::vector<unsigned char> rows(64 * data.mapRegions->Descriptors().size());
    if (!rows.empty()) std::memcpy(rows.data(), data.mapRegions->Descriptors().data(), rows.size());
    spill(dir + "/rows_out.bin", rows);
    std::vector<float> fo;
    for (const auto& f : data.mapRegions->Features()) { fo.push_back(f.x()); fo.push_back(f.y()); }
    spill(dir + "/feat_out.bin", fo);
    std::vector<double> X;
    for (const IndexT id : data.mapRegionIdx) for (int r = 0; r < 3; ++r) X.push_back(data.scene.GetLandmarks().at(id).X[r]);
    spill(dir + "/X_out.bin", X);
    const bool ok = static_cast<bool>(EXIT_SUCCESS);
    return (st_points == ok && st_loc == ok && st == ok && st_append == ok && st_past != ok) ? 0 : 1;
}

// map_cull_policy_driver.cpp -- HIPMatcher::observeMapDev, HIPMatcher::cullMapDev and HIPLocalizer::cullMapPoints (the map culled in place
// behind the drop-in policy classes), then HIPMatcher::extendMapPairDev and HIPLocalizer::appendMapPoints on the same colocData, for
// tests/test_gpu_map_cull_policy.py, which holds the matcher's context, the localizer's context and the host-side database to one another.
// usage: map_cull_policy_driver <dir>    reads the files of tests/host/map_extend_policy_driver.cpp (extend.bin, desc.bin, feat.bin,
// track.bin) with one more double behind max_distance: the number of observe calls; writes <dir>/out.bin = int32 [removed, n_added,
// n_dropped, rows of mapRegionIdx, landmarks of the scene, rows of mapRegions, the matcher context's rows (clc_map_stats_get), the rows
// its match of mapRegions' descriptors names in order (1 / 0), then mapRegionIdx, the remap (nm), d_track of A and of B as the calls
// left them], <dir>/X_db.bin = the scene's landmark of every mapRegionIdx entry, <dir>/X_matcher.bin and <dir>/X_localizer.bin = the
// points the two contexts hold at those rows (3 doubles each), <dir>/rows_out.bin = the descriptors of mapRegions.
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
static hip_malloc_t hip_malloc;
static hip_memcpy_t hip_memcpy;
static hip_sync_t hip_sync;

static geometry::Pose3 pose_of(const double* p)
{
    Mat3 R;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R(i, j) = p[3 * i + j];
    return geometry::Pose3(R, Vec3(p[9], p[10], p[11]));
}

// the first n points a context holds, in row order: clc_track_build_dev of the identity list
static bool points_of(clc_ctx* ctx, size_t n, const clc_camera_k3& cam, std::vector<double>& X)
{
    X.assign(3 * n, 0.0);
    if (n == 0) return true;
    std::vector<int32_t> ident(n);
    for (size_t i = 0; i < n; ++i) ident[i] = (int32_t)i;
    const std::vector<float> feat(2 * n, 0.0f);
    void *d_id = nullptr, *d_feat = nullptr, *d_X = nullptr, *d_x = nullptr, *d_n = nullptr;
    int32_t got = -1;
    if (hip_malloc(&d_id, 4 * n) != 0 || hip_malloc(&d_feat, 8 * n) != 0 || hip_malloc(&d_X, 24 * n) != 0 || hip_malloc(&d_x, 16 * n) != 0 ||
        hip_malloc(&d_n, 64) != 0 || hip_memcpy(d_id, ident.data(), 4 * n, 1) != 0 || hip_memcpy(d_feat, feat.data(), 8 * n, 1) != 0)
        return false;
    clc_track_job jb{};
    jb.d_match = (const int32_t*)d_id; jb.nq = (int)n; jb.d_feat = (const float*)d_feat; jb.feat_stride = 2; jb.cam = cam;
    if (clc_track_build_dev(ctx, &jb, (double*)d_X, (double*)d_x, nullptr, nullptr, (int32_t*)d_n, nullptr) != CLC_OK) return false;
    if (clc_sync(ctx) != CLC_OK || hip_sync() != 0 || hip_memcpy(&got, d_n, 4, 2) != 0 || hip_memcpy(X.data(), d_X, 24 * n, 2) != 0) return false;
    return got == (int32_t)n;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s dir\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    hip_malloc = reinterpret_cast<hip_malloc_t>(dlsym(RTLD_DEFAULT, "hipMalloc"));
    hip_memcpy = reinterpret_cast<hip_memcpy_t>(dlsym(RTLD_DEFAULT, "hipMemcpy"));
    hip_sync = reinterpret_cast<hip_sync_t>(dlsym(RTLD_DEFAULT, "hipDeviceSynchronize"));
    if (!hip_malloc || !hip_memcpy || !hip_sync) { std::fprintf(stderr, "no HIP runtime in the process\n"); return 2; }
    const std::vector<double> in = slurp<double>(dir + "/extend.bin");
    std::vector<unsigned char> desc = slurp<unsigned char>(dir + "/desc.bin");
    const std::vector<float> feat = slurp<float>(dir + "/feat.bin");
    const std::vector<int32_t> track = slurp<int32_t>(dir + "/track.bin");
    if (in.size() < 43) { std::fprintf(stderr, "input sizes\n"); return 2; }
    const clc_camera_k3 cam_a{ in[0], in[1], in[2], in[3], in[4], in[5] }, cam_b{ in[18], in[19], in[20], in[21], in[22], in[23] };
    const geometry::Pose3 pose_a = pose_of(in.data() + 6), pose_b = pose_of(in.data() + 24);
    const size_t na = (size_t)in[36], nb = (size_t)in[37], nm = (size_t)in[38];
    const float band = (float)in[39];
    const int threshold = (int)in[40], max_distance = (int)in[41], n_observes = (int)in[42];
    if (in.size() != 43 + 3 * nm || desc.size() != 64 * (na + nb + nm) || feat.size() != 2 * (na + nb) || track.size() != na + nb || na == 0 || nb == 0) {
        std::fprintf(stderr, "input sizes\n");
        return 2;
    }
    coloc::colocData data;
    data.mapRegions.reset(new features::AKAZE_Binary_Regions());
    data.mapRegions->Features().resize(nm);
    data.mapRegions->Descriptors().resize(nm);
    if (nm) std::memcpy(data.mapRegions->Descriptors().data(), desc.data() + 64 * (na + nb), 64 * nm);
    for (size_t i = 0; i < nm; ++i) {
        data.scene.structure[(IndexT)(1000 + i)].X = Vec3(in[43 + 3 * i], in[44 + 3 * i], in[45 + 3 * i]);     // landmark ids are not row numbers
        data.mapRegionIdx.push_back((IndexT)(1000 + i));
    }
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
    const bool ok = static_cast<bool>(EXIT_SUCCESS);

    // the frames of view A observe the map, then the cull, on both contexts
    bool st_observe = ok;
    for (int f = 0; f < n_observes; ++f)
        if (matcher.observeMapDev(pose_a, cam_a, (int)na, nullptr, (const float*)d_fa, 2, nullptr, (const int32_t*)d_ta, 640, 480, 3.0f, 0.0f, nullptr) != ok) st_observe = !ok;
    int removed = -1;
    std::vector<int32_t> remap;
    const coloc::HIPMatcher<bool>::CullRule rule;
    const bool st_cull = matcher.cullMapDev(data, rule, { { (int32_t*)d_ta, (int)na }, { (int32_t*)d_tb, (int)nb } }, nullptr, &removed, &remap);
    const bool st_cull_points = localizer.cullMapPoints(data, remap);
    std::vector<int32_t> short_remap(remap.begin(), remap.end() - (remap.empty() ? 0 : 1));
    const bool st_short = localizer.cullMapPoints(data, short_remap);              // not one entry per point: refused
    // and the extension finds room behind the surviving rows
    const size_t first = data.mapRegionIdx.size();
    const coloc::HIPMatcher<bool>::ExtendSideDev a{ nullptr, (const float*)d_fa, 2, nullptr, (int32_t*)d_ta }, b{ nullptr, (const float*)d_fb, 2, nullptr, (int32_t*)d_tb };
    int n_added = -1, n_dropped = -1;
    const bool st_extend = matcher.extendMapPairDev(data, Pair(3, 5), d_a, (int)na, d_b, (int)nb, a, b, cam_a, cam_b, pose_a, pose_b, band, max_distance, nullptr,
                                                    &n_added, &n_dropped);
    const bool st_append = localizer.appendMapPoints(data, first);

    // the three holders of the map
    const size_t rows = data.mapRegionIdx.size();
    int ctx_rows = -1;
    if (clc_map_stats_get(matcher.context(), nullptr, nullptr, nullptr, nullptr, &ctx_rows) != CLC_OK) { std::fprintf(stderr, "stats\n"); return 2; }
    std::vector<int32_t> match(rows, -7);
    int in_order = 1;
    if (rows && clc_match_map(matcher.context(), data.mapRegions->Descriptors().data(), (int)rows, 40, match.data()) != CLC_OK) { std::fprintf(stderr, "match\n"); return 2; }
    for (size_t i = 0; i < rows; ++i) if (match[i] != (int32_t)i) in_order = 0;
    std::vector<double> X_db, X_m, X_l;
    for (const IndexT id : data.mapRegionIdx) for (int r = 0; r < 3; ++r) X_db.push_back(data.scene.GetLandmarks().at(id).X[r]);
    if (!points_of(matcher.context(), rows, cam_a, X_m) || !points_of(localizer.context(), rows, cam_a, X_l)) { std::fprintf(stderr, "points\n"); return 2; }

    std::vector<int32_t> out{ removed, n_added, n_dropped, (int32_t)rows, (int32_t)data.scene.structure.size(), (int32_t)data.mapRegions->RegionCount(), ctx_rows,
                              in_order };
    for (const IndexT id : data.mapRegionIdx) out.push_back((int32_t)id);
    out.insert(out.end(), remap.begin(), remap.end());
    std::vector<int32_t> tr(na + nb, -7);
    if (hip_sync() != 0 || hip_memcpy(tr.data(), d_ta, 4 * na, 2) != 0 || hip_memcpy(tr.data() + na, d_tb, 4 * nb, 2) != 0) {
        std::fprintf(stderr, "read back\n");
        return 2;
    }
    out.insert(out.end(), tr.begin(), tr.end());
    spill(dir + "/out.bin", out);
    spill(dir + "/X_db.bin", X_db);
    spill(dir + "/X_matcher.bin", X_m);
    spill(dir + "/X_localizer.bin", X_l);
    std::vector<unsigned char> rows_out(64 * data.mapRegions->Descriptors().size());
    if (!rows_out.empty()) std::memcpy(rows_out.data(), data.mapRegions->Descriptors().data(), rows_out.size());
    spill(dir + "/rows_out.bin", rows_out);
    return (st_points == ok && st_loc == ok && st_observe == ok && st_cull == ok && st_cull_points == ok && st_short != ok && st_extend == ok &&
            st_append == ok) ? 0 : 1;
}

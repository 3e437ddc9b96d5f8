// match_maps_sim_driver.cpp -- HIPRobustMatcher::matchMapsSimilarity driven from C++ the way a caller of matchMaps would drive it; dumps
// raw doubles for tests/test_gpu_match_maps_similarity.py.
// usage: match_maps_sim_driver <dir>   reads <dir>/maps.bin: [n_old, n_new, n_common, old X (3 n_old), new X (3 n_new), i (n_common), j (n_common)]
//                                      writes <dir>/maps_out.bin: [status, s, R (9), t (3), n_left, (i, j) of every common feature left]
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "HIPRobustMatcher.hpp"

using namespace openMVG;

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s dir\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    std::ifstream f(dir + "/maps.bin", std::ios::binary | std::ios::ate);
    std::vector<double> in(static_cast<size_t>(f.tellg()) / 8);
    f.seekg(0);
    f.read(reinterpret_cast<char*>(in.data()), static_cast<std::streamsize>(in.size() * 8));
    const size_t n_old = (size_t)in[0], n_new = (size_t)in[1], n_common = (size_t)in[2];
    const double* p = in.data() + 3;
    std::vector<Vec3> oldX, newX;
    for (size_t i = 0; i < n_old; ++i, p += 3) oldX.emplace_back(p[0], p[1], p[2]);
    for (size_t i = 0; i < n_new; ++i, p += 3) newX.emplace_back(p[0], p[1], p[2]);
    std::vector<matching::IndMatch> common;
    for (size_t k = 0; k < n_common; ++k) common.emplace_back((IndexT)p[k], (IndexT)p[n_common + k]);
    Mat3 K; K(0, 0) = 1000.0; K(1, 1) = 1000.0; K(0, 2) = 640.0; K(1, 2) = 360.0; K(2, 2) = 1.0;
    coloc::colocParams params({ K, K }, { Vec3(0, 0, 0), Vec3(0, 0, 0) }, 'E', { (size_t)1280, (size_t)720 }, ".", coloc::DetectorOptions{},
                              coloc::MatcherOptions{});
    coloc::HIPRobustMatcher robust(params);
    double s = 0.0;
    Mat3 R;
    Vec3 t;
    const bool status = robust.matchMapsSimilarity(oldX, newX, common, s, R, t);
    std::vector<double> out = { status ? 1.0 : 0.0, s };
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) out.push_back(R(i, j));
    for (int i = 0; i < 3; ++i) out.push_back(t[i]);
    out.push_back((double)common.size());
    for (const matching::IndMatch& m : common) { out.push_back(m.i_); out.push_back(m.j_); }
    std::ofstream o(dir + "/maps_out.bin", std::ios::binary);
    o.write(reinterpret_cast<const char*>(out.data()), static_cast<std::streamsize>(out.size() * 8));
    return 0;
}

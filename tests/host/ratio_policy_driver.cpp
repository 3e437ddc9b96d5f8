// ratio_policy_driver.cpp -- exercises HIPRatioMatcher<bool> the way ColoC's non-CUDA build drives CPUMatcher (reference
// include/coloc/coloc.hpp:66-68, :162, :219, :287, :323) and dumps the IndMatch lists for tests/test_gpu_ratio_policy.py to compare with
// the oracle.  usage: ratio_policy_driver <dir> <ncams> <maxkp>; <dir>/desc<c>.bin (n x 64 B) and <dir>/xy<c>.bin (n x 2 float) per camera.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "HIPRatioMatcher.hpp"

using namespace openMVG;
using namespace openMVG::matching;

template <typename T, template <class> class ProcessorType>
class FeatureMatcher : public ProcessorType<T> {    // reference FeatureMatcher.hpp:23-34
public:
    explicit FeatureMatcher(coloc::MatcherOptions& opts) : ProcessorType<T>(opts) {}
    bool computeMatches(coloc::FeatureMap& regions, PairWiseMatches& putativeMatches)
    {
        return ProcessorType<T>::computeMatches(regions, putativeMatches);
    }
};

static std::vector<char> slurp(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void dump_matches(const std::string& path, const IndMatches& m)
{
    std::vector<uint32_t> flat;
    for (const auto& e : m) { flat.push_back(e.i_); flat.push_back(e.j_); }
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(flat.data()), static_cast<std::streamsize>(flat.size() * 4));
}
// an AKAZE_Binary_Regions block from the raw files: positions into the features, descriptors as they are
static std::unique_ptr<features::AKAZE_Binary_Regions> load_regions(const std::string& dir, int c)
{
    const std::vector<char> d = slurp(dir + "/desc" + std::to_string(c) + ".bin");
    const std::vector<char> xy = slurp(dir + "/xy" + std::to_string(c) + ".bin");
    const size_t n = d.size() / 64;
    if (d.size() != n * 64 || xy.size() != n * 8) return nullptr;
    std::unique_ptr<features::AKAZE_Binary_Regions> r(new features::AKAZE_Binary_Regions);
    const float* p = reinterpret_cast<const float*>(xy.data());
    for (size_t i = 0; i < n; ++i) {
        r->Features().emplace_back(p[2 * i], p[2 * i + 1], 1.0f, 0.0f);
        features::AKAZE_Binary_Regions::DescriptorT desc;
        for (size_t k = 0; k < 64; ++k) desc[k] = static_cast<unsigned char>(d[64 * i + k]);
        r->Descriptors().push_back(desc);
    }
    return r;
}

int main(int argc, char** argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: %s dir ncams maxkp\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    const int ncams = std::atoi(argv[2]);
    coloc::MatcherOptions mopts{ 0.8f, 60, static_cast<unsigned>(std::atoi(argv[3])) };      // coloc_node.cpp:83-85
    FeatureMatcher<bool, coloc::HIPRatioMatcher> matcher(mopts);

    coloc::colocData data;
    for (int c = 0; c < ncams; ++c) {
        data.regions[c] = load_regions(dir, c);
        if (!data.regions[c]) { std::fprintf(stderr, "bad input files for camera %d\n", c); return 1; }
    }
    std::ofstream rc(dir + "/rc.txt");
    // initMap: all pairs (coloc.hpp:162)
    PairWiseMatches putative;
    rc << "computeMatches " << matcher.computeMatches(data.regions, putative) << "\n";
    for (const auto& kv : putative)
        dump_matches(dir + "/pair_" + std::to_string(kv.first.first) + "_" + std::to_string(kv.first.second) + ".bin", kv.second);
    // interPoseEstimator: one pair (coloc.hpp:287), default and explicit ratio
    IndMatches one;
    rc << "computeMatchesPair " << matcher.computeMatchesPair({ 0, 1 }, data.regions, one) << "\n";
    dump_matches(dir + "/single_0_1.bin", one);
    rc << "computeMatchesPair06 " << matcher.computeMatchesPair({ 0, 1 }, data.regions, one, 0.6f) << "\n";
    dump_matches(dir + "/single06_0_1.bin", one);
    // map <-> map (coloc.hpp:323): database = first map
    std::vector<IndMatch> common;
    rc << "matchMapFeatures " << matcher.matchMapFeatures(data.regions[0], data.regions[1], common) << "\n";
    dump_matches(dir + "/mapmap_0_1.bin", common);
    // map tracking (coloc.hpp:219): the map is camera 0's regions, the query camera 1
    data.mapRegions = load_regions(dir, 0);
    matcher.setMapData(static_cast<int>(data.mapRegions->RegionCount()), const_cast<void*>(data.mapRegions->DescriptorRawData()));
    IndMatches tracked;
    rc << "matchSceneWithMap " << matcher.matchSceneWithMap(1, data, tracked) << "\n";
    dump_matches(dir + "/map_1.bin", tracked);
    // camera 2 has no regions (its position vector and descriptor block are empty, data() == nullptr): CPUMatcher answers with empty
    // lists and EXIT_SUCCESS, and EXIT_FAILURE when map tracking finds nothing
    IndMatches none;
    rc << "matchSceneWithMapEmpty " << matcher.matchSceneWithMap(2, data, none) << " " << none.size() << "\n";
    IndMatches e02, e20;
    std::vector<IndMatch> e_map;
    rc << "computeMatchesPairEmpty " << matcher.computeMatchesPair({ 0, 2 }, data.regions, e02) << " " << e02.size() << "\n";
    rc << "computeMatchesPairEmptyDb " << matcher.computeMatchesPair({ 2, 0 }, data.regions, e20) << " " << e20.size() << "\n";
    rc << "matchMapFeaturesEmpty " << matcher.matchMapFeatures(data.regions[0], data.regions[2], e_map) << " " << e_map.size() << "\n";
    return 0;
}

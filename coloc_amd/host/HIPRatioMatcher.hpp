// HIPRatioMatcher.hpp -- drop-in for coloc::CPUMatcher<T> (reference include/coloc/CPUMatcher.hpp:22-102), the matcher of every
// non-CUDA build of ColoC (coloc.hpp:66-68), over the C ABI of libcoloc_hip.so (include/coloc_hip.h).
//
// Same public surface and index conventions, member for member:
//   HIPRatioMatcher(MatcherOptions&)                   the options are ignored, as CPUMatcher ignores them (:32-36)
//   computeMatches(FeatureMap&, PairWiseMatches&)      all (first < second) pairs, empty results not inserted (:38-54)
//   matchMapFeatures(scene1, scene2, out)              database = scene1, queries = scene2, ratio 0.8 (:56-65)
//   computeMatchesPair(pair, regions, out, distRatio)  database = regions[first], queries = regions[second] (:67-76)
//   matchSceneWithMap(idx, data, out)                  database = data.mapRegions, queries = data.regions[idx], ratio 0.8;
//                                                      EXIT_FAILURE when nothing is tracked (:78-97)
//   setMapData(n, desc)                                a no-op, as in CPUMatcher (:99-100): the map is data.mapRegions
// Every call is openMVG::matching::DistanceRatioMatch(ratio, BRUTE_FORCE_HAMMING, database, queries) there; here the GPU sweep with
// the ratio rule (clc_match_ratio_pairs / clc_match_ratio_2nn), IndMatch(i_ = database row, j_ = query row), de-duplicated and ordered
// by (x_I, y_I, x_J, y_J, i_, j_) over the regions' GetRegionsPositions() -- the project's statement of OpenMVG's behaviour, not
// pinned against OpenMVG (include/coloc_hip.h).  T carries EXIT_SUCCESS / EXIT_FAILURE; nothing aborts.
#pragma once

#include <cstdlib>
#include <iostream>
#include <memory>
#include <vector>

#include "coloc_hip.h"
#include "coloc_hip_types.hpp"

static_assert(CLC_ABI_VERSION >= 4, "this policy header uses the distance-ratio entry points (clc_match_ratio_pairs, clc_match_map_ratio)");

namespace coloc {

template <typename T>
class HIPRatioMatcher {
public:
    // CPUMatcher keeps nothing of its options; the context takes maxkp (the pair entries are not bounded by it)
    explicit HIPRatioMatcher(MatcherOptions& opts)
    {
        clc_matcher_opts m;
        m.distRatio = kRatio;
        m.thresh = opts.thresh;
        m.maxkp = opts.maxkp;
        const int rc = clc_ctx_create(0, nullptr, &m, &ctx_);
        if (rc != CLC_OK) {
            std::cerr << "HIPRatioMatcher: clc_ctx_create failed: " << clc_status_string(rc) << std::endl;
            ctx_ = nullptr;
        }
        if (clc_abi_version() != CLC_ABI_VERSION)
            std::cerr << "HIPRatioMatcher: libcoloc_hip reports ABI version " << clc_abi_version() << ", this header was written for " << CLC_ABI_VERSION << std::endl;
    }
    HIPRatioMatcher(const HIPRatioMatcher&) = delete;
    HIPRatioMatcher& operator=(const HIPRatioMatcher&) = delete;
    ~HIPRatioMatcher()
    {
        if (ctx_) clc_ctx_destroy(ctx_);
    }

    T computeMatches(FeatureMap& regions, openMVG::matching::PairWiseMatches& putativeMatches)
    {
        const int numImages = static_cast<int>(regions.size());
        const openMVG::Pair_Set pairs = Utils::handlePairs(numImages);
        if (pairs.empty()) return EXIT_SUCCESS;
        // one upload per camera, one launch group for all pairs
        std::vector<const void*> descs(numImages, nullptr);
        std::vector<int> counts(numImages, 0);
        std::vector<std::vector<float>> xy(numImages);
        std::vector<const float*> xyp(numImages, nullptr);
        for (const auto& kv : regions) {
            if (static_cast<int>(kv.first) >= numImages) return EXIT_FAILURE;   // handlePairs assumes ids 0..n-1
            descs[kv.first] = kv.second->DescriptorRawData();
            counts[kv.first] = static_cast<int>(kv.second->RegionCount());
            xy[kv.first] = positions(*kv.second);
            xyp[kv.first] = xy[kv.first].data();
        }
        std::vector<int> flat;
        std::vector<std::vector<int32_t>> out;
        for (const auto& p : pairs) {
            flat.push_back(static_cast<int>(p.first));
            flat.push_back(static_cast<int>(p.second));
            out.emplace_back(2 * static_cast<size_t>(counts[p.second]) + 2);
        }
        std::vector<int32_t*> optr;
        for (auto& o : out) optr.push_back(o.data());
        std::vector<int> n(pairs.size(), 0);
        if (!check(clc_match_ratio_pairs(ctx_, descs.data(), counts.data(), numImages, xyp.data(), flat.data(), static_cast<int>(pairs.size()),
                                         kRatio, optr.data(), n.data()), "computeMatches"))
            return EXIT_FAILURE;
        size_t k = 0;
        for (const auto& pairIdx : pairs) {
            openMVG::matching::IndMatches pairMatches = toIndMatches(out[k], n[k]);
            ++k;
            if (!pairMatches.empty()) putativeMatches.insert({ pairIdx, std::move(pairMatches) });
        }
        return EXIT_SUCCESS;
    }

    bool matchMapFeatures(std::unique_ptr<openMVG::features::AKAZE_Binary_Regions>& scene1,
                          std::unique_ptr<openMVG::features::AKAZE_Binary_Regions>& scene2,
                          std::vector<openMVG::matching::IndMatch>& commonFeatures)
    {
        if (!matchPair(*scene1, *scene2, kRatio, commonFeatures, "matchMapFeatures")) return EXIT_FAILURE;
        return EXIT_SUCCESS;
    }

    bool computeMatchesPair(const openMVG::Pair& pairIdx, FeatureMap& regions, openMVG::matching::IndMatches& putativeMatches,
                            float distRatio = 0.8f)
    {
        if (!matchPair(*regions.at(pairIdx.first), *regions.at(pairIdx.second), distRatio, putativeMatches, "computeMatchesPair"))
            return EXIT_FAILURE;
        return EXIT_SUCCESS;
    }

    // The map is read from data.mapRegions in every call, as CPUMatcher reads it (:85-89): its rows are uploaded (64 B each) and its
    // positions gathered per call (for a 10k-row map: 640 KB up, one sweep, the de-duplication sort).  It is not cached through
    // clc_set_map: the non-CUDA build never calls setMapData (coloc.hpp:196-198, :456-458 are under USE_CUDA) and replaces the map when
    // it updates it (data = updateData, :453-454), so a copy cached here could go stale.
    bool matchSceneWithMap(unsigned int idx, colocData& data, openMVG::matching::IndMatches& trackedFeatures)
    {
        trackedFeatures.clear();
        if (!data.mapRegions || data.regions.find(idx) == data.regions.end()) {
            std::cerr << "HIPRatioMatcher::matchSceneWithMap: no map or no regions for camera " << idx << std::endl;
            return EXIT_FAILURE;
        }
        if (!matchPair(*data.mapRegions, *data.regions.at(idx), kRatio, trackedFeatures, "matchSceneWithMap")) return EXIT_FAILURE;
        if (trackedFeatures.empty()) {
            std::cout << "Unable to track any features" << std::endl;
            return EXIT_FAILURE;
        }
        std::cout << "Number of tracked features: " << trackedFeatures.size() << std::endl;
        return EXIT_SUCCESS;
    }

    void setMapData(int kpMapNum, void* desc)
    {
        (void)kpMapNum;
        (void)desc;
    }

    const char* lastError() const { return ctx_ ? clc_last_error_string(ctx_) : "no context"; }

private:
    static constexpr float kRatio = 0.8f;     // CPUMatcher.hpp:59, :86

    static std::vector<float> positions(const openMVG::features::AKAZE_Binary_Regions& r)
    {
        std::vector<float> xy;
        const auto pts = r.GetRegionsPositions();
        xy.reserve(2 * pts.size());
        for (const auto& p : pts) {
            xy.push_back(static_cast<float>(p.x()));
            xy.push_back(static_cast<float>(p.y()));
        }
        return xy;
    }

    static openMVG::matching::IndMatches toIndMatches(const std::vector<int32_t>& flat, int n)
    {
        openMVG::matching::IndMatches m;
        m.reserve(static_cast<size_t>(n));
        for (int k = 0; k < n; ++k)
            m.emplace_back(static_cast<openMVG::IndexT>(flat[2 * static_cast<size_t>(k)]), static_cast<openMVG::IndexT>(flat[2 * static_cast<size_t>(k) + 1]));
        return m;
    }

    // DistanceRatioMatch(ratio, BRUTE_FORCE_HAMMING, database, queries, out) as one-pair clc_match_ratio_pairs (camera 0 = database)
    bool matchPair(const openMVG::features::AKAZE_Binary_Regions& database, const openMVG::features::AKAZE_Binary_Regions& queries,
                   float ratio, openMVG::matching::IndMatches& out, const char* what)
    {
        out.clear();
        const int counts[2] = { static_cast<int>(database.RegionCount()), static_cast<int>(queries.RegionCount()) };
        const void* descs[2] = { database.DescriptorRawData(), queries.DescriptorRawData() };
        const std::vector<float> xy0 = positions(database), xy1 = positions(queries);
        const float* xy[2] = { xy0.data(), xy1.data() };
        const int pair[2] = { 0, 1 };
        std::vector<int32_t> flat(2 * static_cast<size_t>(counts[1]) + 2);
        int32_t* optr = flat.data();
        int n = 0;
        if (!check(clc_match_ratio_pairs(ctx_, descs, counts, 2, xy, pair, 1, ratio, &optr, &n), what)) return false;
        out = toIndMatches(flat, n);
        return true;
    }

    bool check(int rc, const char* what)
    {
        if (rc == CLC_OK) return true;
        std::cerr << "HIPRatioMatcher::" << what << ": " << clc_status_string(rc) << ": " << lastError() << std::endl;
        return false;
    }

    clc_ctx* ctx_ = nullptr;
};

} // namespace coloc

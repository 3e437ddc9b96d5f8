// HIPMatcher.hpp -- drop-in for coloc::GPUMatcher<T> (reference include/coloc/GPUMatcher.hpp:46-272)
// over the C ABI of libcoloc_hip.so (include/coloc_hip.h).
//
// Same public surface and index conventions:
//   computeMatches(FeatureMap&, PairWiseMatches&)      all (first < second) pairs, empty results not inserted (:143-155)
//   computeMatchesPair(pair, regions, out)             IndMatch(i_ = query idx in regions[first], j_ = train idx in regions[second]), thr 40 (:165-172,:217)
//   matchMapFeatures(map1, map2, out)                  IndMatch(i_ = map1 idx, j_ = map2 idx), thr 60 (:157-163)
//   setMapData(n, desc) / matchSceneWithMap(id, data, out) / matchFeaturesWithMap()
//                                                      IndMatch(i_ = MAP idx, j_ = query idx), thr = MatcherOptions.thresh (:110-117,:174-178,:252-271)
//   setTrainingImage / setQueryImage / computeMatchesPreset (:120-141,:229-250), freeGPUMemory, maxkpNum, dmatches
// Only accepted queries are emitted, in ascending query order.  T carries EXIT_SUCCESS / EXIT_FAILURE.
// Differences underneath: no +8-vector over-read of the caller's buffers (:183-190), explicit
// capacity errors instead of silent overflow, one upload per camera and one launch group for the
// whole all-pairs loop, no texture objects.
#pragma once

#include <cstdlib>
#include <iostream>
#include <memory>
#include <vector>

#include "coloc_hip.h"
#include "coloc_hip_geometry.hpp"
#include "coloc_hip_types.hpp"

static_assert(CLC_ABI_VERSION >= 3, "this policy header uses entry points of ABI version 3 (clc_detect_and_describe_view, clc_desc_handle)");

namespace coloc {

template <typename T>
class HIPMatcher {
public:
    unsigned int maxkpNum;
    std::vector<HipDMatch> dmatches;

    explicit HIPMatcher(MatcherOptions opts) : maxkpNum(opts.maxkp), matchThreshold_(static_cast<uint8_t>(opts.thresh))
    {
        clc_matcher_opts m;
        m.distRatio = opts.distRatio;
        m.thresh = opts.thresh;
        m.maxkp = opts.maxkp;
        const int rc = clc_ctx_create(0, nullptr, &m, &ctx_);
        if (rc != CLC_OK) {
            std::cerr << "HIPMatcher: clc_ctx_create failed: " << clc_status_string(rc) << std::endl;
            ctx_ = nullptr;
        }
        // the library a host was LINKED against and the header it was COMPILED against must agree; a mismatch is reported, the calls
        // that exist in both still work
        if (clc_abi_version() != CLC_ABI_VERSION)
            std::cerr << "HIPMatcher: libcoloc_hip reports ABI version " << clc_abi_version() << ", this header was written for " << CLC_ABI_VERSION << std::endl;
    }
    HIPMatcher(const HIPMatcher&) = delete;
    HIPMatcher& operator=(const HIPMatcher&) = delete;
    ~HIPMatcher() { freeGPUMemory(); }

    void freeGPUMemory()
    {
        if (ctx_) clc_ctx_destroy(ctx_);
        ctx_ = nullptr;
    }

    // Descriptor blocks HIPDetector published are read on the device instead of being uploaded again (the reference uploads per call,
    // GPUMatcher.hpp:188-196).  Default: checked -- the sweep starts on the device rows, the host folds the block it was handed while the
    // GPU works and compares with the fold taken at publish time; a block edited anywhere is uploaded and swept again, so the answer is
    // always the one for the rows passed in.  trustPublishedRegions(true) is the integrator's statement that published regions blocks
    // are never edited in place: address, count, generation and 18 sampled rows then decide (the detector must publish folds -- it
    // does by default -- for the checked mode to find its blocks).  usePublishedRegions(false): every call uploads, like the reference.
    void trustPublishedRegions(bool on)
    {
        if (ctx_) (void)clc_desc_cache_mode(ctx_, on ? CLC_DESC_CACHE_TRUST : CLC_DESC_CACHE_VERIFY);
    }
    void usePublishedRegions(bool on)
    {
        if (ctx_) (void)clc_desc_cache_mode(ctx_, on ? CLC_DESC_CACHE_VERIFY : CLC_DESC_CACHE_OFF);
    }

    void setMapData(int kpNum, void* desc)
    {
        if (check(clc_set_map(ctx_, desc, kpNum), "setMapData")) kpMap_ = kpNum;
    }

    void setTrainingImage(int kpNum, std::vector<uint64_t> const& desc)
    {
        train_.assign(desc.begin(), desc.begin() + static_cast<size_t>(8) * kpNum);
        kpTrain_ = kpNum;
    }

    void setQueryImage(int kpNum, void* desc)
    {
        const uint64_t* p = static_cast<const uint64_t*>(desc);
        query_.assign(p, p + static_cast<size_t>(8) * kpNum);
        queryRef_ = nullptr;
        kpQuery_ = kpNum;
    }

    T computeMatches(FeatureMap& regions, openMVG::matching::PairWiseMatches& putativeMatches)
    {
        const int numImages = static_cast<int>(regions.size());
        const openMVG::Pair_Set pairs = Utils::handlePairs(numImages);
        if (pairs.empty()) return EXIT_SUCCESS;
        // one upload per camera, one launch group for all pairs
        std::vector<const void*> descs(numImages, nullptr);
        std::vector<int> counts(numImages, 0);
        for (const auto& kv : regions) {
            if (static_cast<int>(kv.first) >= numImages) return EXIT_FAILURE;   // handlePairs assumes ids 0..n-1
            descs[kv.first] = kv.second->DescriptorRawData();
            counts[kv.first] = static_cast<int>(kv.second->RegionCount());
        }
        std::vector<int> flat;
        std::vector<std::vector<int32_t>> out;
        for (const auto& p : pairs) {
            flat.push_back(static_cast<int>(p.first));
            flat.push_back(static_cast<int>(p.second));
            out.emplace_back(counts[p.first]);
        }
        std::vector<int32_t*> optr;
        for (auto& o : out) optr.push_back(o.data());
        if (!check(clc_match_pairs(ctx_, descs.data(), counts.data(), numImages, flat.data(), static_cast<int>(pairs.size()), 40,
                                   optr.data()), "computeMatches"))
            return EXIT_FAILURE;
        size_t k = 0;
        for (const auto& pairIdx : pairs) {
            openMVG::matching::IndMatches pairMatches;
            const std::vector<int32_t>& m = out[k++];
            for (size_t i = 0; i < m.size(); ++i)
                if (m[i] != -1) pairMatches.emplace_back(static_cast<openMVG::IndexT>(i), static_cast<openMVG::IndexT>(m[i]));
            if (!pairMatches.empty()) putativeMatches.insert({ pairIdx, std::move(pairMatches) });
        }
        return EXIT_SUCCESS;
    }

    void matchMapFeatures(std::unique_ptr<openMVG::features::AKAZE_Binary_Regions>& map1,
                          std::unique_ptr<openMVG::features::AKAZE_Binary_Regions>& map2,
                          openMVG::matching::IndMatches& commonFeatures)
    {
        commonFeatures = computeMatches(const_cast<void*>(map1->DescriptorRawData()), const_cast<void*>(map2->DescriptorRawData()),
                                        static_cast<int>(map1->RegionCount()), static_cast<int>(map2->RegionCount()), 60);
    }

    void computeMatchesPair(const openMVG::Pair& pairIdx, FeatureMap& regions, openMVG::matching::IndMatches& putativeMatches)
    {
        putativeMatches = computeMatches(const_cast<void*>(regions[pairIdx.first]->DescriptorRawData()),
                                         const_cast<void*>(regions[pairIdx.second]->DescriptorRawData()),
                                         static_cast<int>(regions[pairIdx.first]->RegionCount()),
                                         static_cast<int>(regions[pairIdx.second]->RegionCount()));
    }

    // GPUMatcher.hpp:174-178: setQueryImage(regions[droneId]) + matchFeaturesWithMap().  The regions block itself is handed to the
    // library (no copy into a query buffer first), so that a block HIPDetector published is found on the device.
    void matchSceneWithMap(int& droneId, colocData& data, openMVG::matching::IndMatches& mapMatches)
    {
        // (the query set by this call IS the regions block -- not a copy of it: a later computeMatchesPreset() / matchFeaturesWithMap()
        // reads it there, so it must still exist then; in the reference's flow regions[droneId] lives until the drone's next frame)
        kpQuery_ = static_cast<unsigned int>(data.regions[droneId]->RegionCount());
        queryRef_ = data.regions[droneId]->DescriptorRawData();
        mapMatches = matchWithMap(queryRef_, static_cast<int>(kpQuery_));
    }

    // The landmarks of the map's descriptor rows, in mapRegionIdx order, into the MATCHER's context (clc_set_map_points), as
    // HIPLocalizer::setMapPoints puts them into the localizer's: call it beside setMapData.  Only matchSceneWithMapGuidedDev reads them.
    // false = success.
    bool setMapPoints(colocData& data)
    {
        std::vector<double> X(3 * data.mapRegionIdx.size());
        for (size_t i = 0; i < data.mapRegionIdx.size(); ++i) {
            const auto& P = data.scene.GetLandmarks().at(data.mapRegionIdx[i]).X;
            for (int r = 0; r < 3; ++r) X[3 * i + r] = P[r];
        }
        return !check(clc_set_map_points(ctx_, X.data(), static_cast<int>(data.mapRegionIdx.size())), "setMapPoints");
    }

    // matchSceneWithMap around a PREDICTED pose (clc_match_map_guided_dev, which states the rule; no counterpart in the reference): a
    // keypoint is matched only against the map rows whose landmark projects within `radius` pixels of it under predictedPose -- the last
    // pose, or the filter's statePre -- with the threshold of MatcherOptions.  Everything stays on the device: d_desc / d_kps / d_count are
    // the detector's blocks for this frame (nq planned rows), d_match_out[nq] is what clc_match_map_dev would leave (a map row or -1) and
    // feeds HIPLocalizer::localizeImageDev unchanged.  Enqueue only, on `after_stream` -- the stream that produced the descriptors and
    // keypoints (nullptr: the context's own).  Too few tracks is the caller's cue to fall back on the unguided match.  false = enqueued.
    bool matchSceneWithMapGuidedDev(const openMVG::geometry::Pose3& predictedPose, const clc_camera_k3& intrinsics, const void* d_desc, int nq,
                                    const clc_keypoint* d_kps, const uint32_t* d_count, float radius, int32_t* d_match_out, void* after_stream)
    {
        clc_map_guided_job jb{};
        jb.d_q = d_desc; jb.nq = nq; jb.d_count = d_count; jb.d_kps = d_kps;
        jb.cam = intrinsics;
        const openMVG::Vec3 t = predictedPose.translation();                     // t = -R C
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) jb.Rt[4 * i + j] = predictedPose.rotation()(i, j); jb.Rt[4 * i + 3] = t[i]; }
        jb.radius = radius; jb.threshold = matchThreshold_;
        jb.d_match = d_match_out;
        return !check(clc_match_map_guided_dev(ctx_, &jb, after_stream), "matchSceneWithMapGuidedDev");
    }

    // matchSceneWithMapGuidedDev through a cell grid of the projections (clc_match_map_binned_dev): the same arguments, the same d_match
    // bit for bit, without the whole-map sweep -- a keypoint meets only the map rows binned into the at most 3 x 3 cells around it.  Jobs
    // the grid does not suit (clc_map_binned_plan: SWEEP) run the guided path inside the entry.  false = enqueued.
    bool matchSceneWithMapBinnedDev(const openMVG::geometry::Pose3& predictedPose, const clc_camera_k3& intrinsics, const void* d_desc, int nq,
                                    const clc_keypoint* d_kps, const uint32_t* d_count, float radius, int32_t* d_match_out, void* after_stream)
    {
        clc_map_guided_job jb{};
        jb.d_q = d_desc; jb.nq = nq; jb.d_count = d_count; jb.d_kps = d_kps;
        jb.cam = intrinsics;
        const openMVG::Vec3 t = predictedPose.translation();                     // t = -R C
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) jb.Rt[4 * i + j] = predictedPose.rotation()(i, j); jb.Rt[4 * i + 3] = t[i]; }
        jb.radius = radius; jb.threshold = matchThreshold_;
        jb.d_match = d_match_out;
        return !check(clc_match_map_binned_dev(ctx_, &jb, after_stream), "matchSceneWithMapBinnedDev");
    }

    // matchSceneWithMapBinnedDev and then the one-to-one filter (clc_match_map_binned_unique_dev, which states the rule; no counterpart in
    // the reference): of the keypoints that took one landmark only the nearest keeps it, so the solve behind sees every landmark once.
    // d_owner_out: nullable, one int32 per map row -- the keypoint that holds the landmark, or -1.  false = enqueued.
    bool matchSceneWithMapBinnedUniqueDev(const openMVG::geometry::Pose3& predictedPose, const clc_camera_k3& intrinsics, const void* d_desc, int nq,
                                          const clc_keypoint* d_kps, const uint32_t* d_count, float radius, int32_t* d_match_out, void* after_stream,
                                          int32_t* d_owner_out)
    {
        clc_map_guided_job jb{};
        jb.d_q = d_desc; jb.nq = nq; jb.d_count = d_count; jb.d_kps = d_kps;
        jb.cam = intrinsics;
        const openMVG::Vec3 t = predictedPose.translation();                     // t = -R C
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) jb.Rt[4 * i + j] = predictedPose.rotation()(i, j); jb.Rt[4 * i + 3] = t[i]; }
        jb.radius = radius; jb.threshold = matchThreshold_;
        jb.d_match = d_match_out;
        return !check(clc_match_map_binned_unique_dev(ctx_, &jb, d_owner_out, after_stream), "matchSceneWithMapBinnedUniqueDev");
    }

    // The map extended in place from two posed views (clc_map_extend_dev, which states the rule; no counterpart in the reference): the
    // untracked guided matches of views pair.first (A, the query side) and pair.second (B) are triangulated and appended behind the map
    // of this matcher's context (setMapData + setMapPoints, or an earlier extension).  The views arrive as their device blocks -- the
    // descriptor rows, a side each (positions, the count word, the view's map match d_track, nullable) -- and their two poses; the
    // threshold is MatcherOptions'.  On success colocData receives what setupMapDatabase (colocData.hpp:89-121) would hold for the new
    // landmarks, in the entry's row order: mapRegions gains A's feature and descriptor of every appended row (from data.regions[A], the
    // host copy of the block), mapRegionIdx a fresh landmark id each -- one past the largest key of the scene, ascending --, the scene
    // the landmarks.  n_added / n_dropped (nullable): the entry's counts.  false = success, as the reference's members return it.
    struct ExtendSideDev { const clc_keypoint* d_kps; const float* d_feat; int feat_stride; const uint32_t* d_count; int32_t* d_track; };
    bool extendMapPairDev(colocData& data, openMVG::Pair pair, const void* d_desc_a, int na, const void* d_desc_b, int nb, const ExtendSideDev& a,
                          const ExtendSideDev& b, const clc_camera_k3& cam_a, const clc_camera_k3& cam_b, const openMVG::geometry::Pose3& pose_a,
                          const openMVG::geometry::Pose3& pose_b, float band, int max_distance, void* after_stream, int* n_added = nullptr,
                          int* n_dropped = nullptr)
    {
        if (n_added) *n_added = 0;
        if (n_dropped) *n_dropped = 0;
        const auto ra = data.regions.find(pair.first);
        if (ra == data.regions.end() || !ra->second || static_cast<int>(ra->second->RegionCount()) < na) {
            std::cerr << "HIPMatcher::extendMapPairDev: data.regions holds no host copy of view A's rows" << std::endl;
            return true;
        }
        clc_map_extend jb{};
        const auto side = [](clc_extend_view& v, const void* d_desc, int n, const ExtendSideDev& s, const clc_camera_k3& cam,
                             const openMVG::geometry::Pose3& pose) {
            v.d_desc = d_desc; v.n = n; v.d_count = s.d_count; v.d_kps = s.d_kps; v.d_feat = s.d_feat; v.feat_stride = s.feat_stride;
            v.cam = cam; v.d_track = s.d_track;
            const openMVG::Vec3 t = pose.translation();                            // t = -R C
            for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) v.Rt[4 * i + j] = pose.rotation()(i, j); v.Rt[4 * i + 3] = t[i]; }
        };
        side(jb.a, d_desc_a, na, a, cam_a, pose_a);
        side(jb.b, d_desc_b, nb, b, cam_b, pose_b);
        jb.band = band; jb.threshold = matchThreshold_; jb.max_distance = max_distance; jb.update_tracks = 1; jb.after_stream = after_stream;
        std::vector<int32_t> q(na > 0 ? na : 0), t(na > 0 ? na : 0);
        std::vector<double> X(3 * static_cast<size_t>(na > 0 ? na : 0));
        jb.new_q = q.data(); jb.new_t = t.data(); jb.X = X.data();
        if (!check(clc_map_extend_dev(ctx_, &jb), "extendMapPairDev")) return true;
        if (!data.mapRegions) data.mapRegions.reset(new openMVG::features::AKAZE_Binary_Regions());
        openMVG::IndexT id = data.scene.structure.empty() ? 0 : data.scene.structure.rbegin()->first + 1;
        for (int k = 0; k < jb.n_added; ++k, ++id) {
            data.mapRegions->Features().push_back(ra->second->Features()[q[k]]);
            data.mapRegions->Descriptors().push_back(ra->second->Descriptors()[q[k]]);
            data.mapRegionIdx.push_back(id);
            data.scene.structure[id].X = openMVG::Vec3(X[3 * k], X[3 * k + 1], X[3 * k + 2]);
        }
        kpMap_ += static_cast<unsigned int>(jb.n_added);
        if (n_added) *n_added = jb.n_added;
        if (n_dropped) *n_dropped = jb.n_dropped;
        return false;
    }

    // A tracked frame folded into the map rows' observation statistics (clc_map_observe_dev, which states the rule; no counterpart in the
    // reference): which landmarks the frame's pose should see inside the width x height image less `margin`, and which of them the
    // frame's map match d_track (matchSceneWithMapBinnedUniqueDev's d_match_out) found within `gate` pixels of their projection.  Enqueue
    // only, on the context's stream behind `after_stream`: NO host wait -- call it behind every tracked frame.  false = enqueued.
    bool observeMapDev(const openMVG::geometry::Pose3& pose, const clc_camera_k3& intrinsics, int nq, const clc_keypoint* d_kps, const float* d_feat,
                       int feat_stride, const uint32_t* d_count, const int32_t* d_track, int width, int height, float gate, float margin,
                       void* after_stream)
    {
        clc_map_observe jb{};
        jb.view.n = nq; jb.view.d_count = d_count; jb.view.d_kps = d_kps; jb.view.d_feat = d_feat; jb.view.feat_stride = feat_stride;
        jb.view.cam = intrinsics; jb.view.d_track = d_track;
        const openMVG::Vec3 t = pose.translation();                              // t = -R C
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) jb.view.Rt[4 * i + j] = pose.rotation()(i, j); jb.view.Rt[4 * i + 3] = t[i]; }
        jb.width = width; jb.height = height; jb.gate = gate; jb.margin = margin; jb.after_stream = after_stream;
        return !check(clc_map_observe_dev(ctx_, &jb), "observeMapDev");
    }

    // The map culled in place (clc_map_cull_dev, which states the rule; no counterpart in the reference): rows dropped by their
    // observation statistics under `rule` -- and by the caller's own d_flagged bytes, nullable --, the map of this matcher's context
    // compacted in order, the device lists that name map rows (the frames' d_track lists) remapped in place.  On success colocData holds
    // what setupMapDatabase (colocData.hpp:89-121) would hold for the SURVIVING landmarks: the rows of mapRegions and mapRegionIdx compacted
    // in order, the dropped landmarks erased from the scene -- the mirror of what extendMapPairDev does for new ones.  removed (nullable):
    // the rows dropped; remap (nullable): old row -> new row or -1, for HIPLocalizer::cullMapPoints and whatever else names rows.
    // The default rule is the customary one (a quarter of the frames that should see a point) and is UNTUNED.  false = success.
    struct CullRule { int min_visible = 8, num = 1, den = 4; uint32_t max_idle = 0; const uint8_t* d_flagged = nullptr; };
    struct CullListDev { int32_t* d_track; int n; };
    bool cullMapDev(colocData& data, const CullRule& rule, const std::vector<CullListDev>& lists, void* after_stream, int* removed = nullptr,
                    std::vector<int32_t>* remap = nullptr)
    {
        if (removed) *removed = 0;
        if (remap) remap->clear();
        const size_t rows = data.mapRegionIdx.size();
        if (rows != kpMap_ || lists.size() > CLC_MAX_BATCH || (rows > 0 && (!data.mapRegions || data.mapRegions->RegionCount() != rows))) {
            std::cerr << "HIPMatcher::cullMapDev: colocData's map database is not the context's map, or more than CLC_MAX_BATCH lists" << std::endl;
            return true;
        }
        clc_map_cull jb{};
        jb.min_visible = rule.min_visible; jb.num = rule.num; jb.den = rule.den; jb.max_idle = rule.max_idle; jb.d_flagged = rule.d_flagged;
        jb.n_lists = static_cast<int>(lists.size());
        for (size_t l = 0; l < lists.size(); ++l) { jb.d_track[l] = lists[l].d_track; jb.track_n[l] = lists[l].n; }
        jb.after_stream = after_stream;
        std::vector<int32_t> map(rows);
        jb.h_remap = map.data();
        if (!check(clc_map_cull_dev(ctx_, &jb), "cullMapDev")) return true;
        size_t k = 0;
        for (size_t r = 0; r < rows; ++r) {
            if (map[r] < 0) { data.scene.structure.erase(data.mapRegionIdx[r]); continue; }
            if (k != r) {
                data.mapRegions->Features()[k] = data.mapRegions->Features()[r];
                data.mapRegions->Descriptors()[k] = data.mapRegions->Descriptors()[r];
                data.mapRegionIdx[k] = data.mapRegionIdx[r];
            }
            ++k;
        }
        if (data.mapRegions) { data.mapRegions->Features().resize(k); data.mapRegions->Descriptors().resize(k); }
        data.mapRegionIdx.resize(k);
        kpMap_ = static_cast<unsigned int>(jb.n_kept);
        if (removed) *removed = jb.n_dropped;
        if (remap) *remap = map;
        return false;
    }

    // computeMatchesPair with the one-to-one filter behind the sweep (clc_match_2nn_unique): the same IndMatch(i_ = query idx in
    // regions[first], j_ = train idx in regions[second]) list, thr 40, in which no train index appears twice -- of the queries that named
    // one train row the nearest keeps it, the lowest query index among equals.
    void computeMatchesPairUnique(const openMVG::Pair& pairIdx, FeatureMap& regions, openMVG::matching::IndMatches& putativeMatches)
    {
        const int numKPQuery = static_cast<int>(regions[pairIdx.first]->RegionCount());
        const int numKPTraining = static_cast<int>(regions[pairIdx.second]->RegionCount());
        std::vector<int32_t> m(numKPQuery > 0 ? numKPQuery : 0);
        putativeMatches.clear();
        if (!check(clc_match_2nn_unique(ctx_, regions[pairIdx.first]->DescriptorRawData(), numKPQuery, regions[pairIdx.second]->DescriptorRawData(),
                                        numKPTraining, 40, m.data(), nullptr), "computeMatchesPairUnique"))
            return;
        for (size_t i = 0; i < m.size(); ++i)
            if (m[i] != -1) putativeMatches.emplace_back(static_cast<openMVG::IndexT>(i), static_cast<openMVG::IndexT>(m[i]));
    }

    // GPUMatcher.hpp:180-226: IndMatch(i_ = query index, j_ = train index); dmatches(train, query, 0)
    openMVG::matching::IndMatches computeMatches(void* h_descriptorsQuery, void* h_descriptorsTraining, int numKPQuery,
                                                 int numKPTraining, uint8_t threshold = 40)
    {
        openMVG::matching::IndMatches matches;
        std::vector<int32_t> m(numKPQuery > 0 ? numKPQuery : 0);
        dmatches.clear();
        if (!check(clc_match_2nn(ctx_, h_descriptorsQuery, numKPQuery, h_descriptorsTraining, numKPTraining, threshold, m.data(),
                                 nullptr, nullptr), "computeMatches"))
            return matches;
        for (size_t i = 0; i < m.size(); ++i) {
            if (m[i] != -1) {
                matches.emplace_back(static_cast<openMVG::IndexT>(i), static_cast<openMVG::IndexT>(m[i]));
                dmatches.emplace_back(m[i], static_cast<int>(i), 0.0f);
            }
        }
        return matches;
    }

    // GPUMatcher.hpp:229-250: preset train/query images; IndMatch(i_ = train index, j_ = query index)
    openMVG::matching::IndMatches computeMatchesPreset()
    {
        openMVG::matching::IndMatches matches;
        std::vector<int32_t> m(kpQuery_);
        dmatches.clear();
        if (!check(clc_match_2nn(ctx_, queryData(), static_cast<int>(kpQuery_), train_.data(), static_cast<int>(kpTrain_),
                                 matchThreshold_, m.data(), nullptr, nullptr), "computeMatchesPreset"))
            return matches;
        for (size_t i = 0; i < m.size(); ++i) {
            if (m[i] != -1) {
                matches.emplace_back(static_cast<openMVG::IndexT>(m[i]), static_cast<openMVG::IndexT>(i));
                dmatches.emplace_back(m[i], static_cast<int>(i), 0.0f);
            }
        }
        return matches;
    }

    // GPUMatcher.hpp:252-271: IndMatch(i_ = MAP index, j_ = query index)
    openMVG::matching::IndMatches matchFeaturesWithMap() { return matchWithMap(queryData(), static_cast<int>(kpQuery_)); }

    const char* lastError() const { return ctx_ ? clc_last_error_string(ctx_) : "no context"; }
    // the context behind this matcher, for the entries of the C ABI that have no member here (clc_map_stats_get, clc_track_build_dev)
    clc_ctx* context() const { return ctx_; }

private:
    const void* queryData() const { return queryRef_ ? queryRef_ : static_cast<const void*>(query_.data()); }

    openMVG::matching::IndMatches matchWithMap(const void* desc, int n)
    {
        openMVG::matching::IndMatches matches;
        std::vector<int32_t> m(n > 0 ? n : 0);
        if (!check(clc_match_map(ctx_, desc, n, matchThreshold_, m.data()), "matchFeaturesWithMap")) return matches;
        for (size_t i = 0; i < m.size(); ++i)
            if (m[i] != -1) matches.emplace_back(static_cast<openMVG::IndexT>(m[i]), static_cast<openMVG::IndexT>(i));
        return matches;
    }

    bool check(int rc, const char* what)
    {
        if (rc == CLC_OK) return true;
        std::cerr << "HIPMatcher::" << what << ": " << clc_status_string(rc) << ": " << lastError() << std::endl;
        return false;
    }

    clc_ctx* ctx_ = nullptr;
    uint8_t matchThreshold_;
    unsigned int kpTrain_ = 0, kpQuery_ = 0, kpMap_ = 0;
    std::vector<uint64_t> train_, query_;
    const void* queryRef_ = nullptr;     // the query set by matchSceneWithMap: the regions block itself
};

} // namespace coloc

// clc_ctx.h -- the context behind the C ABI and the helpers the capi_*.hip translation units share (not installed).
#ifndef CLC_CTX_H
#define CLC_CTX_H

#include "clc_buf.h"
#include "clc_internal.h"
#include "clc_layout.h"

#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace clc {
// Event pairs recorded around kernel launches; drained (with a stream sync) by clc_profile_read.
struct Profiler {
    bool on = false;
    unsigned mask = 0xFFFFFFFFu;   // which kernels are bracketed
    struct Pair { hipEvent_t a = nullptr, b = nullptr; int kernel = 0; hipStream_t stream = nullptr; bool open = false; };
    std::vector<Pair> pending;
    std::vector<hipEvent_t> pool;
    double total_ms[CLC_KERNEL_COUNT] = {};
    int launches[CLC_KERNEL_COUNT] = {};
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        // timing events need no system-scope release: a default event makes the GPU write its L2 back at every record, inside
        // the region being timed (the host never reads device data through these events, only their timestamps)
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) (void)hipEventCreate(&e);
        return e;
    }
    void drain()
    {
        for (Pair& p : pending) {
            if (!p.a || !p.b || p.open) continue;
            (void)hipEventSynchronize(p.b);
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { total_ms[p.kernel] += ms; launches[p.kernel] += 1; }
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
    ~Profiler()
    {
        for (Pair& p : pending) { if (p.a) (void)hipEventDestroy(p.a); if (p.b) (void)hipEventDestroy(p.b); }
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
};

struct DescEntry;
// rows_at: STAGED = the frame of the last clc_detect_and_describe* call (pinned block / desc_pending, staged_n rows); OWN = the
// context's own d_desc (own_rows); NONE = the last describing call wrote a caller buffer or failed, or nothing was described yet
enum { ROWS_NONE = 0, ROWS_STAGED = 1, ROWS_OWN = 2 };

// A context's block of gathered correspondences, device and pinned, for `cap` of them (ensure_gather; its arrays: GatherView, clc_layout.h)
struct GatherBlock { DevBuf d; PinBuf h; size_t cap = 0; };
} // namespace clc

struct clc_ctx {
    int device = 0;
    std::vector<float> acr_lg;   // (float) log10(k), k = 0 .. : the a-contrario tables are sums over it
    hipStream_t stream = nullptr;
    std::string err;
    bool has_det = false, has_mat = false;
    clc_detector_opts dopts{};
    clc_matcher_opts mopts{};
    // pyramid
    clc::PyramidDesc pd{};
    clc::DevBuf d_arena;         // (bytes)
    size_t arena_bytes = 0;      // one pyramid
    int arena_slots = 1;         // pyramids the arena holds (grown by clc_describe_batch_dev)
    bool pyramid_valid = false;
    // detect + describe
    clc::DevBuf d_kps;               // clc_keypoint
    clc::DevBuf d_desc;              // uint64_t
    clc::DevBuf d_score;             // arena-shaped FAST score maps (one per pyramid slot; only keypoint pixels are written and read)
    clc::DevBuf d_kpmask;            // uint64_t [slot][tile][16] keypoint bits of a tile row (detect.hip)
    clc::DevBuf d_tcount;            // uint32_t [slot][tile] keypoints of a tile
    clc::DevBuf d_count;             // uint32_t {written, found} of the context's own keypoint list
    uint32_t n_tiles = 0;
    int selection = CLC_SELECT_FIRST;   // which keypoints a frame with more than maxkp keeps (clc_detect_set_selection)
    clc::DevBuf d_select;            // uint32_t [CLC_MAX_BATCH][detect_select_words] score histograms, cutoffs, band counts of CLC_SELECT_STRONGEST
    bool select_dirty = false;       // a selecting detect call failed between its launches: the histograms may not be zero
    bool detected = false;
    // match
    clc::DevBuf d_q, d_t, d_m;       // descriptor rows (bytes)
    int map_n = -1;
    clc::DevBuf d_match;             // int32_t
    clc::DevBuf d_best, d_second;    // uint16_t
    clc::DevBuf d_partial;           // uint2: the armed top-2 rows + arrival counters of the K2NN sweeps
    bool partial_dirty = false;      // armed (all-ones) state of the atomic top-2 rows was lost
    clc::DevBuf d_guided;            // float: the lines (3 per query row) and train points (2 per train row) of a guided match, or the query
                                     // points (2) and the landmarks' projections (2 per map row) of a map match around a pose (GuidedDev)
    clc::DevBuf d_binned;            // the binned map match's query points, projections, cell table and records (BinnedDev)
    clc::DevBuf d_unique;            // the one-to-one filter's claim words, and a composed entry's distances / inverse list (UniqueDev)
    clc::DevBuf d_extend;            // the map extension's running row count and per-job lists, flags and points (ExtendDev / ExtendJobDev)
    clc::PinBuf h_extend;            // its records and mirrors (ExtendJobPin)
    // the map rows' observation statistics and the cull (map_cull.hip): visible | found | last_view of every row (CullStat, room for
    // MatcherOptions.maxkp rows, allocated on first use) in d_stat; d_stat_next changes places with it when a cull installs, as d_m_next and
    // d_map_X_next do.  stat_rows: the rows the counters cover (whatever replaces the map's rows: 0, map_rows_replaced below); epoch: the
    // observe calls since then; obs_serial: the observe calls of the context's life, the stamp of a hit (never 0, never reset)
    clc::DevBuf d_stat, d_stat_next;
    clc::DevBuf d_obs;               // a call's hit stamps, one word per (view, row) (ObserveDev)
    clc::DevBuf d_cull;              // the cull's remap and record (CullDev)
    clc::PinBuf h_cull;              // its polled word, counts and remap mirror (CullPin)
    int stat_rows = 0;
    uint32_t epoch = 0, obs_serial = 0;
    int formulation = clc::K2NN_MATRIX;   // K2NN sweep formulation (k2nn.hip): FP4 matrix pipe, or round 1's popcount kernel for A/B runs
    int target_blocks = 0;           // K2NN sweep workgroups aimed at per launch; 0 = the formulation's default
    int bias_a = 326, bias_b = 249;  // matrix sweep, one-round single-job plans: train share of a workgroup on wave slot 0 / 1 in 1/256 of the
                                     // equal share (k2nn.hip; measured optimum 21 : 16 : 12-13 tiles at 10k x 10k); CLC_K2NN_BIAS=a,b, 0,0 = equal shares
    bool xcd_map = true;         // XCD-aware K2NN tile order (CLC_K2NN_XCD_MAP=0 switches it off for A/B runs)
    clc::K2nnDevice k2dev{};          // XCDs and CUs of this context's device (the sweep planner's balance arguments)
    int bias_source = 0;         // 0: built-in default, 1: CLC_K2NN_BIAS, 2: timed probe on this device (k2nn_probe_bias)
    float bias_probe_us[4] = {}; // the probe's sweep times per candidate (0: not probed)
    clc::Event ev_group;             // acr_drive (pose_batch.hip): orders a shared group's stream and the contexts' own streams
    int cache_mode = CLC_DESC_CACHE_VERIFY;   // how this context's host-pointer match entry points treat published blocks (clc_desc_cache_mode)
    // pnp
    clc::DevBuf d_pairs;          // clc_match_pairs arena (bytes): descriptors of all cameras, then results
    clc::DevBuf d_pnp;            // double
    clc::PinBuf h_pin;            // pinned staging for the pose solve
    // 2D-3D tracks and two-view correspondences (gather.hip)
    clc::DevBuf d_map_X;          // clc_set_map_points: the landmark of map descriptor row i, 3 doubles each
    int map_X_n = -1;             // (-1: none set)
    clc::GatherBlock trk, pair;   // the tracks (clc_track_localize*_dev) / the pairs (clc_pair_filter*_dev) of this context's job
    clc::Event ev_track;             // orders the track / pair launch behind job.after_stream, and the contexts' streams behind the launch
    // the inter-camera step from device memory (inter_dev.hip; InterDev / InterPin, clc_layout.h)
    clc::DevBuf d_inter;
    clc::PinBuf h_inter;
    // the map built on the device (map_build.hip; MapStageDev / MapStagePin); the next map's points, which change places with d_map_X
    // when a build succeeds
    clc::DevBuf d_mapb, d_map_X_next;
    clc::PinBuf h_mapb;
    // the map replaced at the old map's scale (map_update.hip): the NEXT map's descriptor rows, allocated on first use at d_m's size --
    // the sweep clamps its train reads to the last row (k2nn.hip), so nothing past the rows gathered is read and nothing is zeroed --
    // which change places with d_m on install; the match and the common lists and their pinned mirror (AlignDev / AlignPin)
    clc::DevBuf d_m_next, d_align;
    clc::PinBuf h_align;
    // the map grown past the seed pair (map_grow.hip; GrowDev / GrowPin); the per-track state of the last grown build, for
    // clc_map_resect_build_dev -- the table lies in d_mapb, so whatever rewrites that block (a tracks / map build) ends it (grow_table = null)
    clc::DevBuf d_growb;
    clc::PinBuf h_growb;
    const int32_t* grow_table = nullptr; const int32_t* grow_n_tracks = nullptr;
    int grow_n_cams = 0, grow_cap = 0;
    // the bundle adjustment (map_ba.hip; BaDev / BaPin)
    clc::DevBuf d_bab;
    clc::PinBuf h_bab;
    // host front end (clc_detect_and_describe*): ONE pinned block [ image | keypoints | descriptors | {written, found} ] the frame goes
    // in and out through, and the block of the descriptor table (desc_cache.h) the frame's descriptors are written into on the device
    clc::PinBuf h_stage;          // (bytes)
    size_t stage_img = 0, stage_kps = 0, stage_desc = 0, stage_cnt = 0;      // byte offsets inside h_stage
    clc::DescEntry* desc_pending = nullptr;
    int staged_n = -1;            // rows of the last staged frame (-1: none)
    // where the rows of this context's last describing call lie: what clc_desc_cache_publish(d_src = NULL) publishes
    int rows_at = clc::ROWS_NONE;
    int own_rows = 0;             // ROWS_OWN: rows described into d_desc (-1: the detector's {written} counter tells)
    // host-pointer match entries: pinned mirror of the results (so that the host can verify published blocks while the GPU sweeps)
    clc::PinBuf h_res;            // (bytes)
    clc::Profiler prof;
};

namespace clc {

// records the failure text on the context (clc_last_error_string) and returns `code`
int fail(clc_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess);

// The pose entry points (P3P, a-contrario pose, refinement) read K as { fx, skew, cx; 0, fy, cy; 0, 0, 1 }: the minimal solver and the
// refinement use K[0], K[1], K[2], K[4], K[5] only, while the residual kernels apply all nine entries.  A K that is anything else (a
// scaled K, K[3] != 0) would give the two halves of one solve different cameras, so it is refused (include/coloc_hip.h, clc_pnp_refine).
inline bool pose_K_ok(const double* K) { return K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0; }

#define CLC_HIP(ctx, call)                                                      \
    do {                                                                        \
        hipError_t e__ = (call);                                                \
        if (e__ != hipSuccess) return ::clc::fail((ctx), CLC_ERR_HIP, #call, e__);     \
    } while (0)

inline hipStream_t pick(clc_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream; }

// the map's rows were replaced (clc_set_map, an install of map_build.hip / map_update.hip, an empty map): row identities are new, so the
// observation statistics cover nothing and the epochs start again (map_cull.hip)
inline void map_rows_replaced(clc_ctx* ctx) { ctx->stat_rows = 0; ctx->epoch = 0; }

// THE way a context's workspace grows: a buffer that holds `need` bytes stays; any other is freed and allocated anew with
// need + need * num / den bytes -- behind a synchronisation of the context's stream where work in flight may still use the old block
// (sync_first).  The contents do not survive.  `what` names the workspace in a failure's text; *fresh: a call that succeeds made a new block.
template <class B> inline int grow(clc_ctx* ctx, B& b, size_t need, size_t num, size_t den, bool sync_first, const char* what, bool* fresh = nullptr)
{
    if (fresh) *fresh = need > b.bytes;
    if (need <= b.bytes) return CLC_OK;
    if (sync_first) CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const hipError_t e = b.grow(need, num, den);
    return e == hipSuccess ? CLC_OK : fail(ctx, CLC_ERR_HIP, what, e);
}

// THE way a block gets its arrays (clc_layout.h).  lay(Carve&): the block's layout -- a view's carve() with the block's dimensions.  It
// is run on a measuring cursor, the block grown to what that took (grow's arguments as they are), then run on the block.  place_block:
// the second half alone, for a consumer that places a view on a block an earlier call laid out; a view that runs past its block is
// refused (CLC_ERR_STATE, `what`) instead of being handed to a kernel.
template <class B, class F> inline int place_block(clc_ctx* ctx, const B& b, const char* what, F&& lay)
{
    Carve c(b.ptr);
    lay(c);
    return c.bytes() <= b.bytes ? CLC_OK : fail(ctx, CLC_ERR_STATE, what);
}
template <class B, class F> inline int carve_block(clc_ctx* ctx, B& b, size_t num, size_t den, bool sync_first, const char* what, F&& lay)
{
    Carve measure;
    lay(measure);
    const int rc = grow(ctx, b, measure.bytes(), num, den, sync_first, what);
    return rc == CLC_OK ? place_block(ctx, b, what, lay) : rc;
}

// context-owned workspaces, grown on demand (capi_core.hip)
int ensure_partial(clc_ctx* ctx, size_t elems);           // armed K2NN top-2 rows + arrival counters
int ensure_slots(clc_ctx* ctx, int n, hipStream_t st);    // pyramids (+ detector maps) of n cameras
// the pose scratch and the pinned staging of the pose solves -- ONE pinned buffer, one transfer in, one out --, both half as much again:
// a stream of solves whose sizes creep upwards (map matches per frame) must not reallocate at every new maximum, and a pinned
// allocation costs a millisecond; the pinned mirror of match results
template <class F> inline int ensure_pnp(clc_ctx* ctx, F&& lay) { return carve_block(ctx, ctx->d_pnp, 1, 2, true, "growing d_pnp", lay); }
template <class F> inline int ensure_pinned(clc_ctx* ctx, F&& lay) { return carve_block(ctx, ctx->h_pin, 1, 2, true, "growing h_pin", lay); }
template <class F> inline int ensure_results(clc_ctx* ctx, F&& lay) { return carve_block(ctx, ctx->h_res, 0, 1, true, "growing h_res", lay); }
int ensure_gather(clc_ctx* ctx, GatherBlock& g, size_t cap, const GatherLayout& lay);      // a gather block (gather.hip)

// one 2-D side -- exactly one of kps / feat, the stride, the alignment, the focal length -- validated ONCE for whoever takes one, into
// the kernels' view of it (gather.hip).  who: the entry point, for the failure's text (CLC_ERR_BAD_ARG)
int gather_side(clc_ctx* ctx, const char* who, const uint32_t* count, const clc_keypoint* kps, const float* feat, int stride, const clc_camera_k3& cam,
                GatherSide& out);
// the pyramid levels' scales as clc_keypoints_to_features has them (GPUDetector.hpp:173): pow(float, integer) evaluated in double, rounded
// to float -- on the host, once per launch record
inline void level_scales(float out[CLC_MAX_LEVELS])
{
    for (int l = 0; l < CLC_MAX_LEVELS; ++l) out[l] = (float)std::pow((double)1.2f, (double)l);
}

// a describing call begins: the rows of the last one no longer stand (staged_n = -1, desc_pending abandoned, rows_at = NONE)
// (desc_cache.hip)
void rows_leave(clc_ctx* ctx);

// K2NN: plan + launch a job list on `st` with the context's formulation / shares (capi_match.hip)
int default_target_blocks(int formulation, const K2nnDevice& dev = K2nnDevice{});
int run_jobs(clc_ctx* ctx, std::vector<K2nnJobDev>& jobs, hipStream_t st, bool probe = false);
void k2nn_probe_bias(clc_ctx* ctx);                       // once per process and device: which unequal shares suit this device

// ---- the one-to-one filter (k2nn_unique.hip) ---------------------------------------------------------------------------------------------
// What the entries that compose a producer with the filter share.  unique_check: the filter's own rules for the n_jobs jobs -- CLC_ERR_BAD_ARG,
// CLC_ERR_STATE, CLC_ERR_CAPACITY on `who` --, with nothing allocated or enqueued (need_best: false where the distances will come from
// the context's scratch).  unique_scratch: ONE pair's claim words in d_unique, and where asked the distances a producer writes and an
// inverse list for a download.  unique_enqueue: arm, claim, resolve on `st` for jobs whose claim words are dv[j].claim.
int unique_check(clc_ctx* ctx, const char* who, const clc_unique_job* jobs, int n_jobs, bool need_best);
int unique_scratch(clc_ctx* ctx, int nq, int nt, bool with_best, bool with_owner, UniqueDev& dv);
int unique_enqueue(clc_ctx* ctx, const clc_unique_job* jobs, const UniqueDev* dv, int n_jobs, hipStream_t st);

// all two-view a-contrario filters of a batch (pose_batch.hip); jobs[i] on ctxs[i]
int acr_two_view_batch(clc_ctx* const* ctxs, clc_two_view_job* const* jobs, int n_jobs, int kind /* kAcrEssential, kAcrFundamental or kAcrHomography */);
int check_batch_contexts(clc_ctx* const* ctxs, int n_jobs, const char* what);
// clc_sim3_acransac on N 3-D / 3-D pairs that lie in DEVICE memory (d_x_new | d_x_old, 3 N each; read in place, they must stand until the
// call returns) with the box { min, max } of d_x_old from whoever gathered them (pose_batch.hip).  out: identity where there is no model
int sim3_solve_dev(clc_ctx* ctx, const double* d_x_new, const double* d_x_old, int N, const double* box, int max_iteration, uint64_t seed,
                   double precision, Sim3Out* out, uint8_t* h_mask, int* n_inliers, double* error_max, double* min_nfa, int* iterations);
// clc_pair_filter_batch_dev under model 'E' (pose_batch.hip), which also says where each job's inlier list lies for the DEVICE:
// inliers[i] = the list in job i's context's pinned block, in the filter's order, written by the round that completed the run before
// its word (null: the job's solve did not start); it stands until the context's next solve
int pair_filter_essential(clc_ctx* const* ctxs, clc_pair_job* jobs, int n_jobs, const int32_t** inliers);
// rows idx[0 .. n) of a descriptor block (64 B each) -> dst, the index list on the device (null: rows 0 .. n) (gather.hip)
hipError_t launch_gather_rows(const uint4* src, const int32_t* d_idx, uint4* dst, uint32_t n, hipStream_t stream);
// The map-to-map sweep of the reference's chain (coloc.hpp:317-323; inter_pose.hip), enqueued on `stream`: rows d_idx[0 .. nf) of
// d_first_desc -> d_rows (the temporary map's descriptors), then K2NN with Q = the global map's map_n rows, T = d_rows, threshold <= 0:
// 60 (GPUMatcher.hpp:162): d_match[q] = temporary map point matched by global map point q, or -1
int map_sweep_enqueue(clc_ctx* ctx, const void* d_first_desc, const int32_t* d_idx, int nf, const void* d_map_desc, int map_n, uint4* d_rows,
                      int32_t* d_match, int threshold, hipStream_t stream);
// its sweep alone, over nf rows already in d_rows
int map_sweep_rows_enqueue(clc_ctx* ctx, int nf, const void* d_map_desc, int map_n, const uint4* d_rows, int32_t* d_match, int threshold,
                           hipStream_t stream);

// A map build's two halves (map_build.hip).  map_stage: tracks, the seed launch, the wait for the row count, the capacity check, the host
// outputs -- the new map's points in d_map_X_next, its rows of the lower seed camera's block in the map block, the context's map as it
// was.  map_install: the rows gathered into d_m, the points swapped in (clc_map_build_dev, clc_map_init_batch_dev).
// d_cam: the per-row camera list of a GROWN stage (row i's descriptor = row d_row[i] of camera d_cam[i]'s block); null: every row from
// cam_i's block
struct MapStaged { int n = 0, cam_i = 0, cam_j = 0; const int32_t* d_row = nullptr; const int32_t* d_cam = nullptr; };
int map_stage(clc_ctx* ctx, clc_map_job& job, MapStaged& out);
int map_install(clc_ctx* ctx, clc_map_job& job, const MapStaged& staged);

// ---- the grow step (map_grow.hip; the host side in map_build.hip) --------------------------------------------------------------------
// The per-track state every grow launch works on: the track table, the landmark X[t] and the observation mask obs[t] (0: no landmark).
struct GrowState {
    const int32_t* table; const int32_t* n_tracks;      // cap x n_cams, the count in device memory
    int32_t n_cams, cap;
    double* X; uint32_t* obs;                           // cap tracks each
};
// the cameras' 2-D sides (count unused) and what the grow launch needs of every camera: [R|t], P = K [R|t], valid or not
struct GrowCams {
    GatherSide side[kMaxBatch];
    float scale[CLC_MAX_LEVELS];
    double Rt[kMaxBatch][12], P[kMaxBatch][12];
    uint32_t valid;
};
// the staged seed map (map_stage) into the per-track state: obs cleared, then { cam_a, cam_b } and X of the n seed rows
hipError_t launch_grow_scatter(const GrowState& s, const int32_t* map_track, const double* map_X, int n_rows, uint32_t seed_bits, hipStream_t stream);
// camera's resection list in ascending track id: X (3 N) | x (2 N) | track ids | rows, cap of each written; the count -- ALL of them, also
// past cap -- last, into d_n (nullable) and the pinned word h_n (nullable).  h_track / h_row: pinned mirrors, nullable.
struct ResectOut { double* X; double* x; int32_t* track; int32_t* row; int32_t* h_track; int32_t* h_row; int32_t* d_n; uint32_t* h_n; int32_t cap; };
hipError_t launch_resect_gather(const GrowState& s, const GatherSide& side, int camera, const ResectOut& out, hipStream_t stream);
// the grow of camera `camera` (valid in cams.valid): one thread per track
hipError_t launch_grow(const GrowState& s, const GrowCams& cams, int camera, int n_tracks, hipStream_t stream);
// the map of the tracks with a landmark, in ascending track id; the row count last into the pinned word h_n
struct GrowMapOut {
    double* X; int32_t* track; int32_t* cam; int32_t* row;            // device, cap rows
    double* h_X; int32_t* h_track; int32_t* h_cam; int32_t* h_row; uint8_t* h_obs;      // pinned mirrors, nullable
    uint32_t* h_n;
};
hipError_t launch_grow_compact(const GrowState& s, const GrowMapOut& out, hipStream_t stream);
// dst row i = row d_idx[i] of block src[d_cam[i]] (64 B rows; gather.hip); a camera outside [0, kMaxBatch) or without a block: zeros
struct RowSources { const uint4* src[kMaxBatch]; };
hipError_t launch_gather_rows_multi(const RowSources& srcs, const int32_t* d_cam, const int32_t* d_idx, uint4* dst, uint32_t n, hipStream_t stream);
// The a-contrario resection of the N correspondences in ctx->trk (kTrackLayout: X | x), through acr_drive like every solve
// (pose_batch.hip): clc_pnp_acransac's result on the same correspondences, bit for bit.  Rt: 12 doubles, zeros without a model.
int resect_solve(clc_ctx* ctx, int N, const clc_camera_k3& cam, int max_iteration, uint64_t seed, double precision, double* Rt, int* n_inliers,
                 double* error_max);
// The optional steps of a batch composition, null where absent: grow -- the grown stage; ba -- that stage bundle-adjusted (needs grow);
// align or sim, not both -- a replacement rule of map_update.hip in place of map_install.  map_init_batch (map_build.hip) is the seven
// clc_map_{init,update}_*_batch_dev entries behind their extern "C" names: it refuses an illegal combination or a ba that fails ba_check
// with CLC_ERR_BAD_ARG before any out field of grow, align or sim is written, then clears the given steps' out fields.
struct MapSteps { clc_map_grow* grow = nullptr; clc_map_ba* ba = nullptr; clc_map_align* align = nullptr; clc_map_align_sim* sim = nullptr; };
int map_init_batch(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, const MapSteps& steps);
int map_build_grow(clc_ctx* ctx, clc_map_job& job, clc_map_grow& gr, clc_map_ba* ba);
// ---- the bundle adjustment (map_ba.hip) ---------------------------------------------------------------------------------------------
// ba's in fields checked (CLC_ERR_BAD_ARG on `who`) and its out fields cleared
int ba_check(clc_ctx* ctx, clc_map_ba* ba, const char* who);
// The problem in device memory: cameras 0 .. n_cams - 1, those of `mask` adjusted; X / obs of n_points points.  x: the dense pixel block
// (n_points x n_cams x 2), or null: formed first from the track table and the cameras' 2-D sides (cams, table: a composition).
struct BaProblem {
    int n_cams, n_points; uint32_t mask;
    double K[kMaxBatch][3], Rt[kMaxBatch][12];           // Rt in / out (rewritten for the masked cameras when a step was accepted)
    double* X; const uint32_t* obs; const double* x;
    const GrowCams* cams; const int32_t* table;
};
// the whole step on the context's stream: the rounds, the waits, ba's out fields.  Returns CLC_OK for every CLC_BA_* status.
int ba_drive(clc_ctx* ctx, BaProblem& pb, clc_map_ba& ba);
// ---- the map replaced (map_update.hip) ---------------------------------------------------------------------------------------------------
// CLC_ERR_STATE unless the context holds a map with points
int map_align_state(clc_ctx* ctx, const char* who);
// the out fields of the two rules as a call leaves them when it ends before its step: no scale (1), no model (the identity)
void align_outputs_none(clc_map_align& job);
void sim_outputs_none(clc_map_align_sim& job);
// A rule on a staged map, installing it: the scale rule (job.X, the seed poses and -- gr != null, a grown stage whose rows are gathered by
// the stage's camera list -- the resected cameras' poses rescaled) or the a-contrario similarity (points and poses under sim.apply; no
// model: as they are).  Both are thin over the one step of map_update.hip.
int map_align_staged(clc_ctx* ctx, clc_map_job& job, const MapStaged& staged, clc_map_align& align, clc_map_grow* gr);
int map_align_sim_staged(clc_ctx* ctx, clc_map_job& job, const MapStaged& staged, clc_map_align_sim& sim, clc_map_grow* gr);

// Every consumer stream behind what `producer` holds now (pose_batch.hip): ONE event (ev: its owner's, created on first use), no host
// synchronisation; where an event call fails the host waits for the producer instead, and what that synchronisation reports is returned.
hipError_t order_behind(Event& ev, hipStream_t producer, const hipStream_t* consumers, size_t n);

// THE blocking wait for a word a kernel publishes in pinned memory (system-scope release): spins while *word == not_yet, looks at the
// clock every 1 024 spins, and once `ms` have passed since t0 synchronises `stream` ONCE (which also surfaces errors); fails -- `what`
// on ctx -- if that reports an error or the word is still not out.  What a failure means for the jobs in flight is the caller's.
template <class T> int wait_pinned(clc_ctx* ctx, const T* word, T not_yet, hipStream_t stream, std::chrono::steady_clock::time_point t0, int ms, const char* what)
{
    for (uint32_t spins = 0; __atomic_load_n(word, __ATOMIC_ACQUIRE) == not_yet;) {
        if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(ms)) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess || __atomic_load_n(word, __ATOMIC_ACQUIRE) == not_yet) return fail(ctx, CLC_ERR_HIP, what, e);
        }
    }
    return CLC_OK;
}

// a refinement's pinned record into the outputs of an inter-camera job (clc_inter_pose_job, clc_inter_dev_job)
template <class Job> void take_refined(Job& jb, const RefineOut& f)
{
    memcpy(jb.Rt, f.Rt, sizeof jb.Rt); memcpy(jb.cov, f.cov, sizeof jb.cov); jb.rmse = f.rmse; jb.n_refined = f.n_used;
}

} // namespace clc
#endif

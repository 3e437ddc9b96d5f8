// clc_internal.h -- shared declarations of libcoloc_hip.so's translation units (not installed).
#ifndef CLC_INTERNAL_H
#define CLC_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/coloc_hip.h"
#include "acr_kind.h"

namespace clc {

// ---- optional per-kernel event timing (clc_profile_* in the C ABI) ---------------------------
struct Profiler;
// Records an event on `stream` tagged (kernel, begin/end); no-op when prof is null or disabled.
void prof_mark(Profiler* prof, int kernel, bool begin, hipStream_t stream);

// ---- pyramid -------------------------------------------------------------------------------
struct LevelDesc {
    uint32_t w, h;        // level size
    uint32_t pitch;       // bytes per row (multiple of 64)
    uint32_t offset;      // byte offset of the level inside the pyramid arena
    // The same bytes a second time in 16-pixel-wide column strips (CLATCH's gather source; every other reader keeps the row-major
    // level): pixel (x, y) lies at tiled_offset + (x >> 4) * tiled_strip + y * 16 + (x & 15), so a 128-byte line holds 8 rows x 16 pixels.
    uint32_t tiled_offset;
    uint32_t tiled_strip; // bytes per strip: 16 x (h padded to a multiple of 8); pitch / 16 strips
};
__host__ __device__ inline uint32_t tiled_pos(const LevelDesc& L, uint32_t x, uint32_t y)
{
    return L.tiled_offset + (x >> 4) * L.tiled_strip + y * 16u + (x & 15u);
}
struct PyramidDesc {
    LevelDesc lv[CLC_MAX_LEVELS];
    float     f[CLC_MAX_LEVELS];      // resampling factor of level i (f_0 = 1)
    uint32_t  blk_begin[CLC_MAX_LEVELS + 1]; // first workgroup of level i in the fused resample launch
    int       levels;
};

// One launch: copy the caller's device image (d_src, src_pitch bytes per row) into level 0 of the
// arena and resample levels 1..L-1 from it.
hipError_t launch_pyramid(const PyramidDesc& pd, uint8_t* arena, const uint8_t* d_src, uint32_t src_pitch,
                          hipStream_t stream, Profiler* prof = nullptr);
// The same for the frames of n_img cameras in ONE launch: image b goes to the pyramid at arena + b * slot_stride.
static constexpr int kMaxBatch = CLC_MAX_BATCH;
hipError_t launch_pyramid_batch(const PyramidDesc& pd, uint8_t* arena, size_t slot_stride, const uint8_t* const* d_src,
                                int n_img, uint32_t src_pitch, hipStream_t stream, Profiler* prof = nullptr);

// ---- CLATCH ----------------------------------------------------------------------------------
hipError_t launch_clatch(const PyramidDesc& pd, const uint8_t* arena, const clc_keypoint* d_kps,
                         int n, uint64_t* d_desc, hipStream_t stream, Profiler* prof = nullptr);
// Keypoint lists of n_img cameras in ONE launch (blockIdx.y = camera; pyramid b at arena + b * slot_stride).
struct ClatchBatch {
    const clc_keypoint* kps[kMaxBatch];
    uint64_t*           desc[kMaxBatch];
    int                 n[kMaxBatch];
};
hipError_t launch_clatch_batch(const PyramidDesc& pd, const uint8_t* arena, size_t slot_stride, const ClatchBatch& batch,
                               int n_img, hipStream_t stream, Profiler* prof = nullptr);

// ---- detector (FAST-9 + NMS + orientation) ---------------------------------------------------
// Two launches (three when selecting) for the pyramids of n_img cameras (pyramid b at arena + b * slot_stride, score map b at score + b * slot_stride):
// d_mask: n_img x detect_total_tiles() x 16 keypoint-mask words, d_tcount: n_img x detect_total_tiles() tile counts (both rewritten
// by every call: nothing to clear); d_count[b][0] = keypoints written to d_kps[b] (<= maxkp), d_count[b][1] = found.
// d_select != nullptr: CLC_SELECT_STRONGEST, three launches.  d_select = kMaxBatch x detect_select_words() words, zero before the first
// call (every complete call leaves the score histograms in it zeroed again); *select_dirty = a call did not get to enqueue all its
// launches -- the next one clears the workspace first (a stream operation, no synchronisation).
hipError_t launch_detect(const PyramidDesc& pd, const uint8_t* arena, size_t slot_stride, int n_img, uint8_t* score, uint64_t* d_mask,
                         uint32_t* d_tcount, uint32_t threshold, uint32_t maxkp, clc_keypoint* const* d_kps, uint32_t* const* d_count,
                         hipStream_t stream, Profiler* prof = nullptr, uint32_t* d_select = nullptr, bool* select_dirty = nullptr);
uint32_t detect_select_words(const PyramidDesc& pd);
uint32_t detect_total_tiles(const PyramidDesc& pd);
// CLATCH with the keypoint count read from device memory (no host round trip after detect)
hipError_t launch_clatch_counted(const PyramidDesc& pd, const uint8_t* arena, const clc_keypoint* d_kps,
                                 const uint32_t* d_count, int max_n, uint64_t* d_desc, hipStream_t stream,
                                 Profiler* prof = nullptr);
// the same for n_img cameras in one launch: batch.n[b] = capacity of camera b's lists, d_count[b] = its count on the device
hipError_t launch_clatch_counted_batch(const PyramidDesc& pd, const uint8_t* arena, size_t slot_stride, const ClatchBatch& batch,
                                       const uint32_t* const* d_count, int n_img, hipStream_t stream, Profiler* prof = nullptr);

// ---- K2NN ------------------------------------------------------------------------------------
struct K2nnJobDev {
    const uint4* q;        // first query row of this job
    const uint4* t;        // first train row
    int32_t*     out;      // match indices, nq entries
    uint16_t*    best_out; // nullable
    uint16_t*    second_out; // nullable
    uint32_t     nq, nt;
    uint32_t     thr;      // already truncated to 8 bits
    uint32_t     qblocks;  // ceil(nq / queries-per-workgroup)
    uint32_t     splits;   // train-dimension splits
    uint32_t     t_per_split;
    uint32_t     partial_off; // first uint2 of this job's partial slab (slab mode) / of its top-2 row (atomic mode)
    uint32_t     nq_pad;      // row length of the slab
    uint32_t     atomic_merge;// 1: splits are folded with two atomicMin per query into a top-2 row, no slab
    uint32_t     cnt_off;     // atomic mode: first arrival counter (one per query block) of this job, in uint32 units
    // device-resident row counts (nullable; the multi-camera step plans its shares on the block CAPACITY and lets the sweep read the
    // gathered counts itself, so that no host synchronisation sits between the exchange and the sweep): with cnt_q the job covers
    // query rows [q_row0, q_row0 + nq) of a set of *cnt_q valid rows -- rows past the end are answered -1 --, with cnt_t the train
    // set has min(nt, *cnt_t) rows.  nq / nt stay the planned sizes (grid, splits, result layout).
    const int32_t* cnt_q;
    const int32_t* cnt_t;
    uint32_t     q_row0;
    uint32_t     xcd_rot;     // matrix sweep: the XCD (workgroup id & 7) that takes this job's query block 0 -- the jobs of a launch
                              // continue round the XCDs where the job before them stopped (k2nn_plan)
    // matrix sweep, ONE job that fills the chip once (round 4): unequal train shares by the wave slot a workgroup lands on.  The first
    // 256 workgroup ids take slot 0 of every SIMD, the next 256 slot 1, the rest slot 2 (measured: slot == id / 256 for 760 of 760), and the
    // matrix pipe serves a lower slot first: with equal shares the slot-0 workgroup of a CU ends its loop at 17.3 us, slot 1 at 19.0, slot 2
    // at 22.5, the last part of it alone on the CU at a quarter of the CU's rate.  bias_a / bias_b = train tiles of a slot-0 / slot-1 split
    // (0 = equal shares); the slot-2 splits of a query block take what is left.
    uint32_t     bias_a, bias_b;
    uint32_t     bias_magic;  // ceil(2^32 / qblocks): workgroup id / qblocks as a multiply-high (exact for ids below 2^16)
    uint32_t     slot_wgs;    // biased plans: workgroup ids per wave slot in the plan's id space (CUs of one XCD, or of the device)
    // acceptance rule of the finalize (uniform per job; the sweep and the top-2 fold do not depend on it):
    // K2NN_RULE_K2NN (0, the default of K2nnJobDev{}): second - best > thr (CUDAK2NN.cu:75);
    // K2NN_RULE_RATIO: a second distance exists and (float)best < r2 * (float)second (OpenMVG DistanceRatioMatch as CPUMatcher calls it)
    uint32_t     rule;
    float        r2;          // ratio * ratio, rounded to float once on the host
};
enum { K2NN_RULE_K2NN = 0, K2NN_RULE_RATIO = 1 };
// what the planner needs to know about the device (clc_ctx_create fills it from the HIP device attributes)
static constexpr uint32_t kK2nnXcds = 8;       // XCDs the sweep kernel's workgroup map is compiled for (every gfx950 part has eight)
struct K2nnDevice {
    uint32_t n_xcd = kK2nnXcds;                // hipDeviceAttributeNumberOfXccs
    uint32_t n_cu = 256;                       // multiProcessorCount
};
// the sizes a sweep workgroup works with (scalar loads when the counts live in device memory)
__device__ __forceinline__ uint32_t k2nn_job_nq(const K2nnJobDev& job)
{
    if (!job.cnt_q) return job.nq;
    const int left = *job.cnt_q - (int)job.q_row0;
    return left <= 0 ? 0u : ((uint32_t)left < job.nq ? (uint32_t)left : job.nq);
}
__device__ __forceinline__ uint32_t k2nn_job_nt(const K2nnJobDev& job)
{
    if (!job.cnt_t) return job.nt;
    const int c = *job.cnt_t;
    return c <= 0 ? 0u : ((uint32_t)c < job.nt ? (uint32_t)c : job.nt);
}
static constexpr int kK2nnJobsPerLaunch = 16;
// Passed BY VALUE as the kernel argument (1.2 KB of kernarg): no job upload, no staging hazard.
struct K2nnJobList {
    K2nnJobDev j[kK2nnJobsPerLaunch];
    // job 0 with unequal shares by wave slot (bias_a != 0), filled by launch_k2nn (no integer division in the kernel: ~30 vector
    // instructions each).  bias_magic == 0: what workgroup w = id >> 3 of an XCD takes -- query block of the XCD (bits 0..4), first train
    // tile (5..22), train tiles (23..31: k2nn.hip kBias*); bias_magic != 0: per query block, see launch_k2nn
    uint32_t bias_tab[128];
};
static_assert(sizeof(K2nnJobList) <= 4096, "K2nnJobList is passed as a kernel argument: it must stay within the 4 KB kernarg segment");
struct K2nnPlan {
    size_t   partial_elems;// uint2 entries needed
    bool     atomic_merge; // every job fits the 22-bit global train index -> atomic top-2 merge
};
// The two formulations of the sweep (k2nn.hip): FP4 matrix pipe (default) and round 1's xor + popcount VALU kernel.
enum { K2NN_MATRIX = 0, K2NN_POPCOUNT = 1 };
// Fill the derived fields of jobs[] (qblocks/splits/t_per_split/partial_off/nq_pad).
// bias_a / bias_b: train share of a workgroup on wave slot 0 / 1 in 1/256 of the equal share (0: equal shares); used by single-job one-round plans only
K2nnPlan k2nn_plan(K2nnJobDev* jobs, int njobs, int target_blocks, bool xcd_map = true, int formulation = K2NN_MATRIX, int bias_a = 0, int bias_b = 0,
                   K2nnDevice dev = K2nnDevice{});
// Sweep + merge over all jobs (chunks of kK2nnJobsPerLaunch per launch pair).
// In atomic mode d_partial must hold 0xFF bytes in every entry the jobs use (top-2 rows and arrival counters);
// the workgroup that completes a query block leaves it that way again (self re-arming workspace).
// d_stamps (matrix formulation only, nullable): run the diagnostic build whose workgroups record their shader-clock /
// real-time stamps, 4 uint64 per workgroup of the launch grid
// probe: the share probe's launches (the default matrix sweep under a symbol of its own, so that kernel traces keep them apart)
hipError_t launch_k2nn(const K2nnJobDev* jobs, int njobs, uint2* d_partial, hipStream_t stream,
                       Profiler* prof = nullptr, int formulation = K2NN_MATRIX, uint64_t* d_stamps = nullptr, bool probe = false);
int k2nn_queries_per_block(int formulation);

// ---- PnP -------------------------------------------------------------------------------------
hipError_t launch_pnp_residuals(const double* d_Rt, int H, const double* d_X, const double* d_x,
                                int N, const double* d_K, double* d_err, hipStream_t stream,
                                Profiler* prof = nullptr);
hipError_t launch_pnp_score(const double* d_Rt, int H, const double* d_X, const double* d_x, int N,
                            const double* d_K, double thr2, int32_t* d_count, double* d_cost,
                            hipStream_t stream, Profiler* prof = nullptr);

// The records the pose launches leave for the host (device or pinned host memory; the host reads them as they are).
struct PnpResult {      // launch_pnp_ransac: one packed record so the host needs a single D2H copy
    double Rt[12];
    double cost;
    int32_t h;          // winning hypothesis (< 0: none)
    int32_t count;
};
struct EpiResult {      // launch_essential_ransac: the same for the five-point problems
    double E[9];
    double F[9];
    double cost;
    int32_t h;
    int32_t count;
};
struct RefineOut {      // launch_pnp_refine
    double Rt[12];
    double cov[36];
    double cost;        // final 1/2 sum rho
    double rmse;        // sqrt(final_cost / (2 n_used))  (Refiner.hpp:226)
    int32_t iterations;
    int32_t n_used;
    int32_t ready;      // written LAST (system-scope release): a host that cleared it in a pinned record can poll it instead of
    int32_t pad_;       // synchronising the stream
};

// P3P hypotheses for S minimal samples (4 slots each) -> score -> select + inlier mask of the winner.
// d_result receives one PnpResult.
// hs (nullable): the inputs are still in the caller's pinned host buffer [X 3N | x 2N | K 16 | samples]; the first
// launch reads them from there and stages them into d_X.. itself, the last one mirrors record + mask into pinned host
// memory -- no copy commands around the launches.
struct PnpHostStage {
    const double* src;      // pinned host input block
    int           n_doubles;// its length
    uint8_t*      h_mask;   // pinned host: N bytes
    void*         h_result; // pinned host: PnpResult
};
hipError_t launch_pnp_ransac(const double* d_X, const double* d_x, int N, const double* d_K, const int32_t* d_samples,
                             int S, double thr2, double* d_Rt, int32_t* d_count, double* d_cost, uint8_t* d_mask,
                             void* d_result, hipStream_t stream, Profiler* prof = nullptr, const PnpHostStage* hs = nullptr);
// five-point problems for S minimal samples (10 slots of {F(9), E(9)} each) -> symmetric-epipolar score -> select + mask.
// d_result: one EpiResult.
hipError_t launch_essential_ransac(const double* d_x1, const double* d_x2, int N, const double* d_K1, const double* d_K2,
                                   const int32_t* d_samples, int S, double thr2, double* d_FE, int32_t* d_count, double* d_cost,
                                   uint8_t* d_mask, void* d_result, hipStream_t stream, Profiler* prof = nullptr);
// symmetric epipolar distance of H fundamental matrices: d_err != null -> H x N residuals, else counts / costs
hipError_t launch_epipolar(const double* d_F, int H, const double* d_x1, const double* d_x2, int N, double thr2, double* d_err,
                           int32_t* d_count, double* d_cost, hipStream_t stream, Profiler* prof = nullptr);
// Levenberg-Marquardt refinement of one pose over the (masked) correspondences + 6x6 covariance.
// d_out: one RefineOut.
hipError_t launch_pnp_refine(const double* d_Rt_in, const double* d_X, const double* d_x, const uint8_t* d_mask, int N,
                             const double* d_K, double huber_a, int max_iter, void* d_out, hipStream_t stream,
                             Profiler* prof = nullptr, const int32_t* d_valid = nullptr, void* h_out = nullptr);
// (h_out: pinned host record written INSTEAD of d_out, so that no device-to-host copy command is needed)

// inter_scale_kernel (inter_dev.hip): what the scale step of the inter-camera path leaves in pinned memory
struct InterScaleRec {
    double scale;
    int32_t stage, n_common, n_map_matches;
    int32_t ready;      // written LAST (system-scope release)
};

// ---- a-contrario RANSAC (acransac.hip) -----------------------------------------------------------------------
static constexpr int kAcrMaxBatch = 128;           // iterations evaluated per round
static constexpr int kAcrMaxN = 16384;             // correspondences per solve: 8 B x 16 384 = 128 KB of LDS per model slot (16 elements per thread)
static constexpr size_t kAcrMaxLds = (size_t)kAcrMaxN * 8;
struct AcrProblem {        // passed by value to every kernel of a solve
    int kind;              // an AcrKindId (acr_kind.h).  Models: [R|t], 12 doubles (resection); {F, E}, 18 (essential); F / H in normalised
                           // coordinates, 9 in a stride of 12 (fundamental, homography); A = [sR | t], 12 (similarity)
    int n, m, max_models, model_doubles;   // m, max_models, model_doubles: acr_kind(kind)'s m, M, md, filled in by the host
    int batch_cap;         // most iterations a round evaluates (<= kAcrMaxBatch): the schedule, not the result, depends on it
    const double* a;       // X (3 n)  | x1 (2 n; fundamental, homography: conditioned by the image size) | X_new (3 n)
    const double* b;       // x (2 n)  | x2 (2 n)                                                              | X_old (3 n)
    const double* K1;      // 9 doubles row-major (+ padding)
    const double* K2;
    const float* logc_n;   // log10 C(n, k), k = 0..n
    const float* logc_k;   // log10 C(k, m)
    double loge0, logalpha0, mult, max_threshold;
    double norm;           // resection: 1 / focal (residuals are scaled to the normalised camera plane); essential, similarity: 1; fundamental, homography: N2(0,0)
    uint64_t seed;
    double K1v[9];         // resection: K1 by value -- kernel arguments sit in scalar registers, a load of K1 is a ~1 us round trip
};
struct AcrState {          // device resident; the host sees one packed 8-byte word of it after every round
    double min_nfa, error_max;
    double model[18];
    int32_t n_inliers, best_iter;
    int32_t iter, n_iter, reserve;
    int32_t n_index, index_all, ac_mode;
    int32_t rounds, last_batch;
    int32_t cur_batch;     // iterations the NEXT round evaluates (the solve / nfa kernels read it from here: rounds are enqueued
    int32_t grow;          // one ahead of the host's knowledge); grow = batch size while no event has happened (32, 64, 128)
    int32_t rounds_eval;   // rounds that evaluated at least one iteration (`rounds` also counts the empty round enqueued ahead)
    int32_t evaluated;     // acr_round_kernel: the slots of the other parity hold a batch of cur_batch iterations to replay (0: a fresh run)
};
struct AcrResult {
    double model[18];
    double min_nfa;
    double error_max;      // un-normalised: pixels (resection), squared pixels (essential)
    int32_t n_inliers;
    int32_t valid;         // iteration that produced the model, -1: no meaningful model
    int32_t iterations, rounds;
};
struct AcrHyp {            // per model slot, written by the nfa kernel
    double nfa;            // min_k NFA(k); +inf for an empty slot
    double e_k;            // the k-th smallest residual (kernel units)
    int32_t k;             // minimising k
    int32_t n_le;          // residuals <= max_threshold (upper-bound mode gate)
};
// where the round that COMPLETES a run leaves the result (the finish work rides in that round's launch, and the host returns as soon as
// the polled word says "done" instead of launching a finish kernel behind the round enqueued ahead)
struct AcrFinish {
    uint8_t* d_mask; AcrResult* d_res;                 // device copies (the refinement reads them)
    uint8_t* h_mask; int32_t* h_inliers; AcrResult* h_res;     // pinned host memory (nullable)
};
// Everything the launches of ONE solve work on.  The solves of a group (pose_batch.hip: acr_drive) share their launches, up to kMaxBatch
// chains of one kind per launch (blockIdx.y = chain): their rounds advance in lockstep, one launch (resection) or two (two-view) per round
// for all of them (round 5: eight poses in chains of their own were ~80 launches from one thread).
struct AcrChain {
    AcrProblem pb;
    AcrState* states; AcrHyp* hyps; uint32_t* sorted; double* models;      // two copies each, indexed by launch parity
    uint32_t* best_inliers; uint32_t* index_set;
    unsigned long long* h_word;
    AcrFinish fin;
};
struct AcrChains { AcrChain c[kMaxBatch]; };
// One round of n_chains solves of one kind (a single solve: n_chains = 1): ONE launch for every kind (replay of the previous round +
// samples + P3P / seven-point / four-point / similarity + residuals / sort / NFA) but the essential, which takes TWO (replay + samples +
// five-point; nfa).  The states,
// slots, sorted lists and models of a chain hold two copies: this launch reads copy par ^ 1 and writes copy par; the initial state goes
// into copy 1 and the first launch has par 0.  batch_bound (iterations the grids cover, >= the batch the device states ask for) and the
// sort width cover the largest chain; chain.fin: where the round that completes a run leaves mask / inlier list / result record.
hipError_t launch_acr_round(const AcrChains& chains, int n_chains, int par, int batch_bound, hipStream_t stream);
// the inputs of n_chains solves, pinned host blocks -> device workspaces, in one launch
// d_a / d_b / n_corr (all three or none; entries nullable): chain c's first a_width[c] n_corr[c] + 2 n_corr[c] doubles -- the solve's
// a | b -- come from the DEVICE blocks d_a[c] and d_b[c] instead of the pinned block (gather.hip; the track kernel's X | x: a_width 3, the
// default; the pair kernel's x1 | x2: a_width 2); everything behind them still comes from the pinned block.  cond (nullable;
// cond[c] = { d, tx, ty }, d == 0: none): the two-view 'F' / 'H' conditioning x * d + tx, y * d + ty of the device points on their way in
hipError_t launch_acr_stage(const double* const* h_pinned, double* const* d_dst, const size_t* n_doubles /* even */, int n_chains,
                            hipStream_t stream, const double* const* d_a = nullptr, const double* const* d_b = nullptr,
                            const int* n_corr = nullptr, const int* a_width = nullptr, const double (*cond)[3] = nullptr);

// ---- the gathers (gather.hip): Localizer::setupTracks and the loop of RobustMatcher::computeRelativePose (RobustMatcher.hpp:393-398) ----
// on the device.  ONE ordered compaction; a track writes x | X, a pair x1 | x2.
struct UdCamera { double focal, ppx, ppy, k1, k2, k3; };              // Pinhole_Intrinsic_Radial_K3 (ud_pixel.h)
// one 2-D side: rows of detector keypoints or of float feature positions (exactly one), and the camera that undistorts them
struct GatherSide {
    const uint32_t* count;                                              // nullable: the rows really there (a detector's counter)
    const clc_keypoint* kps; const float* feat; int feat_stride;
    UdCamera cam;
};
// what the compaction itself reads and writes
struct GatherJob {
    const int32_t* match; GatherSide a;                                 // in: row of side a (the query) -> train row, or -1
    int nq, cap;                                                        // queries; most correspondences written
    int32_t* n; uint32_t* h_n;                                          // out: the count, device and pinned (both nullable)
};
struct TrackJobDev : GatherJob {
    double* X; double* x; int32_t* query; int32_t* map;                 // out, device (cap tracks; query / map nullable)
    int32_t* h_query; int32_t* h_map;                                   // out, pinned host mirrors (nullable)
};
struct PairJobDev : GatherJob {
    GatherSide b; int nt;                                               // in: the train side, camera B
    double* x1; double* x2; int32_t* pair_q; int32_t* pair_t;           // out, device (cap pairs; pair_q / pair_t nullable)
    int32_t* h_q; int32_t* h_t; double* h_x1; double* h_x2;             // out, pinned host mirrors (nullable)
};
struct TrackJobs {
    TrackJobDev j[kMaxBatch];
    const double* map_X; int map_n;
    float scale[CLC_MAX_LEVELS];      // the pyramid levels' scales, from the host (level_scales, clc_ctx.h)
};
struct PairJobs {
    PairJobDev j[kMaxBatch];
    float scale[CLC_MAX_LEVELS];      // as TrackJobs::scale
};
// The common features of two maps as 3-D / 3-D pairs (clc_map_align_sim_dev): query = old map row q, match[q] = new map row.  Pair i
// writes X_new | X_old into the solve's point blocks and (q, m) into the common lists; the bounding box of the X_old written and then the
// count (GatherJob::n / h_n; all of them, also past cap) come out in the same launch, the box in front of the count.  a: unused but count.
struct MapPairJobDev : GatherJob {
    const double* old_X; const double* new_X; int n_new;               // in: the installed map's points, the new map's, its rows
    double* xn; double* xo; int32_t* cq; int32_t* ct;                   // out, device (cap pairs)
    double* h_box;                                                      // out, pinned: { min x, y, z, max x, y, z } of xo (6 doubles)
};
struct MapPairJobs { MapPairJobDev j[1]; };
hipError_t launch_gather(MapPairJobs& jobs, hipStream_t stream);
// ONE launch for n_jobs <= kMaxBatch cameras / pairs (blockIdx.y = job); scale[] is filled in here
hipError_t launch_gather(TrackJobs& jobs, int n_jobs, hipStream_t stream);
hipError_t launch_gather(PairJobs& jobs, int n_jobs, hipStream_t stream);
// validates a job's inputs (a track's against the context that holds the map points) and fills the kernel's view of them; the outputs
// and cap are the caller's.  who: the text of a refused nq / nt / d_match
int gather_inputs(clc_ctx* ctx_map, const clc_track_job& job, TrackJobDev& out, const char* who);
int gather_inputs(clc_ctx* ctx, const clc_pair_job& job, PairJobDev& out, const char* who);
// the seven-point / four-point models (kAcrFundamental: <= 3 per sample, kAcrHomography: 1) of S samples of normalised correspondences: d_out S x M x 9, NaN = no model
hipError_t launch_twoview_minimal(int kind, const double* d_x1, const double* d_x2, int N, const int32_t* d_samples, int S, double* d_out, hipStream_t stream);

// ---- the 3-D similarity (kAcrSimilarity of the a-contrario path; sim3_math.h) -------------------------------------------------------------------
// What the refit launch behind the last round leaves (device and pinned): the similarity NEW -> OLD that is reported.
struct Sim3Out {
    double s, R[9], t[3], A[12];      // found: the refit's (refit = 1) or the minimal model's; else s = 1, R = I, t = 0, A = [I | 0]
    int32_t found;          // sim3_accepted(valid, n_inliers)
    int32_t refit;
    int32_t n_inliers;      // 0 where not found
    int32_t ready;          // written LAST (system-scope release)
};
// the minimal models of S samples of three correspondences each: d_out S x 12, NaN = degenerate sample or an index outside [0, N)
hipError_t launch_sim3_minimal(const double* d_x, const double* d_y, int N, const int32_t* d_samples, int S, double* d_out, hipStream_t stream);
// ONE workgroup behind the round that completed a similarity run: acceptance rule, the inliers of d_mask in ascending index (d_list: N words
// of scratch), Umeyama's refit by partial sums of kSim3Chunk inliers, the record to d_out and (nullable) the pinned h_out, `ready` last
hipError_t launch_sim3_refit(const AcrResult* d_res, const uint8_t* d_mask, const double* d_x, const double* d_y, int N, int32_t* d_list,
                             Sim3Out* d_out, Sim3Out* h_out, hipStream_t stream);

// ---- the pose from a prediction (pose_prior.hip; include/coloc_hip.h: clc_track_prior_dev, THE RULE) -----------------------------------------
// What the kernel leaves in PINNED memory, one per job
struct PriorOut {
    double Rt[12];
    double cov[36];         // zeros: CLC_TRACK_PRIOR_FEW, or the 6 x 6 is not positive definite
    double cost, rmse;      // 1/2 sum rho and sqrt(cost / (2 n_inliers)) at the pose over the mask
    int32_t n_tracks;       // the count as read (all tracks, also past the capacity)
    int32_t n_inliers, iterations, rounds_run, converged, result;
    int32_t capacity;       // 1: more tracks than the block holds, the kernel worked on the first `cap`
    int32_t ready;          // written LAST (system-scope release)
};
struct PriorJobDev {
    const double* X; const double* x;          // the tracks: 3 N | 2 N (a context's track block, or an upload)
    const int32_t* n_dev; int n;               // N: the device word where given (the gather's count), else n
    int cap;                                   // most tracks X | x hold (<= 16 384)
    double fx, sk, cx, fy, cy;                 // K = { fx, sk, cx; 0, fy, cy; 0, 0, 1 }
    double Rt[12];                             // the prior
    double g2, huber_a;
    int rounds, max_iter, min_inliers;
    uint8_t* h_mask; PriorOut* out;            // pinned: cap bytes, the record
};
struct PriorJobs { PriorJobDev j[kMaxBatch]; };
// ONE launch for n_jobs <= kMaxBatch poses (blockIdx.x = job, one workgroup each)
hipError_t launch_pose_prior(const PriorJobs& jobs, int n_jobs, hipStream_t stream);

} // namespace clc
#endif

/*
 * coloc_hip.h -- C ABI of libcoloc_hip.so: the MI355X (gfx950) implementation of CoLoC's
 * describe -> 512-bit Hamming 2-NN match -> batched PnP scoring hot path.
 *
 * This is the drop-in boundary.  It replaces the reference's static library `koral`
 * (CMakeLists.txt:37 = src/CUDALERP.cu + src/CLATCH.cu + src/CUDAK2NN.cu) and the CUDA-runtime
 * plumbing inside include/coloc/GPUDetector.hpp / GPUMatcher.hpp.  Plain C types only: no C++
 * types, no exceptions, no exit() -- every entry point returns an int status (the reference
 * aborts via exit(code) on four calls and ignores all other CUDA errors,
 * GPUMatcher.hpp:33-41,188-195).
 *
 * Conventions
 *   - descriptors: rows of 64 bytes = 16 little-endian uint32 = 8 little-endian uint64
 *     (CLATCH.cu:185-188, CUDAK2NN.cu:47-52).
 *   - `h_` pointers are host memory (caller-owned), `d_` pointers are device memory on the
 *     context's GPU (caller-owned unless stated); `stream` is a hipStream_t passed as void*
 *     (NULL = the context's own stream).  Host-pointer entry points are synchronous on return,
 *     like the reference (CUDAK2NN.cu:80, GPUDetector.hpp:290); `_dev` entry points only enqueue.
 *   - device buffers owned by the context are sized from the options' maxkp with an explicit
 *     capacity check (CLC_ERR_CAPACITY); the reference has none (GPUDetector.hpp:135,281).
 *   - inputs need no padding (the reference needs +8 readable train vectors,
 *     GPUMatcher.hpp:183-186).
 *   - a context is thread-compatible: one host thread at a time; several contexts per
 *     process / device are fine.  The one process-wide state is the descriptor table behind
 *     clc_desc_cache_* (one per device, guarded by a lock; what one context publishes, another's
 *     host-pointer match calls may read).  A context owns ONE set of device
 *     workspaces (pyramid arena, matcher top-2 rows and arrival counters, pose scratch), so the `_dev`
 *     calls made on one context must be ordered with respect to each other -- same stream, or
 *     streams joined by events; use one context per concurrently running stream.
 */
#ifndef COLOC_HIP_H
#define COLOC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1: rounds 1-3.  2: round 4's additions (clc_detect_batch_dev, clc_desc_cache_*, clc_k2nn_plan_query, clc_mc_open_peers,
 * clc_pnp_localize_ac_batch / clc_pose_job, one-rank communicators in clc_mc_create).  3: round 5's additions (clc_desc_cache_mode,
 * clc_describe_match_pair_dev, clc_essential_acransac_batch, clc_inter_pose_batch, clc_k2nn_device_info) and round 6's changes
 * (clc_describe_match_pair_dev lost its `chunks` argument, CLC_K2NN_MATRIX_PLAIN is gone, the descriptor hand-over is by ownership:
 * clc_desc_cache_publish returns a handle).  4: the 'F' / 'H' models of the two-view filter (clc_two_view_acransac, _batch, clc_two_view_minimal);
 * the distance-ratio entries (clc_match_ratio_*, clc_match_map_ratio*, clc_ratio_matches_to_pairs) came later under 4: new entry points only;
 * so did the keypoint selection rule (clc_detect_set_selection, clc_detect_selection) and the device-side 2D-3D tracks
 * (clc_set_map_points, clc_track_build_dev, clc_track_localize_dev, clc_track_localize_batch_dev) and two-view correspondences
 * (clc_pair_build_dev, clc_pair_filter_dev, clc_pair_filter_batch_dev), the inter-camera step from device memory (clc_inter_*_dev) and
 * the map built on the device (clc_tracks_build_dev, clc_map_build_dev, clc_map_init_batch_dev) and replaced at the old map's scale
 * (clc_map_align_dev, clc_map_update_batch_dev), and the a-contrario 3-D similarity that aligns a replaced map to the old one
 * (clc_sim3_acransac, clc_sim3_minimal, clc_map_align_sim_dev, clc_map_update_sim_batch_dev), and a tracked frame's pose from the
 * prediction (clc_track_prior_dev, clc_track_prior_batch_dev, clc_pnp_refine_prior).
 * Bindings check clc_abi_version() BEFORE resolving symbols an older library does not export. */
#define CLC_ABI_VERSION 4
#define CLC_DESC_BYTES 64
#define CLC_MAX_LEVELS 8
#define CLC_MAX_BATCH 8    /* cameras per clc_describe_batch_dev / clc_detect_batch_dev call */
#define CLC_DETECT_MAX_WIDTH 4096   /* widest image the GPU detector takes (its row-walk replay keeps a row's pre-test bits in LDS) */

/* status codes */
enum {
    CLC_OK = 0,
    CLC_ERR_BAD_ARG = 1,    /* null pointer, negative count, misaligned device pointer ...      */
    CLC_ERR_CAPACITY = 2,   /* more keypoints / descriptors / hypotheses than the ctx was sized for */
    CLC_ERR_HIP = 3,        /* a HIP runtime call failed; see clc_last_error_string            */
    CLC_ERR_NO_DEVICE = 4,  /* no usable gfx950 device                                          */
    CLC_ERR_STATE = 5       /* call order violated (e.g. describe before pyramid_build)        */
};

/* mirrors coloc::DetectorOptions, include/coloc/colocData.hpp:29-36 */
typedef struct clc_detector_opts {
    float    scale_factor;  /* 1.2f in coloc_node.cpp:77 */
    uint8_t  scale_levels;  /* 8; at most CLC_MAX_LEVELS (CLATCH indexes d_all_tex[8], CLATCH.cu:160) */
    uint32_t width;
    uint32_t height;
    uint32_t maxkp;
    uint8_t  thresh;        /* FAST threshold (host feeder), coloc_node.cpp:81 */
} clc_detector_opts;

/* mirrors coloc::MatcherOptions, include/coloc/colocData.hpp:38-42 */
typedef struct clc_matcher_opts {
    float    distRatio;     /* unused by the 2-NN difference rule and, like CPUMatcher, by the ratio entries (they take ratio) */
    int      thresh;        /* map-tracking threshold (Mopts.thresh = 60, coloc_node.cpp:85)    */
    uint32_t maxkp;
} clc_matcher_opts;

/* wire format shared with the host feeder: include/coloc/Keypoint.h:155-163, sizeof == 20 */
typedef struct clc_keypoint {
    int32_t x;      /* level-local pixel column */
    int32_t y;      /* level-local pixel row    */
    uint8_t score;
    float   angle;  /* radians                  */
    uint8_t scale;  /* pyramid level 0..7       */
} clc_keypoint;

typedef struct clc_ctx clc_ctx;

/* one unit of matcher work for clc_match_jobs_dev: queries [q_begin, q_begin+nq) of a query set
 * against a whole train set.  Offsets are in descriptors (rows of 64 B) from the base pointers. */
typedef struct clc_match_job {
    uint32_t q_offset;   /* first query row, relative to d_desc_base        */
    uint32_t nq;
    uint32_t t_offset;   /* first train row, relative to d_desc_base        */
    uint32_t nt;
    uint32_t out_offset; /* first int32 of the result, relative to d_match  */
    uint32_t threshold;  /* truncated to 8 bits, see clc_match_2nn          */
} clc_match_job;

/* descriptor hand-over (see clc_desc_cache_mode below) */
/* what a publication hands out: the host address and row count it stands for, and the generation it was stamped with (a process-wide
 * counter: publishing the same address again, destroying the publishing context -- freeGPUMemory -- or a lookup that sees changed
 * rows ends a generation).  clc_desc_handle_live: 1 while that very publication still stands. */
typedef struct clc_desc_handle {
    const void* host;
    uint64_t    generation;
    uint32_t    count;
    uint32_t    slot;
} clc_desc_handle;

/* ---- lifecycle --------------------------------------------------------------------------- */

int clc_abi_version(void);
const char* clc_status_string(int status);

/* Replaces the constructors GPUDetector(DetectorOptions) (GPUDetector.hpp:70-138) and
 * GPUMatcher(MatcherOptions) (GPUMatcher.hpp:70-95): allocates pyramid levels, keypoint /
 * descriptor / match buffers and the learned triplet table on device `device_id`.
 * Either opts pointer may be NULL if that half is not used. */
int clc_ctx_create(int device_id, const clc_detector_opts* dopts, const clc_matcher_opts* mopts,
                   clc_ctx** out_ctx);
/* Replaces freeGPUMemory() (GPUDetector.hpp:144-155, GPUMatcher.hpp:102-108). */
int clc_ctx_destroy(clc_ctx* ctx);
const char* clc_last_error_string(const clc_ctx* ctx);
/* Blocks until everything enqueued on the context's stream has finished. */
int clc_sync(clc_ctx* ctx);
/* The context's hipStream_t (as void*), for callers that enqueue their own work in order. */
void* clc_stream(clc_ctx* ctx);
/* The device the context lives on. */
int clc_ctx_device(const clc_ctx* ctx);

/* ---- kernel timing (replaces the std::chrono prints around CUDAK2NN, GPUMatcher.hpp:204-206) ---
 * When enabled, every kernel launch made through this context is bracketed by a pair of HIP
 * events on the stream it is launched on.  clc_profile_read drains the finished pairs (it
 * synchronises those streams) and returns the accumulated device time and launch count of one
 * kernel since the last clc_profile_reset. */
enum {
    CLC_KERNEL_PYRAMID = 0,
    CLC_KERNEL_CLATCH = 1,
    CLC_KERNEL_K2NN_SWEEP = 2,
    CLC_KERNEL_K2NN_MERGE = 3,
    CLC_KERNEL_PNP_RESIDUALS = 4,
    CLC_KERNEL_PNP_SCORE = 5,
    CLC_KERNEL_DETECT = 6,      /* the FAST-9 / NMS / emit launch group, bracketed as one */
    CLC_KERNEL_COUNT = 7
};
/* on = 0: off; 1: bracket every kernel; otherwise a mask, bit (k + 1) selecting kernel k. */
int clc_profile_enable(clc_ctx* ctx, int on);
int clc_profile_reset(clc_ctx* ctx);
int clc_profile_read(clc_ctx* ctx, int kernel, double* total_ms, int* launches);
const char* clc_kernel_name(int kernel);

/* ---- pyramid: replaces CUDALERP() (CUDALERP.h:166) + the level loop GPUDetector.hpp:232-255 -- */

/* Upload a WxH u8 image (tight rows) as level 0 and resample levels 1..L-1 from it. */
int clc_pyramid_build(clc_ctx* ctx, const uint8_t* h_img, uint32_t width, uint32_t height);
/* Same from a device image with `pitch` bytes per row. */
int clc_pyramid_build_dev(clc_ctx* ctx, const void* d_img, uint32_t width, uint32_t height,
                          size_t pitch, void* stream);
/* Geometry and device address of one level (GPUDetector.hpp:109-114 dims). */
int clc_pyramid_level(const clc_ctx* ctx, int level, uint32_t* w, uint32_t* h, size_t* pitch,
                      const void** d_ptr);
/* Download one level into tight host rows (the reference's per-level D2H, GPUDetector.hpp:265). */
int clc_pyramid_download(clc_ctx* ctx, int level, uint8_t* h_out);

/* ---- detect: replaces the host loop KFAST<true,true> + featureAngle per level ---------------
 * (GPUDetector.hpp:262-277; KFAST.h:502-540; FeatureAngle.h:197-246) -- on the GPU, all levels.
 * Keypoints come out in the reference's order: level-major, then (y, x) ascending, with level-local
 * integer coordinates, corner score, orientation and level.  FAST threshold = opts.thresh.
 * At most DetectorOptions.maxkp keypoints are kept; *n_found reports how many there were.  WHICH ones are kept when a frame has
 * more is this library's choice, not the reference's: the reference writes past its maxkp-sized buffers instead
 * (GPUDetector.hpp:135,281).  The context's selection rule (clc_detect_set_selection) decides:
 *   CLC_SELECT_FIRST (the default): the first maxkp in that order -- a frame that overflows loses its coarse levels.
 *   CLC_SELECT_STRONGEST: the maxkp with the highest corner scores, still in that order.  With c the largest score such that at
 *     least maxkp keypoints score >= c, every keypoint scoring above c is kept, and of those scoring exactly c the first
 *     maxkp - #{score > c} in that order; in numpy, D[sort(argsort(-score, kind="stable")[:maxkp])] of the uncapped list D.
 *     The result does not depend on scheduling; a frame with no more than maxkp keypoints comes out as under CLC_SELECT_FIRST.
 * Either way {written, found} = {min(found, maxkp), found}, and the fields of a kept keypoint are those it has in the uncapped list. */
enum { CLC_SELECT_FIRST = 0, CLC_SELECT_STRONGEST = 1 };
/* The rule of every later detect call of the context (clc_detect, clc_detect_dev, clc_detect_and_describe, clc_detect_and_describe_view,
 * clc_detect_batch_dev -- there every camera gets its own cutoff).  CLC_SELECT_STRONGEST costs one more launch between the detector's two
 * and no synchronisation.  CLC_ERR_BAD_ARG for an unknown mode or a NULL context, CLC_ERR_STATE for a context without detector options. */
int clc_detect_set_selection(clc_ctx* ctx, int mode);
/* The context's current rule; negative for a NULL context. */
int clc_detect_selection(const clc_ctx* ctx);
int clc_detect(clc_ctx* ctx, clc_keypoint* h_kps, int capacity, int* n_written, int* n_found);
/* Device-resident: keypoints stay in the context (clc_detect_buffers), nothing is copied back. */
int clc_detect_dev(clc_ctx* ctx, void* stream);
/* Device addresses of the context's keypoint array, of its uint32 count pair {written, found} and
 * of its descriptor array (valid for the context's lifetime). */
int clc_detect_buffers(clc_ctx* ctx, const clc_keypoint** d_kps, const uint32_t** d_count, void** d_desc);
/* CLATCH over the context's own keypoints with the count taken from device memory; writes
 * descriptors to d_desc (NULL = the context's descriptor array). */
int clc_describe_detected_dev(clc_ctx* ctx, void* d_desc, void* stream);
/* Whole front end on host buffers, like GPUDetector::detectAndDescribe (GPUDetector.hpp:216-291):
 * upload image -> pyramid -> detect -> describe -> download keypoints + descriptors. */
int clc_detect_and_describe(clc_ctx* ctx, const uint8_t* h_img, uint32_t width, uint32_t height,
                            clc_keypoint* h_kps, uint8_t* h_desc, int capacity, int* n_written, int* n_found);
/* The same without the copies out: *h_kps / *h_desc point into the context's pinned staging block (valid until the next call of this
 * family on the context), *n_written keypoints / rows of 64 B.  ONE enqueue sequence and ONE stream synchronisation per frame: image
 * into pinned memory -> DMA upload -> pyramid -> detector -> CLATCH -> one small launch that mirrors the count, the keypoints and the
 * descriptors that were found into the pinned block (the reference: 7 level downloads each with a synchronisation, two uploads, a
 * download, a device synchronisation, GPUDetector.hpp:262-290). */
int clc_detect_and_describe_view(clc_ctx* ctx, const uint8_t* h_img, uint32_t width, uint32_t height, const clc_keypoint** h_kps,
                                 const uint8_t** h_desc, int* n_written, int* n_found);
/* The frame's ONE copy of its descriptors into the caller's block (regions[idx]->Descriptors(), GPUDetector.hpp:181): copies the first n
 * rows staged by the last clc_detect_and_describe* call to h_dst and -- when n is all of them and the context's cache mode is not OFF --
 * publishes h_dst (see clc_desc_cache_mode): the rows are on the device already, the fold is taken during the copy. */
int clc_detect_store_descriptors(clc_ctx* ctx, void* h_dst, int n, clc_desc_handle* handle /* nullable */);

/* The device-resident front end for the frames of n_images <= CLC_MAX_BATCH cameras at once (GPUDetector::detectAndDescribe,
 * GPUDetector.hpp:216-291, once per drone in ColoC::processImages, coloc.hpp:150-163): ONE pyramid launch, TWO detector launches (three
 * under CLC_SELECT_STRONGEST)
 * and -- when d_desc is not NULL -- ONE CLATCH launch for all of them, nothing synchronised, nothing copied back.  d_imgs[b]: u8
 * width x height device image (pitch bytes per row, the DetectorOptions size); d_kps[b]: room for DetectorOptions.maxkp keypoints;
 * d_counts[b]: uint32[2] on the device, {written, found}; d_desc[b]: maxkp x 64 B (rows past the count are left alone).  Same
 * keypoints, order and descriptors as n_images times clc_pyramid_build_dev + clc_detect_dev + clc_describe_detected_dev.  The
 * pointer arrays themselves are host memory.  Afterwards camera 0's pyramid is the context's current one. */
int clc_detect_batch_dev(clc_ctx* ctx, int n_images, const void* const* d_imgs, uint32_t width, uint32_t height, size_t pitch,
                         clc_keypoint* const* d_kps, uint32_t* const* d_counts, void* const* d_desc, void* stream);

/* ---- describe: replaces CLATCH() (CLATCH.h:168) + GPUDetector.hpp:280-290 ------------------ */

/* n keypoints on the current pyramid -> n x 64 B descriptors. */
int clc_describe(clc_ctx* ctx, const clc_keypoint* h_kps, int n, uint8_t* h_desc);
int clc_describe_dev(clc_ctx* ctx, const clc_keypoint* d_kps, int n, void* d_desc, void* stream);
/* A host that owns several cameras on one GPU (BASELINE configs 2-3: ColoC::processImages walks the drones one
 * by one, coloc.hpp:150-163) hands over the frames of all n_images <= CLC_MAX_BATCH cameras at once: ONE pyramid
 * launch and ONE CLATCH launch for all of them instead of one pair per camera -- same results as n_images times
 * clc_pyramid_build_dev + clc_describe_dev.  d_imgs[b]: u8 width x height device image (pitch bytes per row, the
 * DetectorOptions size); d_kps[b] / counts[b]: that camera's keypoints; d_desc[b]: counts[b] x 64 B out.  The
 * pointer arrays themselves are host memory.  Afterwards camera 0's pyramid is the context's current one. */
int clc_describe_batch_dev(clc_ctx* ctx, int n_images, const void* const* d_imgs, uint32_t width, uint32_t height,
                           size_t pitch, const clc_keypoint* const* d_kps, const int* counts, void* const* d_desc,
                           void* stream);
/* {scale*x, scale*y, 7*scale, angle}, scale = pow(1.2f, level): GPUDetector.hpp:172-179. */
int clc_keypoints_to_features(const clc_keypoint* h_kps, int n, float* h_feat4);

/* ---- match: replaces CUDAK2NN() (CUDAK2NN.h:54) + GPUMatcher.hpp:180-226 -------------------- */

/* For each query the best train index if (second_best - best > (uint8_t)threshold), else -1
 * (CUDAK2NN.cu:75; the kernel's threshold parameter is uint8_t, :46, so the int is truncated).
 * Ties for the minimum keep the lowest train index.  nt == 0 gives -1 everywhere (undefined in
 * the reference).  h_best / h_second (nullable) receive the two distances saturated to 65535
 * (the reference's 100000 / 200000 "none" sentinels read as 65535). */
int clc_match_2nn(clc_ctx* ctx, const void* h_q, int nq, const void* h_t, int nt, int threshold,
                  int32_t* h_match, uint16_t* h_best, uint16_t* h_second);
/* Detector -> matcher hand-over without a second upload.  The reference passes descriptors between the two through host memory
 * (FeatureMap regions, GPUDetector.hpp:181 -> GPUMatcher.hpp:188-196) and uploads them again in every match call.  Here the front end
 * keeps a frame's descriptors in a device block of a process-wide, per-device table; when the host stores the rows at a host address it
 * PUBLISHES that fact (clc_detect_store_descriptors does both; clc_desc_cache_publish for rows copied by the caller, d_src = where they
 * lie on the device, NULL = the frame this context staged last), and clc_match_2nn / clc_match_map / clc_match_pairs given that ADDRESS
 * and COUNT read the rows where they already are -- as far as the looking-up context's mode allows:
 *   CLC_DESC_CACHE_VERIFY (default, the policy classes included): optimistic and checked -- the sweep starts on the device rows at once,
 *       and while it runs the host folds ALL rows of the block it was handed (64-bit position-keyed fold) and compares with the fold
 *       taken when the block was published; a block edited anywhere since is uploaded and the sweep repeated.  Edited host rows are
 *       never matched stale; an unchanged block costs no upload and no extra latency (the fold hides behind the sweep);
 *   CLC_DESC_CACHE_TRUST: address, count, generation and 18 sampled rows; the caller STATES that it does not edit published blocks in
 *       place (opt-in: HIPMatcher::trustPublishedRegions(true));
 *   CLC_DESC_CACHE_OFF: every block is uploaded, like the reference (GPUMatcher.hpp:188-196); the front end publishes nothing.
 * A block published by a TRUST context carries no fold and is invisible to VERIFY lookups.  Up to 32 blocks, least recently used
 * replaced; CLC_DESC_CACHE=0|verify|trust in the environment sets the mode contexts start with.
 * The fold proves only that the host rows have not changed SINCE the publication, never that the device rows equal them: publishing
 * must put the caller's exact rows on the device.  clc_desc_cache_publish(ctx, d_src, h_desc, n, handle):
 *   d_src != NULL: the caller states that d_src holds the n rows of h_desc.  The copy runs on the context's stream: rows written on
 *       another stream must be complete, or that stream joined to the context's, before the call;
 *   d_src == NULL: the rows of this context's LAST describing call, and only those --
 *     - after clc_detect_and_describe(_view): the staged frame.  n must be <= its row count and the n host rows must equal its first
 *       n rows (compared), else CLC_ERR_STATE;
 *     - after clc_describe (n rows), or clc_describe_detected_dev / clc_describe_dev with the context's own array as the target (the
 *       detected count / the given n): the context's array.  More rows than that is CLC_ERR_BAD_ARG (a clc_detect* since then makes
 *       the detected count another list's, and leaves nothing to publish);
 *     - after a describing call into caller buffers (clc_describe_detected_dev / clc_describe_dev with another target,
 *       clc_detect_batch_dev with d_desc, clc_describe_batch_dev, clc_describe_match_pair_dev) or a failed one: CLC_ERR_STATE.  Such a
 *       call also ends the staged frame, so clc_detect_store_descriptors then fails with CLC_ERR_STATE too.
 *   On every error nothing is published and *handle is zeroed.  Mode CLC_DESC_CACHE_OFF publishes nothing and returns CLC_OK. */
enum { CLC_DESC_CACHE_OFF = 0, CLC_DESC_CACHE_VERIFY = 1, CLC_DESC_CACHE_TRUST = 2 };
int clc_desc_cache_mode(clc_ctx* ctx, int mode);
int clc_desc_cache_publish(clc_ctx* ctx, const void* d_src, const void* h_desc, int n, clc_desc_handle* handle /* nullable */);
int clc_desc_handle_live(const clc_desc_handle* handle);
int clc_desc_cache_clear(void);
/* lookups of the host-pointer match entry points answered from the cache / uploaded, since the process started */
int clc_desc_cache_stats(unsigned long long* hits, unsigned long long* misses);
/* Device-resident form; d_q / d_t must be 16-byte aligned. */
int clc_match_2nn_dev(clc_ctx* ctx, const void* d_q, int nq, const void* d_t, int nt,
                      int threshold, int32_t* d_match, void* stream);
/* Describe both cameras of a pair and match them as ONE step: replaces detectAndDescribe of each camera (GPUDetector.hpp:216-291)
 * followed by computeMatchesPair (GPUMatcher.hpp:165-172 -> :180-226).  Camera 0 is the query side (regions[pair.first]), camera 1 the
 * train side; d_desc[b] receives counts[b] x 64 B, d_match counts[0] indices into camera 1 (or -1), exactly what clc_describe_batch_dev +
 * clc_match_2nn_dev give: one pyramid launch, one CLATCH launch (train camera dispatched first), one sweep launch on the caller's stream.
 * What overlaps describe and sweep on MI355X is two contexts on two streams taking alternate steps (bench.py's headline loop), not a
 * split inside one step (profiles/r05_step_overlap.txt).  Enqueue only; capturable.  16-byte aligned descriptor pointers. */
int clc_describe_match_pair_dev(clc_ctx* ctx, const void* const* d_imgs, uint32_t width, uint32_t height, size_t pitch,
                                const clc_keypoint* const* d_kps, const int* counts, void* const* d_desc, int threshold,
                                int32_t* d_match, void* stream);
/* Many (query-slice, train-set) jobs over one descriptor arena in ONE sweep launch: the
 * all-pairs loop of GPUMatcher::computeMatches (GPUMatcher.hpp:143-155) and the per-rank share
 * of it after the multi-GPU all-gather.  h_jobs is host memory. */
int clc_match_jobs_dev(clc_ctx* ctx, const void* d_desc_base, const clc_match_job* h_jobs,
                       int njobs, int32_t* d_match, void* stream);
/* The same with the row counts of the two sets of every job living in DEVICE memory (the sweep reads them; no host
 * round trip between whatever produced the counts and this call): job j's nq / nt are the PLANNED sizes (grid and result
 * layout), its query slice starts at row q_row0[j] of a set with *d_cnt_q[j] valid rows, its train set has
 * min(nt, *d_cnt_t[j]) rows.  Planned query rows past the count are answered -1. */
int clc_match_jobs_counted_dev(clc_ctx* ctx, const void* d_desc_base, const clc_match_job* h_jobs, int njobs,
                               const int32_t* const* d_cnt_q, const int32_t* const* d_cnt_t, const uint32_t* q_row0,
                               int32_t* d_match, void* stream);

/* Which formulation of the all-pairs sweep a context uses (same results bit for bit, same workspace):
 * CLC_K2NN_MATRIX (default): bits as +-1 FP4 values on the matrix pipe, exact distances in the fp32 accumulator;
 * CLC_K2NN_POPCOUNT: xor + popcount on the vector ALU, the literal form of CUDAK2NN.cu:58-66 (kept for A/B timing).
 * Also settable at context creation through the environment, CLC_K2NN_FORMULATION=matrix|popcount. */
enum { CLC_K2NN_MATRIX = 0, CLC_K2NN_POPCOUNT = 1 };
int clc_k2nn_set_formulation(clc_ctx* ctx, int formulation);
/* Queries per sweep workgroup of the context's formulation: the grain on which a caller that deals query slices out
 * to several GPUs (clc_match_job.q_offset / nq) should cut them, so that no workgroup is split between two jobs. */
int clc_k2nn_queries_per_block(const clc_ctx* ctx);
/* How the context would cut ONE nq x nt pair into sweep workgroups (planning only, nothing is launched): info[0] query blocks, [1] train
 * splits per query block, [2] train rows per equal split, [3] 1 = splits folded in-launch (atomic top-2 rows), 0 = slabs + merge kernel,
 * [4], [5] train TILES (32 rows) of a split on wave slot 0 / 1 when the pair runs as one round with unequal shares by wave slot
 * (0 = equal shares; round 4, k2nn.hip), [6] queries per workgroup, [7] workgroups aimed at per launch.  The reference has no such
 * entry (its grid is ((num_q - 1) >> 8) + 1 blocks, CUDAK2NN.cu:79); tests and bench.py report the plan with it. */
int clc_k2nn_plan_query(const clc_ctx* ctx, int nq, int nt, int32_t* info);
/* What the sweep planner knows about the context's device and which unequal shares it uses (round 5): info[0] XCDs
 * (hipDeviceAttributeNumberOfXccs), [1] CUs, [2] the formulation's default workgroups per launch (3 per CU: one resident round of the
 * matrix sweep), [3], [4] share of a slot-0 / slot-1 workgroup in 1/256 of the equal share, [5] where that pair comes from: 0 built-in
 * default, 1 CLC_K2NN_BIAS, 2 a timed probe of four candidate pairs on this device (once per process and device, at the first matcher
 * context's creation; CLC_K2NN_PROBE=0 skips it), [6] XCDs the sweep kernel's workgroup map is compiled for, [7] CLC_K2NN_TARGET_BLOCKS
 * (0: unset).  probe_us (nullable, 4 floats): the 10k x 10k sweep's time under the candidates 295:264, 311:256, 326:249, 326:233. */
int clc_k2nn_device_info(const clc_ctx* ctx, int32_t* info, float* probe_us);

/* Measurement aid (replaces nothing in the reference): runs ONE sweep of d_q x d_t with the diagnostic build of the
 * matrix-formulation kernel, whose workgroups bracket their tile loop with the shader-clock and the constant 100 MHz
 * real-time counters, and returns the clock the chip actually held inside the kernel (median / min / max over the
 * workgroups, GHz).  Call it straight after a sustained run: peaks quoted at 2.4 GHz are only reached if this says so.
 * The results in d_match are the normal ones (threshold 40). */
int clc_k2nn_clock_check(clc_ctx* ctx, const void* d_q, int nq, const void* d_t, int nt, int32_t* d_match, void* stream,
                         double* ghz_median, double* ghz_min, double* ghz_max, int* workgroups);

/* The all-pairs loop of GPUMatcher::computeMatches (GPUMatcher.hpp:143-155) on host buffers: uploads
 * each camera's descriptors once (the reference re-uploads both sides for every pair,
 * GPUMatcher.hpp:188-196), sweeps every listed (first, second) pair in one launch group (Q = first,
 * T = second) and downloads one int32 array of counts[first] entries per pair into h_match[p]. */
int clc_match_pairs(clc_ctx* ctx, const void* const* h_desc, const int* counts, int ncams,
                    const int* pairs /* npairs x {first, second} */, int npairs, int threshold,
                    int32_t* const* h_match);

/* Map database: GPUMatcher::setMapData (GPUMatcher.hpp:110-117) / matchFeaturesWithMap (:252-271). */
int clc_set_map(clc_ctx* ctx, const void* h_desc, int n);
int clc_match_map(clc_ctx* ctx, const void* h_q, int nq, int threshold, int32_t* h_match);
/* The same against descriptors that are still on the GPU (clc_describe*_dev output): enqueue only; d_match[i] = map
 * index or -1.  In a streaming loop the frame's descriptors then never leave the device, only the nq x 4 B result does. */
int clc_match_map_dev(clc_ctx* ctx, const void* d_q, int nq, int threshold, int32_t* d_match, void* stream);

/* ---- match, distance-ratio rule: replaces CPUMatcher<T> (include/coloc/CPUMatcher.hpp:22-102), the matcher of every non-CUDA build
 * (coloc.hpp:66-68), whose calls all go through openMVG::matching::DistanceRatioMatch(ratio, BRUTE_FORCE_HAMMING, database, queries).
 * Rule, per query: the two smallest Hamming distances d1 <= d2 over all database rows (the same exact sweep as the K2NN entries);
 * accept iff the database holds at least two rows and (float)d1 < r2 * (float)d2 with r2 = ratio * ratio rounded to float.  Ties for the
 * minimum (d1 == d2) therefore never pass for ratio <= 1; for ratio > 1 they give the lowest database index.  Fewer than two database
 * rows (nt < 2): no match.  ratio must be finite and > 0 (else CLC_ERR_BAD_ARG); MatcherOptions.distRatio is not read -- CPUMatcher
 * ignores its options and passes its own constants.
 * Per-query entries: the same orientation and outputs as clc_match_2nn / clc_match_2nn_dev / clc_match_map_dev (h_match[q] = database
 * index or -1; h_best / h_second unchanged), the same descriptor-cache resolution of host blocks.
 * Pair entries: CPUMatcher's IndMatch lists.  IndMatch(i_ = database row, j_ = query row), two int32 per match; per pair then
 *   - with positions (xy = count x 2 floats per set): exact duplicate pairs dropped, and matches whose (x_I, y_I, x_J, y_J) repeat an
 *     earlier one dropped; ordered by (x_I, y_I, x_J, y_J, i_, j_);
 *   - without positions: identical pairs dropped only; ordered by (i_, j_), the order IndMatch::getDeduplicated leaves.
 *   That order and the position pass are this project's statement of recalled OpenMVG behaviour (OpenMVG is not available to pin it
 *   against; the CPU oracle orc_cpumatcher_pair states the same).  Positions for one side only: CLC_ERR_BAD_ARG; a NaN position too.
 *   A set without rows needs no positions (NULL is fine): a pair with an empty side has no match.
 *   Capacity of a pair list: one match per query row.  De-duplication runs on the host, O(k log k) over the k accepted matches. */
int clc_match_ratio_2nn(clc_ctx* ctx, const void* h_q, int nq, const void* h_t, int nt, float ratio,
                        int32_t* h_match, uint16_t* h_best, uint16_t* h_second);
/* Enqueue only, on `stream`; 16-byte aligned descriptor pointers, like clc_match_2nn_dev. */
int clc_match_ratio_2nn_dev(clc_ctx* ctx, const void* d_q, int nq, const void* d_t, int nt, float ratio, int32_t* d_match, void* stream);
/* CPUMatcher::computeMatches / computeMatchesPair (CPUMatcher.hpp:37-76) over host blocks: DATABASE = camera pairs[p].first, QUERIES =
 * camera pairs[p].second -- the opposite of clc_match_pairs.  Each camera uploaded (or found published) once, all pairs in one launch
 * group.  h_xy (nullable; else one pointer per camera, counts[c] x 2 floats) selects the position pass
 * (h_xy[c] may be NULL for a camera with counts[c] == 0).  h_pairs_out[p] receives n_out[p]
 * (i_, j_) pairs, capacity 2 x counts[pairs[p].second] int32. */
int clc_match_ratio_pairs(clc_ctx* ctx, const void* const* h_desc, const int* counts, int ncams, const float* const* h_xy,
                          const int* pairs /* npairs x {first = database, second = queries} */, int npairs, float ratio,
                          int32_t* const* h_pairs_out, int* n_out);
/* CPUMatcher::matchSceneWithMap (CPUMatcher.hpp:78-97): the map of clc_set_map is the database, IndMatch(i_ = map row, j_ = query row).
 * xy_map (map_n x 2) and xy_q (nq x 2) both given or both NULL (either may be NULL when its set is empty); h_pairs capacity 2 x nq int32. */
int clc_match_map_ratio(clc_ctx* ctx, const void* h_q, int nq, const float* xy_map, const float* xy_q, float ratio,
                        int32_t* h_pairs, int* n_out);
/* Per query against the map, enqueue only: d_match[q] = map row or -1 (no de-duplication). */
int clc_match_map_ratio_dev(clc_ctx* ctx, const void* d_q, int nq, float ratio, int32_t* d_match, void* stream);
/* Host arithmetic only (ctx not needed, no GPU): per-query ratio results match[nq] (database row or -1) -> the de-duplicated, ordered
 * pair list above; xy_db indexed by match[q], xy_q by q (both or neither; either may be NULL when nq == 0).  pairs capacity 2 x nq int32.  The code the two host pair
 * entries use. */
int clc_ratio_matches_to_pairs(const int32_t* match, int nq, const float* xy_db, const float* xy_q, int32_t* pairs, int* n);

/* ---- pose scoring: the data-parallel core of SfM_Localizer::Localize (Localizer.hpp:82-93) --- */

/* err[h*N+i] = || x_i - hnormalized(K (R_h X_i + t_h)) ||^2, fp64.
 * h_Rt: H x 12 row-major [R|t]; h_X: N x 3; h_x: N x 2; h_K: 9 row-major. */
int clc_pnp_residuals(clc_ctx* ctx, const double* h_Rt, int H, const double* h_X,
                      const double* h_x, int N, const double* h_K, double* h_err);
/* Fused scoring without materialising the H x N matrix: per hypothesis the inlier count
 * (err < thr2) and the truncated cost sum_i min(err, thr2).  Outputs nullable. */
int clc_pnp_score(clc_ctx* ctx, const double* h_Rt, int H, const double* h_X, const double* h_x,
                  int N, const double* h_K, double thr2, int32_t* h_count, double* h_cost);

/* ---- two-view scoring: the data-parallel core of RobustMatcher::filterEssential -------------------
 * (RobustMatcher.hpp:153-186: AC-RANSAC over FivePointSolver + SymmetricEpipolarDistanceError.)
 * h_F: H x 9 row-major FUNDAMENTAL matrices (F = K2^-T E K1^-1); h_x1 / h_x2: N x 2 pixel points of the
 * two views.  err[h*N+i] = (x2^T F x1)^2 (1/|(F x1)_xy|^2 + 1/|(F^T x2)_xy|^2) / 4, fp64.  The minimal
 * solver stays with the caller (OpenMVG's, when linked in): generate all hypotheses, score once. */
int clc_epipolar_residuals(clc_ctx* ctx, const double* h_F, int H, const double* h_x1, const double* h_x2,
                           int N, double* h_err);
int clc_epipolar_score(clc_ctx* ctx, const double* h_F, int H, const double* h_x1, const double* h_x2, int N,
                       double thr2, int32_t* h_count, double* h_cost);

/* Essential-matrix RANSAC on the GPU -- the role of RobustMatcher::filterEssential (RobustMatcher.hpp:153-186:
 * ACRANSAC over essential::kernel::FivePointSolver + SymmetricEpipolarDistanceError): S minimal samples of 5
 * correspondences -> one five-point problem per lane (<= 10 essential matrices each, csrc/fivept.h) -> all
 * 10 S hypotheses scored over all N pixel correspondences (F = K2^-T E K1^-1) -> best = most inliers
 * (err < thr2), then lowest truncated cost, then lowest index -> inlier mask.  h_samples: S x 5 indices
 * (NULL = drawn from a xorshift64* stream seeded with `seed`).  Outputs (nullable): h_E, h_F 9 doubles
 * row-major, h_inlier_mask N bytes, *n_inliers (0 = no model).  OpenMVG's a-contrario threshold selection and
 * its solver's root order are unpinned (absent submodule). */
int clc_essential_ransac(clc_ctx* ctx, const double* h_x1, const double* h_x2, int N, const double* h_K1,
                         const double* h_K2, const int32_t* h_samples, int S, uint64_t seed, double thr2,
                         double* h_E, double* h_F, uint8_t* h_inlier_mask, int* n_inliers);
/* The five-point hypotheses alone: h_E_out receives S x 10 x 9 doubles (NaN = no solution). */
int clc_essential_fivepoint(clc_ctx* ctx, const double* h_x1, const double* h_x2, int N, const double* h_K1,
                            const double* h_K2, const int32_t* h_samples, int S, double* h_E_out);

/* Whole robust pose solve on the GPU -- the role of SfM_Localizer::Localize(P3P, max_iteration = 256)
 * at Localizer.hpp:82-93: S minimal samples -> one P3P problem per lane (<= 4 poses each) -> all
 * 4 S hypotheses scored over all N correspondences in one launch -> best = most inliers (err < thr2),
 * then lowest truncated cost, then lowest index -> its inlier mask.  h_samples: S x 3 point indices
 * (NULL = drawn from a xorshift64* stream seeded with `seed`; OpenMVG draws from std::mt19937 and
 * scores a contrario -- unpinned).  Outputs: h_Rt 12 doubles row-major [R|t],
 * h_inlier_mask N bytes (nullable), *n_inliers, *cost (nullable).  *n_inliers == 0 means no pose. */
int clc_pnp_ransac(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K,
                   const int32_t* h_samples, int S, uint64_t seed, double thr2, double* h_Rt,
                   uint8_t* h_inlier_mask, int* n_inliers, double* cost);
/* Single-pose refinement + covariance -- the role of Localizer::refine -> PoseRefiner::refinePose
 * (Localizer.hpp:110-177, Refiner.hpp:47-239; Ceres LM, HuberLoss(Square(4.0)), structure and intrinsics
 * fixed): Levenberg-Marquardt on 1/2 sum rho(||obs - proj||^2) over the 6 parameters [angle-axis | t],
 * from the initial pose h_Rt_in, using the correspondences with h_inlier_mask[i] != 0 (NULL = all).
 * Outputs (all nullable): h_Rt_out 12 doubles, h_cov 36 doubles = (J^T W J)^-1 in the [angle-axis | t]
 * parametrisation (row-major), *rmse = sqrt(final_cost / (2 n_used)) (Refiner.hpp:226), *iterations.
 * huber_a <= 0 selects the reference's 16.  Ceres is absent here, so results are defined by this
 * cost, not by Ceres' iterates (unpinned).
 * h_K, here and in clc_pnp_ransac / clc_pnp_localize / clc_pnp_p3p / clc_pnp_acransac / clc_pnp_localize_ac(_batch), must be
 * { fx, skew, cx; 0, fy, cy; 0, 0, 1 } exactly: any other K (a scaled one, K[3] != 0) is CLC_ERR_BAD_ARG. */
int clc_pnp_refine(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K,
                   const uint8_t* h_inlier_mask, const double* h_Rt_in, double huber_a, int max_iter,
                   double* h_Rt_out, double* h_cov, double* rmse, int* iterations);

/* clc_pnp_ransac followed by clc_pnp_refine on its inliers as ONE submission (one upload, chained
 * kernels, one download): what Localizer::localizeImage does end to end (Localizer.hpp:77-108).
 * Outputs nullable; *n_inliers == 0 means no pose (h_Rt / h_cov are zero then). */
int clc_pnp_localize(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K,
                     const int32_t* h_samples, int S, uint64_t seed, double thr2, double huber_a,
                     double* h_Rt, double* h_cov, uint8_t* h_inlier_mask, int* n_inliers, double* rmse);

/* The hypotheses of the minimal solver alone: h_Rt_out receives 4 S x 12 doubles (NaN = no solution). */
int clc_pnp_p3p(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K,
                const int32_t* h_samples, int S, double* h_Rt_out);

/* ---- several cameras on several GPUs (no counterpart in the reference) ------------------------------------------------
 * The reference matches its cameras in a serial all-pairs loop inside one process (GPUMatcher::computeMatches,
 * GPUMatcher.hpp:143-155 over Utils::handlePairs, colocUtils.hpp:58-61).  Here: one process (and context) per GPU, rank r
 * owns camera r; clc_mc_gather_dev exchanges the descriptor blocks over xGMI, clc_mc_match_dev sweeps this rank's
 * contiguous share of the flattened (pair, query block) sequence; the union over the ranks is exactly the serial loop's
 * per-pair result (Q = descriptors of `first`, T = of `second`).  RCCL is loaded at run time (dlopen), only when
 * world > 1.  Exchange forms: CLC_MC_RCCL = ncclAllGather of the fixed-capacity blocks; CLC_MC_PEER_COPY = every rank
 * copies its block into each peer's arena through IPC-mapped pointers (one xGMI hop each) and a 4-byte all-gather of
 * the counts acts as the fence. */
#define CLC_MC_ID_BYTES 128
enum { CLC_MC_RCCL = 0, CLC_MC_PEER_COPY = 1 };
typedef struct clc_mc clc_mc;
/* one contiguous run of query rows of pair (first, second) assigned to a rank */
typedef struct clc_mc_share {
    int32_t  first, second;  /* camera ids, first < second                                  */
    uint32_t q_begin, nq;    /* query rows [q_begin, q_begin + nq) of camera `first`         */
    uint32_t out_offset;     /* first int32 of this run inside the rank-local result buffer */
} clc_mc_share;
/* Pure host arithmetic (no GPU, no context): the shares of `rank` when `world` ranks split the all-pairs work of
 * cameras with counts[c] descriptors, cut on `grain` queries (clc_k2nn_queries_per_block).  The C twin of
 * coloc_amd/multicam.py shard_pairs. */
int clc_mc_plan(const int* counts, int ncams, int world, int rank, int grain, clc_mc_share* out, int capacity, int* n_out);
/* Rank 0 creates the rendezvous id; the HOST application hands it to the other ranks (MPI, a socket, a file ...). */
int clc_mc_unique_id(uint8_t id[CLC_MC_ID_BYTES]);
/* Joins the `world`-rank group on ctx's device; maxkp = capacity of a camera's descriptor block (the same on all
 * ranks).  world == 1 needs no id and no RCCL (with an id it builds a one-rank communicator and every exchange goes
 * through the same RCCL / IPC calls as world > 1).  world > 1 with id == NULL creates a REHEARSAL handle without a
 * communicator: the calling process plays the other ranks with clc_mc_virtual_put (how the one-GPU tests drive every
 * rank's share through this entry); clc_mc_gather_dev then only files the rank's own block. */
int clc_mc_create(clc_ctx* ctx, const uint8_t id[CLC_MC_ID_BYTES], int world, int rank, int maxkp, clc_mc** out);
int clc_mc_virtual_put(clc_mc* mc, int other_rank, const void* d_desc, int count, void* stream);
/* Collective over the group (every rank calls it): exchanges the arenas' IPC handles through the communicator and maps the peers'
 * arenas, which the first CLC_MC_PEER_COPY exchange would otherwise do.  Calling it up front lets a host learn that the mapping is
 * not possible on this machine (status != CLC_OK) BEFORE any rank waits in an exchange. */
int clc_mc_open_peers(clc_mc* mc, void* stream);
int clc_mc_destroy(clc_mc* mc);
const char* clc_mc_last_error_string(const clc_mc* mc);
/* The arena [world][maxkp][64 B] the LAST exchange filled (one of the handle's two buffers: it alternates per exchange). */
int clc_mc_arena(const clc_mc* mc, void** d_arena, int* world, int* maxkp);
/* Exchange: this rank's descriptors (d_my_desc: a device buffer of maxkp rows, my_count of them valid) go to every
 * rank's arena, the counts come back to the host (h_counts_out: world ints, nullable).  Synchronises the stream. */
int clc_mc_gather_dev(clc_mc* mc, const void* d_my_desc, int my_count, int mode, int* h_counts_out, void* stream);
/* Sweep this rank's shares of the gathered arena (enqueue only): d_match receives the runs back to back
 * (share.out_offset), h_shares the shares themselves.  Needs the counts on the host: follows clc_mc_gather_dev. */
int clc_mc_match_dev(clc_mc* mc, int threshold, int32_t* d_match, int match_capacity, clc_mc_share* h_shares,
                     int share_capacity, int* n_shares, void* stream);
/* The same step WITHOUT a host synchronisation between the exchange and the sweep (a streaming host enqueues step after
 * step): clc_mc_gather_enqueue_dev only enqueues the exchange -- my_count from the host, or d_my_count != NULL: read on the
 * device (e.g. the detector's count, clc_detect_buffers), the whole capacity block then travels --, and
 * clc_mc_match_enqueue_dev cuts the shares on the block CAPACITY (identical for every step of a handle) and lets the sweep
 * read the gathered counts from device memory: planned query rows past a camera's count are answered -1, train rows past
 * it are not swept.  Per pair and valid row the result is the serial loop's.  clc_mc_counts synchronises the stream and
 * returns the counts of the last exchange.
 * Ordering contract (both gather forms): the arena is double-buffered by step parity, every rank calls the gather the same
 * number of times, and a rank enqueues step k + 1's exchange on the stream that holds its step-k sweep; then no peer copy
 * lands in a buffer a sweep still reads (coloc_amd/csrc/multicam.hip, top). */
int clc_mc_gather_enqueue_dev(clc_mc* mc, const void* d_my_desc, int my_count, const int32_t* d_my_count, int mode, void* stream);
int clc_mc_match_enqueue_dev(clc_mc* mc, int threshold, int32_t* d_match, int match_capacity, clc_mc_share* h_shares,
                             int share_capacity, int* n_shares, void* stream);
int clc_mc_counts(clc_mc* mc, int* h_counts_out, void* stream);
/* OVERLAPPED steps (round 6; default off, call before the handle's first exchange and before clc_mc_open_peers): the caller passes one
 * stream to clc_mc_gather_enqueue_dev -- and enqueues its describe on it -- and ANOTHER to clc_mc_match_enqueue_dev; step k + 1's
 * describe + exchange then run beside step k's sweep.  The handle keeps three arena buffers and orders the two streams with events
 * (sweep k behind exchange k; exchange k behind sweep k - 2); all collectives stay on the exchange stream, so one communicator serves.
 * Results are those of the one-stream step.  The context's front-end work (pyramid, CLATCH) must be enqueued on the exchange stream and
 * nothing but the sweep on the other one: a context's matcher workspace and its detector workspace are separate. */
int clc_mc_set_overlap(clc_mc* mc, int on);
/* What RCCL itself says about the communicator behind the handle: *n_ranks = ncclCommCount, *user_rank = ncclCommUserRank
 * (*n_ranks == 0: the handle has no communicator -- one rank without an id, or a rehearsal handle). */
int clc_mc_comm_info(const clc_mc* mc, int* n_ranks, int* user_rank);

/* ---- a-contrario model selection: what the reference actually runs ------------------------------------------------------
 * Localizer::localizeImage calls SfM_Localizer::Localize(P3P_KE_CVPR17, ..., {error_max = +inf, max_iteration = 256})
 * (include/coloc/Localizer.hpp:82-93) and RobustMatcher::filterEssential calls robust::ACRANSAC over the five-point
 * kernel with precision +inf (include/coloc/RobustMatcher.hpp:153-171): OpenMVG's AC-RANSAC, which needs NO threshold --
 * per model it sorts the residuals, evaluates the number of false alarms NFA(k) of "the k best are inliers" for every k
 * and keeps the model / k of lowest NFA; after the first meaningful model (NFA < 0) the reserved 10 % of the iterations
 * sample among its inliers.  (Moisan, Moulon, Monasse, IPOL 2012; OpenMVG itself is an empty submodule in the reference
 * tree, so its RNG stream and solver root order are unpinned: samples here are a documented pure function of
 * (seed, iteration, index set), coloc_amd/csrc/clc_acr.h.)  Batches of iterations are evaluated per round on the GPU --
 * minimal solves, one sort + NFA scan per model in LDS, a sequential-semantics selection -- with results identical to
 * the iteration-by-iteration loop (oracle/clc_oracle_acr.c).  precision = INFINITY is the reference's setting; a finite
 * value is OpenMVG's upper bound on the inlier residual, in pixels^2.  At most 16384 correspondences per solve (CLC_ERR_CAPACITY beyond: the per-model sort runs in one workgroup's LDS).
 *
 * clc_pnp_acransac: h_X N x 3, h_x N x 2 UNDISTORTED pixels, h_K 9 row-major (fx = K[0] scales residuals to the
 * normalised camera plane as ACKernelAdaptorResection_Intrinsics does).  Outputs (nullable): h_Rt 12 doubles [R|t],
 * h_inlier_mask N bytes, h_inliers the inlier indices in ascending residual order (capacity N; vec_inliers),
 * *n_inliers (0 = no meaningful model; the caller applies Localize's "> 2.5 x 3" test), *error_max the precision found
 * in pixels (ACRansacOut.first), *min_nfa the log10 NFA (ACRansacOut.second), *iterations actually run. */
int clc_pnp_acransac(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, int max_iteration,
                     uint64_t seed, double precision, double* h_Rt, uint8_t* h_inlier_mask, int32_t* h_inliers,
                     int* n_inliers, double* error_max, double* min_nfa, int* iterations);
/* The same followed by clc_pnp_refine on the inliers in one submission: Localizer::localizeImage end to end
 * (Localizer.hpp:77-108).  h_cov 36 doubles, *rmse as clc_pnp_refine. */
int clc_pnp_localize_ac(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, int max_iteration,
                        uint64_t seed, double precision, double huber_a, double* h_Rt, double* h_cov,
                        uint8_t* h_inlier_mask, int32_t* h_inliers, int* n_inliers, double* error_max, double* rmse);
/* Several independent localisations at once -- BASELINE config[2]'s "batched PnP/RANSAC pose", one per camera: job i is what
 * clc_pnp_acransac (refine == 0) or clc_pnp_localize_ac (refine != 0) does, on ctxs[i] (every job needs a context of its own; contexts created
 * without detector and matcher options are enough).  A solve is a chain of short launches with the host in the loop and leaves the GPU idle
 * most of the time; here ONE host thread drives all the chains, so they interleave on the device.  Every job's result is the one the
 * single-solve entry gives for the same arguments (same model, inliers, threshold, covariance, bit for bit).  jobs[i].status holds the
 * job's own status; the return value is the first failure, CLC_OK if none.
 * Since round 5 the solves of a larger batch (eight or more here, four or more two-view filters below) SHARE their launches instead --
 * round r of every unfinished solve is one launch on ctxs[0]'s stream, blockIdx.y = solve -- which changes the schedule, not a result;
 * on return the streams of all the contexts are ordered behind whatever of those launches is still in flight (CLC_ACR_LOCKSTEP=0|1
 * forces the form). */
typedef struct clc_pose_job {
    /* in */
    const double* X;          /* n x 3 world points                                      */
    const double* x;          /* n x 2 pixels                                            */
    const double* K;          /* 3 x 3 row-major                                         */
    int           n;
    int           max_iteration;
    uint64_t      seed;
    double        precision;  /* +inf: a-contrario threshold (Localizer.hpp:82-84)       */
    int           refine;     /* != 0: LM refinement + 6 x 6 covariance behind the solve */
    double        huber_a;    /* <= 0: 16                                                */
    /* out (pointers nullable) */
    double*       Rt;         /* 12                                                      */
    double*       cov;        /* 36 (refine)                                             */
    uint8_t*      inlier_mask;/* n                                                       */
    int32_t*      inliers;    /* n                                                       */
    int           n_inliers;
    int           iterations;
    int           status;
    double        error_max;
    double        rmse;       /* refine                                                  */
} clc_pose_job;
int clc_pnp_localize_ac_batch(clc_ctx* const* ctxs, clc_pose_job* jobs, int n_jobs);

/* RobustMatcher::filterEssential's ACRANSAC: h_x1 / h_x2 N x 2 undistorted pixels, K1 / K2, img_w x img_h the size of
 * image 2 (point-to-line alpha0 = 2 D / A / 2, residual^(1/2)); residual = symmetric epipolar distance of
 * F = K2^-T E K1^-1 as clc_epipolar_residuals.  *error_max is that squared distance at the a-contrario threshold. */
int clc_essential_acransac(clc_ctx* ctx, const double* h_x1, const double* h_x2, int N, const double* h_K1,
                           const double* h_K2, int img_w, int img_h, int max_iteration, uint64_t seed, double precision,
                           double* h_E, double* h_F, uint8_t* h_inlier_mask, int32_t* h_inliers, int* n_inliers,
                           double* error_max, double* min_nfa, int* iterations);

/* Several two-view filters at once (round 5): what RobustMatcher::filterMatches runs pair after pair (RobustMatcher.hpp:455-483 ->
 * filterEssential :153-171).  As clc_pnp_localize_ac_batch: one context per job (all on one device), ONE host thread drives all the solves
 * (chains of launches of their own that interleave on the device, or -- four or more jobs -- rounds in launches shared by the batch);
 * every job's result is clc_essential_acransac's for the same arguments. */
typedef struct clc_two_view_job {
    /* in */
    const double* x1;         /* n x 2 undistorted pixels, image 1                        */
    const double* x2;         /* n x 2, image 2                                           */
    const double* K1;         /* 3 x 3 row-major                                          */
    const double* K2;
    int           n, img_w, img_h, max_iteration;
    uint64_t      seed;
    double        precision;  /* +inf: a-contrario threshold                              */
    /* out (pointers nullable) */
    double*       E;          /* 9                                                        */
    double*       F;          /* 9                                                        */
    uint8_t*      inlier_mask;/* n                                                        */
    int32_t*      inliers;    /* n                                                        */
    int           n_inliers, iterations, status;
    double        error_max, min_nfa;
} clc_two_view_job;
int clc_essential_acransac_batch(clc_ctx* const* ctxs, clc_two_view_job* jobs, int n_jobs);

/* The same a-contrario filter under RobustMatcher's other two models (ABI 4; RobustMatcher.hpp:399-405 dispatches on colocParams::model):
 *   CLC_MODEL_FUNDAMENTAL 'F'  filterFundamental :128-151  ACKernelAdaptor<SevenPointSolver, EpipolarDistanceError, UnnormalizerT>(.., true)
 *   CLC_MODEL_HOMOGRAPHY  'H'  filterHomography  :188-239  ACKernelAdaptor<FourPointSolver, AsymmetricError, UnnormalizerI>(.., false)
 *   CLC_MODEL_ESSENTIAL   'E'  = clc_essential_acransac (h_M = E, h_F = F)
 * h_x1 / h_x2: N x 2 pixels; both images img_w x img_h (the reference hands params.imageSize for both): the points are conditioned by the
 * image size, samples of 7 (4) correspondences give <= 3 (1) models, residual = squared distance to the epipolar line in image 2
 * ('F', point-to-line alpha0, residual^(1/2)) / squared transfer error ('H', point-to-point alpha0), both in conditioned coordinates.
 * h_M (9, nullable): the model brought back to PIXELS (x2^T F x1 = 0; x2 ~ H x1) -- what RelativePose_Info::essential_matrix receives;
 * h_F (9, nullable): F for 'E' and 'F', zeros for 'H'.  *error_max: the a-contrario threshold in pixels (sqrt(e) / N2(0,0)); K1 / K2
 * are read for 'E' only.  The rounds are the resection's (one launch per round: replay + seven-/four-point solve + residuals, sort, NFA). */
enum { CLC_MODEL_ESSENTIAL = 'E', CLC_MODEL_FUNDAMENTAL = 'F', CLC_MODEL_HOMOGRAPHY = 'H' };
int clc_two_view_acransac(clc_ctx* ctx, int model, const double* h_x1, const double* h_x2, int N, const double* h_K1,
                          const double* h_K2, int img_w, int img_h, int max_iteration, uint64_t seed, double precision,
                          double* h_M, double* h_F, uint8_t* h_inlier_mask, int32_t* h_inliers, int* n_inliers,
                          double* error_max, double* min_nfa, int* iterations);
/* Several filters of ONE model at once, as clc_essential_acransac_batch (which is this with 'E'): job.E receives the model matrix (E, F
 * or H), job.F the fundamental matrix ('E', 'F') or zeros ('H'); job.K1 / K2 are read for 'E' only. */
int clc_two_view_acransac_batch(clc_ctx* const* ctxs, int model, clc_two_view_job* jobs, int n_jobs);
/* The minimal solver of 'F' / 'H' on caller-chosen samples (the hypothesis generator the tests hand to the sequential oracle, as
 * clc_pnp_p3p / clc_essential_fivepoint are for the other kinds): h_samples S x 7 (4) indices into the N correspondences; h_models
 * S x 3 (1) x 9 matrices IN CONDITIONED COORDINATES, NaN-filled where a sample has fewer real roots. */
int clc_two_view_minimal(clc_ctx* ctx, int model, const double* h_x1, const double* h_x2, int N, int img_w, int img_h,
                         const int32_t* h_samples, int S, double* h_models);

/* The 3-D similarity between two landmark sets by a-contrario RANSAC (a new entry under ABI 4).  OUR OWN STATEMENT, an addition with
 * OpenMVG parity unpinned: the reference's matchMaps was meant to filter the matches between the old and the new map geometrically, its
 * homography filter is commented out (RobustMatcher.hpp:247-293) and the live code keeps every match (:348-362); the scale rule behind it
 * (colocUtils.hpp:184-211, clc_map_align_dev) averages distance ratios over all of them.  Convention: the similarity maps NEW to OLD,
 * X_old ~ s R X_new + t; a model is A = [sR | t], 12 doubles, 3 x 4 row-major.  The arithmetic is coloc_amd/csrc/sim3_math.h, one
 * statement for host and device (IEEE +, -, *, /, sqrt in a written order, no contraction):
 *   minimal solver  three correspondences.  In each cloud an orthonormal triad from p1 - p0 and (p1 - p0) x (p2 - p0); R = F_old F_new^T;
 *                   s = sqrt(S_old / S_new), S = sum |p_i - mean|^2 over the three points; t = mean_old - s R mean_new.  A sample is
 *                   degenerate when, in either cloud, |e1 x e2|^2 <= 1e-12 |e1|^2 |e2|^2: its slot is NaN-filled (an empty root).
 *   residual        |X_old - (A [X_new; 1])|^2 in old-map units, every row ((A0 X + A1 Y) + A2 Z) + A3.
 *   a-contrario     the fifth kind of the one multi-solve launch path (one launch per round, as resection): samples of 3, one model per
 *                   sample, alpha0 = ((4 / 3) pi) / V with V = (ex ey) ez the volume of the axis-aligned bounding box of the OLD points,
 *                   exponent 1.5, loge0 as for the other kinds.  A V that is not positive and finite admits no model.
 *   acceptance      a meaningful model (NFA < 0) with more than 2.5 x 3 inliers -- the rule of HIP_SfM_Localizer::Localize.
 *   refit           Umeyama's least-squares similarity over the inliers in ascending index: centroids and the 3 x 3 cross-covariance as
 *                   partial sums of 128 consecutive inliers, each left to right, the partials left to right; 3 x 3 SVD by one-sided
 *                   Jacobi (<= 30 sweeps); R = U diag(1, 1, d) V^T, d = sign(det U det V); s = (sigma1 + sigma2 + d sigma3) / (S_new / n);
 *                   t = mean_old - s R mean_new.  Refused -- the minimal model is kept, *refit = 0 -- when sigma2 <= 1e-12 sigma1 or an
 *                   output is not finite.  One single-workgroup launch behind the last round, no floating-point atomics.
 *   reported        after a refit its own s, R, t with A = [sR | t]; else s = sqrt((A00^2 + A10^2) + A20^2), R = A[:, :3] / s, t = A[:, 3].
 * h_x_new / h_x_old: N x 3.  precision: upper bound of the residual (squared old-map units), +inf: none.  Outputs (all nullable): *s,
 * h_R (9), h_t (3), h_A (12), h_inlier_mask (N), h_inliers (N, ascending residual), *n_inliers, *error_max (sqrt of the threshold
 * residual: old-map units), *min_nfa, *iterations, *valid (the iteration that gave the model, -1: none), *refit.  Not found -- N <= 3
 * (no solve runs), a degenerate box, no meaningful model or the acceptance rule failing --: s = 1, R = I, t = 0, A = [I | 0], no inliers,
 * *valid = -1; *min_nfa and *iterations are the run's.  N > 16 384: CLC_ERR_CAPACITY. */
int clc_sim3_acransac(clc_ctx* ctx, const double* h_x_new, const double* h_x_old, int N, int max_iteration, uint64_t seed,
                      double precision, double* s, double* h_R, double* h_t, double* h_A, uint8_t* h_inlier_mask, int32_t* h_inliers,
                      int* n_inliers, double* error_max, double* min_nfa, int* iterations, int* valid, int* refit);
/* The minimal solver above on caller-chosen samples (the hypothesis generator, as clc_two_view_minimal is for 'F' / 'H'): h_samples
 * S x 3 indices into the N correspondences; h_models S x 12, NaN-filled for a degenerate sample or an index outside [0, N). */
int clc_sim3_minimal(clc_ctx* ctx, const double* h_x_new, const double* h_x_old, int N, const int32_t* h_samples, int S,
                     double* h_models);

/* The inter-camera step of ColoC::interPoseEstimator(source, dest) between the pair's putative matches and the covariance intersection
 * (coloc.hpp:296-340), for several camera pairs at once: a-contrario five-point filter (filterMatchesPair, :296) -> relative pose from
 * E with the chirality vote (RobustMatcher.hpp:176-183) -> the pair's temporary map triangulated in the source camera's frame (:306) ->
 * the features it shares with the global map -> its scale against the global map through them (colocUtils.hpp:184-211) -> the
 * destination's pose through the source's, refined against the temporary map with its 6 x 6 covariance (refinePose, :340;
 * Huber(huber_a)).  tv.x1 = the SOURCE frame's features, tv.x2 = the destination's; tv.E and tv.inliers must be given.
 * The common features come, per job, from one of two places:
 *   THE REFERENCE'S CHAIN (d_first_desc, first_feature and d_map_desc given): setupMapDatabase(inter) keeps, for every point of the
 *       temporary map, the descriptor of its FIRST observation -- the pair's camera with the lower id (colocData.hpp:109-117) --, and
 *       matchMapFeatures(mapRegions, interMapRegions) matches the global map's descriptors against them: K2NN, Q = global map, T =
 *       temporary map, threshold 60 (coloc.hpp:317-323, GPUMatcher.hpp:157-163); commonFeatures = the accepted map points in ascending
 *       order.  Here: the rows are gathered on the device from that camera's descriptor block and swept against the map's block, which
 *       both stay where they are (device pointers);
 *   THE SHORTCUT (map_index given, the chain's pointers NULL): correspondence i's SOURCE feature is global map point map_index[i] (-1:
 *       none) -- what the source frame's own map tracking (matchSceneWithMap) already found; no descriptor work, common features in
 *       correspondence order.
 * stage says how far a job got. */
enum { CLC_INTER_OK = 0, CLC_INTER_NO_MODEL = 1 /* filter found < 13 inliers */, CLC_INTER_NO_RELATIVE_POSE = 2 /* < 8 points in front of both cameras */,
       CLC_INTER_NO_SCALE = 3 /* < 8 features shared with the global map */, CLC_INTER_NO_REFINEMENT = 4 };
typedef struct clc_inter_pose_job {
    clc_two_view_job tv;
    /* in */
    const int32_t* map_index; /* the shortcut: tv.n, index of correspondence i's SOURCE feature in the global map, -1 = none (nullable) */
    const double*  map_X;     /* global map points, 3 doubles each                         */
    int            map_n;     /* number of map points: an index outside [0, map_n) counts as "not a map feature" */
    const double*  Rt_source; /* 12: [R|t] of the source camera, x_cam = R X + t           */
    double         huber_a;   /* <= 0: 16                                                  */
    /* the reference's chain (all three, or none): */
    const void*    d_first_desc;   /* DEVICE: the descriptor block (rows of 64 B, 16-byte aligned) of the pair's camera with the lower id */
    const int32_t* first_feature;  /* tv.n: correspondence i's feature (row) in that block  */
    const void*    d_map_desc;     /* DEVICE: the global map's descriptors, map_n rows in map_X's order, 16-byte aligned */
    int            match_threshold;/* <= 0: 60 (GPUMatcher.hpp:162)                         */
    /* out */
    double         Rt[12];    /* the destination's pose through the source, refined        */
    double         cov[36];   /* [angle-axis | translation] order, as clc_pnp_refine       */
    double         rmse, scale;
    int            n_front, n_common, n_refined, stage;
    int            n_map_matches; /* the reference's chain: global map points matched to the temporary map (before the depth-ratio screen) */
} clc_inter_pose_job;
int clc_inter_pose_batch(clc_ctx* const* ctxs, clc_inter_pose_job* jobs, int n_jobs);

/* ---- 2D-3D tracks on the device: replaces Localizer::setupTracks (include/coloc/Localizer.hpp:59-75) ---------------------
 * The one stage of ColoC::intraPoseEstimator (coloc.hpp:201-272: matchSceneWithMap -> setupTracks -> Localize -> refine) that ran
 * on the host.  With it the frame stays on the device from the image to the pose: clc_match_map_dev leaves d_match[nq] on the GPU,
 * the track kernel turns it -- with the detector's keypoints and the map's 3-D points -- into the solve's correspondences, and the
 * a-contrario solve starts from them.  (Later under ABI 4: new entry points only.)
 *
 * clc_set_map_points: h_X n x 3 doubles, row i = the landmark of map descriptor row i -- scene.GetLandmarks().at(mapRegionIdx[i]).X
 * (Localizer.hpp:66), the order of clc_inter_pose_job.map_X.  Uploaded once per map, beside clc_set_map (GPUMatcher::setMapData,
 * coloc.hpp:196-198, 456-458); synchronous.  Works on a context without detector / matcher options.  n == 0: no map points any more.
 *
 * A track job, per camera.  All inputs are DEVICE memory:
 *   d_match[nq]   query q -> map row or -1, as clc_match_map_dev writes it; an index outside [0, number of map points) counts as
 *                 "no match" (the rule of clc_inter_pose_job.map_n);
 *   d_count       nullable: the detector's {written, found} pair (clc_detect_buffers); rows q >= d_count[0] are ignored, as
 *                 clc_match_jobs_counted_dev treats them.  nq is then the PLANNED size (at most the keypoint capacity);
 *   the 2-D side  EITHER d_kps, the detector's level-local keypoints (levels 0 .. 7) -- the feature position is scale * (float)x,
 *                 scale * (float)y in float with scale = (float)pow((double)1.2f, level), clc_keypoints_to_features' values
 *                 (GPUDetector.hpp:172-179) -- OR d_feat, float positions already scaled, row q at d_feat + q * feat_stride (a
 *                 Features() block: feat_stride = 4).  Exactly one of the two;
 *   cam           Pinhole_Intrinsic_Radial_K3: the position, widened to double, goes through get_ud_pixel (ima2cam, the r2 == 0
 *                 shortcut, both 1.05 bracket loops, bisection to 1e-10, cam2ima) in fp64 in the host's operation order, so the
 *                 result has the host's bits.  (A bracket the host's bisection would never leave ends after 4096 steps here.)
 * The tracks are the accepted queries in ASCENDING q -- the order matchFeaturesWithMap emits (GPUMatcher.hpp:263-266) and
 * setupTracks walks; the a-contrario sampler is a function of (seed, iteration, index set), so the order is part of the result.
 *
 * clc_track_build_dev: the kernel alone, enqueue only on `stream` (capturable like the other _dev entries); reads the inputs and
 * cam of *job, writes d_X (3 N), d_x (2 N), d_query / d_map (N int32: the reference's trackedFeatures j_ / i_) and *d_n = N.  The
 * output buffers hold job->nq tracks each; all but d_X and d_x are nullable.
 *
 * clc_track_localize_dev: tracks + Localizer::localizeImage (Localizer.hpp:77-108) for one camera, from device memory: the track
 * launch, then the a-contrario solve of clc_pnp_acransac (refine == 0) / clc_pnp_localize_ac (refine != 0) with
 * K = { focal, 0, ppx; 0, focal, ppy; 0, 0, 1 } (Pinhole_Intrinsic_Radial_K3::K()), same result bit for bit as those entries give
 * for the host-gathered copy of the same tracks.  The host waits for ONE number, the track count N (a pinned word the kernel
 * writes; the a-contrario tables depend on it); matches, keypoints, map points and correspondences are never copied in either
 * direction.  Host outputs (nullable): Rt 12, cov 36 (refine), track_query / track_map / inliers / inlier_mask with room for nq
 * entries (inliers index the track list, ascending residual order).  N <= 3: CLC_OK, n_inliers = 0; N > 16384: CLC_ERR_CAPACITY;
 * no map points, or fewer map points than the context's map rows (clc_set_map): CLC_ERR_STATE; both or neither of d_kps / d_feat:
 * CLC_ERR_BAD_ARG.
 * ORDERING.  A context's stream is NON-BLOCKING: it does not wait for work on the NULL stream or any other stream.  A caller that
 * produced d_match / d_kps on another stream (torch's current stream, say) passes it as after_stream: the call records an event
 * there and makes its own stream wait for it -- no host synchronisation.  after_stream == NULL means "already ordered": the inputs
 * were produced on the context's own stream (clc_stream) or are complete.
 *
 * clc_track_localize_batch_dev: n jobs, job i on ctxs[i] (a context of its own each, one device, as clc_pnp_localize_ac_batch);
 * the map points are ctxs[0]'s.  ONE track launch for the batch on ctxs[0]'s stream, then the solves interleaved or in lockstep
 * exactly as clc_pnp_localize_ac_batch runs them; every job's result is the single call's.  jobs[i].status per job; returns the
 * first failure. */
typedef struct clc_camera_k3 { double focal, ppx, ppy, k1, k2, k3; } clc_camera_k3;
typedef struct clc_track_job {
    /* in */
    const int32_t*      d_match;
    int                 nq;
    const uint32_t*     d_count;      /* nullable */
    const clc_keypoint* d_kps;        /* or */
    const float*        d_feat;
    int                 feat_stride;  /* floats per row of d_feat */
    clc_camera_k3       cam;
    void*               after_stream; /* nullable: the stream that produced d_match / d_kps */
    int                 max_iteration;
    uint64_t            seed;
    double              precision;    /* +inf: a-contrario threshold */
    int                 refine;
    double              huber_a;      /* <= 0: 16 */
    /* out (pointers nullable, host memory) */
    double*             Rt;
    double*             cov;
    int32_t*            track_query;
    int32_t*            track_map;
    int32_t*            inliers;
    uint8_t*            inlier_mask;
    int                 n_tracks, n_inliers, iterations, status;
    double              error_max, rmse;
} clc_track_job;
int clc_set_map_points(clc_ctx* ctx, const double* h_X, int n);
int clc_track_localize_dev(clc_ctx* ctx, clc_track_job* job);
int clc_track_localize_batch_dev(clc_ctx* const* ctxs, clc_track_job* jobs, int n_jobs);
int clc_track_build_dev(clc_ctx* ctx, const clc_track_job* job, double* d_X, double* d_x, int32_t* d_query, int32_t* d_map,
                        int32_t* d_n, void* stream);

/* ---- two-view correspondences on the device: replaces the gather of RobustMatcher::computeRelativePose (RobustMatcher.hpp:372-424,
 * the loop at :393-398) -----------------------------------------------------------------------------------------------------------
 * The twin of the track entries for the pair filter (filterMatches in initMap / updateMap, filterMatchesPair in interPoseEstimator,
 * coloc.hpp:296): the pair's d_match stays on the GPU, the pair kernel turns it -- with the two cameras' keypoints -- into the
 * undistorted correspondences x1 / x2, and the a-contrario solve of clc_two_view_acransac starts from them.  (Later under ABI 4: new
 * entry points only.)
 *
 * A pair job.  Camera A = pair.first (the QUERY side of the match), camera B = pair.second (the TRAIN side).  All inputs are DEVICE
 * memory:
 *   d_match[nq]   query row of camera A -> train row of camera B, or -1, as clc_match_2nn_dev / clc_match_jobs_*_dev /
 *                 clc_match_ratio_2nn_dev write it;
 *   nt            rows of camera B; d_count_a / d_count_b nullable: the detectors' {written, found} words (clc_detect_buffers).  Rows
 *                 q >= d_count_a[0] are ignored; a train index outside [0, min(nt, d_count_b[0])) counts as "no match" (the rule of
 *                 clc_track_job);
 *   the 2-D side  for each camera independently EITHER d_kps_* (level-local keypoints, position = scale * (float)x in float, the
 *                 values of clc_keypoints_to_features) OR d_feat_* + feat_stride_* (float positions already scaled), as clc_track_job;
 *   cam_a, cam_b  Pinhole_Intrinsic_Radial_K3 of the two cameras: both positions go through get_ud_pixel in fp64 in the host's
 *                 operation order (the host's bits).
 * The correspondences are the accepted queries in ASCENDING q -- the order GPUMatcher::computeMatches emits IndMatch(i, h_matches[i])
 * (GPUMatcher.hpp:215-220); the a-contrario sampler is a function of the index set, so the order is part of the result.
 *
 * clc_pair_build_dev: the kernel alone, enqueue only on `stream` (capturable like the other _dev entries); writes d_x1 / d_x2 (2 N
 * doubles each, undistorted PIXELS), d_pair_q / d_pair_t (N int32: the rows of camera A / B) and *d_n = N.  The output buffers hold
 * job->nq pairs each; all but d_x1 and d_x2 are nullable.
 *
 * clc_pair_filter_dev: the pair launch, then the solve of clc_two_view_acransac under model 'E', 'F' or 'H' (both images img_w x img_h)
 * from device memory, same result bit for bit as that entry gives for the host-gathered copy of the same correspondences; for 'E',
 * K1 / K2 = { focal, 0, ppx; 0, focal, ppy; 0, 0, 1 } of cam_a / cam_b.  The conditioning of 'F' / 'H' (x * d + tx, y * d + ty) is
 * applied by the staging launch on the device.  The host waits for ONE number, the pair count N; matches, keypoints and
 * correspondences are never copied in either direction (no copy command is issued).  Host outputs (nullable): M 9 (E, F or H in
 * pixels), F 9 (zeros for 'H'), pair_q / pair_t / inliers / inlier_mask with room for nq entries, x1 / x2 with room for 2 nq doubles
 * (the undistorted pixels, from pinned mirrors the kernel writes).  N <= sample size (5, 7, 4): CLC_OK, n_inliers = 0;
 * N > 16384: CLC_ERR_CAPACITY; both or neither of d_kps / d_feat for a camera, a misaligned pointer, a non-positive focal, an unknown
 * model: CLC_ERR_BAD_ARG.  after_stream: as clc_track_job.
 *
 * clc_pair_filter_batch_dev: n jobs of ONE model, job i on ctxs[i] (a context of its own each, one device).  ONE pair launch for the
 * batch on ctxs[0]'s stream, then the solves interleaved or in lockstep exactly as clc_two_view_acransac_batch runs them; every job's
 * result is the single call's.  jobs[i].status per job; returns the first failure. */
typedef struct clc_pair_job {
    /* in */
    const int32_t*      d_match;
    int                 nq, nt;
    const uint32_t*     d_count_a;      /* nullable */
    const uint32_t*     d_count_b;      /* nullable */
    const clc_keypoint* d_kps_a;        /* or */
    const float*        d_feat_a;
    int                 feat_stride_a;  /* floats per row of d_feat_a */
    const clc_keypoint* d_kps_b;        /* or */
    const float*        d_feat_b;
    int                 feat_stride_b;
    clc_camera_k3       cam_a, cam_b;
    void*               after_stream;   /* nullable: the stream that produced d_match / the keypoints */
    int                 img_w, img_h, max_iteration;
    uint64_t            seed;
    double              precision;      /* +inf: a-contrario threshold */
    /* out (pointers nullable, host memory) */
    double*             M;
    double*             F;
    int32_t*            pair_q;
    int32_t*            pair_t;
    double*             x1;
    double*             x2;
    int32_t*            inliers;
    uint8_t*            inlier_mask;
    int                 n_pairs, n_inliers, iterations, status;
    double              error_max, min_nfa;
} clc_pair_job;
int clc_pair_filter_dev(clc_ctx* ctx, int model, clc_pair_job* job);
int clc_pair_filter_batch_dev(clc_ctx* const* ctxs, int model, clc_pair_job* jobs, int n_jobs);
int clc_pair_build_dev(clc_ctx* ctx, const clc_pair_job* job, double* d_x1, double* d_x2, int32_t* d_pair_q, int32_t* d_pair_t,
                       int32_t* d_n, void* stream);

/* ---- the guided match: K2NN along epipolar lines under a known F -------------------------------------------------------------------
 * The reference began this step and never finished it: RobustMatcher::matchMaps (RobustMatcher.hpp:295-362) evaluates f1^T F f2 for
 * every putative match, sorts by it and keeps everything (the gate and the "best two" variant are commented out).  What follows is THIS
 * library's statement of the step, as clc_match_ratio_2nn_dev and CLC_SELECT_STRONGEST are; OpenMVG is an empty submodule of the
 * reference, so parity with its geometry_aware::GuidedMatching is NOT pinned.  (Later under ABI 4: new entry points only.)
 *
 * K2NN's acceptance is global: a query is accepted only if its best Hamming distance beats its second best over ALL train rows by more
 * than the threshold (CUDAK2NN.cu:75), so on repeated structure the true match loses to, or ties with, a look-alike elsewhere in the
 * image.  Once a pair has a model -- clc_pair_filter_dev's F, or two poses -- the match of x_a lies on the line F x_a: the guided match
 * takes the top-2 over the train rows near that line only.
 *
 * THE RULE.  Camera A is the query side, camera B the train side.  F: 9 doubles, row-major, in undistorted PIXELS, x_b^T F x_a = 0 --
 * the orientation and units of clc_pair_job.F, so the filter's output is usable as it is.
 *   positions   feature position (d_kps: scale * (float)x in float; d_feat + stride: the floats as they are), then get_ud_pixel in fp64,
 *               for every row of A and of B: exactly what clc_pair_job's gather computes, rows from d_kps_* or d_feat_* per side with
 *               clc_camera_k3 per side, row counts nq / nt, clipped by d_count_a[0] / d_count_b[0] where given.
 *   line of q   l = F (u, v, 1) in fp64 (each row (F0 u + F1 v) + F2, no contraction), n = sqrt(l0 l0 + l1 l1), L = (l0 / n, l1 / n,
 *               l2 / n), each rounded ONCE to float.  n zero or not finite, or a component of L not finite: the query has NO candidates.
 *   train point (x, y) = the undistorted pixel, each rounded once to float.
 *   gate        in fp32 with explicit fused operations: e = fmaf(L0, x, fmaf(L1, y, L2)); train row t is a CANDIDATE of q iff
 *               fabsf(e) <= band.  band: the caller's half-width in pixels, finite and > 0.
 *   top-2       CUDAK2NN.cu:54-75 over the CANDIDATES only, in train-index order: the lowest index wins a tie for the minimum; the
 *               sentinels are second = 100000 with exactly one candidate, best = 100000 (second = 200000) with none; accept iff
 *               second - best > threshold (threshold truncated to 8 bits as the reference's kernel parameter is).  So a lone candidate
 *               is accepted, a query without candidates is -1, and a tie for the minimum INSIDE the band is rejected.
 *   outputs     d_match[nq] (train row or -1), d_best / d_second (nullable; distances, sentinels saturated to 65535) as the other
 *               entries write them; d_line (3 nq floats) / d_tpos (2 nt floats), nullable: the lines and train points the sweep read.  A
 *               query without a line, and every row at or past a device-side count, holds quiet NaNs (0x7FC00000) there; planned query
 *               rows past d_count_a[0] are answered -1, train rows past d_count_b[0] are never candidates.
 * The gate is the ONE-SIDED point-to-line distance in image B.  That is a choice: the symmetric form would need B's lines in A too
 * (a second prep pass and two more fused operations per pair).
 *
 * Both entries are enqueue-only on `stream` (0: the context's), capturable once the context's scratch has its size, no host wait: F and
 * band are host arguments.  They run the popcount formulation of the sweep with the gate in its loop, whatever formulation the context
 * is set to (the matrix formulation is not touched), preceded by a prep launch that writes the lines and the train points.
 * clc_match_guided_batch_dev: n_jobs in [0, CLC_MAX_TRACK_PAIRS] on one context, every job's result the single call's, ONE sweep
 * launch; the prep is ONE launch for up to 14 jobs and two beyond (a prep record carries two cameras and F in fp64: 14 of them fill the
 * 4 KB of kernel arguments).
 * Limits and errors: nt > 2^22 (where the plain sweep changes to its slab path): CLC_ERR_CAPACITY; nt == 0: every query -1; both or
 * neither of d_kps / d_feat for a camera, a misaligned pointer (descriptor rows: 16 bytes), a non-positive focal, a band that is not
 * finite and positive, a null context or job: CLC_ERR_BAD_ARG; a context without matcher options: CLC_ERR_STATE.
 * d_match feeds clc_pair_build_dev, clc_pair_filter_dev, clc_tracks_pair and clc_map_build_dev unchanged. */
typedef struct clc_guided_job {
    const void*         d_q;            /* camera A's descriptors: nq rows of 64 bytes, 16-byte aligned */
    int                 nq;
    const void*         d_t;            /* camera B's */
    int                 nt;
    const uint32_t*     d_count_a;      /* nullable, as clc_pair_job */
    const uint32_t*     d_count_b;
    const clc_keypoint* d_kps_a;        /* or */
    const float*        d_feat_a;
    int                 feat_stride_a;
    const clc_keypoint* d_kps_b;        /* or */
    const float*        d_feat_b;
    int                 feat_stride_b;
    clc_camera_k3       cam_a, cam_b;
    double              F[9];
    float               band;
    int                 threshold;
    int32_t*            d_match;        /* nq, device */
    uint16_t*           d_best;         /* nullable, device */
    uint16_t*           d_second;
    float*              d_line;         /* nullable, device: 3 nq floats */
    float*              d_tpos;         /* nullable, device: 2 nt floats */
} clc_guided_job;
int clc_match_guided_dev(clc_ctx* ctx, const clc_guided_job* job, void* stream);
int clc_match_guided_batch_dev(clc_ctx* ctx, const clc_guided_job* jobs, int n_jobs, void* stream);

/* ---- tracking by projection: K2NN against the map around a predicted pose ------------------------------------------------------------
 * The step every frame runs, matchSceneWithMap / clc_match_map_dev (coloc.hpp:219), sweeps every query against every map row whatever
 * the camera is known to be looking at, so K2NN's global acceptance (CUDAK2NN.cu:75) lets a look-alike landmark anywhere in the map
 * kill a true match.  From the second frame on a pose prediction exists (the previous pose, or the filter's statePre), and the map's
 * landmarks are in the context (clc_set_map_points and every clc_map_*_dev install): a keypoint is matched only against the landmarks
 * that PROJECT near it under the predicted pose.  The same call serves as a re-match under the pose a solve has just returned.  The
 * reference has no such step: like the guided match above this is THIS library's statement, parity with nothing is pinned, and no
 * existing entry changes.  (Later under ABI 4: new entry points only.)
 *
 * THE RULE.  The train side is the context's map: the rows of clc_set_map and the landmarks of clc_set_map_points (or of an install),
 * map_n = the number of map rows, as for clc_match_map_dev.
 *   query point  feature position (d_kps: scale * (float)x in float; d_feat + stride: the floats as they are), then get_ud_pixel in
 *                fp64: exactly what the track kernel computes for pt2D (clc_track_job).  Each coordinate rounded ONCE to float.  Rows
 *                at or past d_count[0] hold quiet NaNs (0x7FC00000) and are answered -1.
 *   train point  of map row i, in fp64, source order, no contraction: Xc = R X_i + t, each row ((R0 X0 + R1 X1) + R2 X2) + t;
 *                u = focal * (Xc[0] / Xc[2]) + ppx, v = focal * (Xc[1] / Xc[2]) + ppy, each rounded once to float.  The row has NO
 *                projection (two quiet NaNs) unless Xc[2] > 0 and both floats are finite.  This is the UNDISTORTED pixel, the space the
 *                solve works in: no distortion is applied to the projection (k1, k2, k3 act on the query side only).
 *   gate         in fp32 with explicit operations: dx = x_t - x_q, dy = y_t - y_q, d2 = fmaf(dx, dx, dy * dy); map row t is a CANDIDATE
 *                of q iff d2 <= r2, where r2 = radius * radius is formed once on the host in float.  A NaN anywhere gives false; a
 *                distance of exactly `radius` is inside.
 *   top-2        word for word the guided match's: CUDAK2NN.cu:54-75 over the CANDIDATES only, in map-row order; a lone candidate is
 *                accepted, no candidate gives -1, a tie for the minimum inside the window is rejected; the threshold is truncated to 8
 *                bits; d_best / d_second (nullable) are saturated to 65535.
 *   outputs      d_match[nq]: a map row or -1, clc_match_map_dev's orientation, so it feeds clc_track_localize_dev / _batch_dev /
 *                clc_track_build_dev unchanged.  d_qpos (2 nq floats) / d_proj (2 map_n floats), nullable: the points the sweep read.
 *   Rt           HOST, 12 doubles: the PREDICTED [R|t], world to camera, row-major 3 x 4 -- the layout clc_track_job.Rt returns.
 *
 * Both entries are enqueue-only on `stream` (0: the context's), capturable once the context's scratch has its size, no host wait.  They
 * run the popcount formulation of the sweep with the gate in its loop (the guided match's kernel, instantiated with this gate),
 * preceded by ONE prep launch that writes the query points and the projections.  clc_match_map_guided_batch_dev: the cameras of one
 * frame against the context's one map, n_jobs in [0, CLC_MAX_BATCH], every job's result the single call's, one prep and one sweep launch.
 * Errors, all checked before anything is enqueued: radius or radius * radius not finite and positive, a non-finite Rt, both or neither
 * of d_kps / d_feat, a misaligned pointer (descriptor rows: 16 bytes), a non-positive focal, a null context or job, n_jobs out of range:
 * CLC_ERR_BAD_ARG; a context without matcher options, without a map, or with fewer map points than map rows (the rule of
 * clc_track_localize_dev): CLC_ERR_STATE; more than 2^22 map rows: CLC_ERR_CAPACITY.  nq == 0: nothing is written.  An empty map
 * (map_n == 0): every query -1.  The fallback is the caller's: a wrong prediction yields few matches, never wrong geometry, and fewer
 * tracks than wanted means calling clc_match_map_dev. */
typedef struct clc_map_guided_job {
    const void*         d_q;            /* the frame's descriptors: nq rows of 64 bytes, 16-byte aligned */
    int                 nq;
    const uint32_t*     d_count;        /* nullable, as clc_track_job */
    const clc_keypoint* d_kps;          /* or */
    const float*        d_feat;
    int                 feat_stride;
    clc_camera_k3       cam;
    double              Rt[12];         /* host: the predicted pose */
    float               radius;         /* pixels */
    int                 threshold;
    int32_t*            d_match;        /* nq, device */
    uint16_t*           d_best;         /* nullable, device */
    uint16_t*           d_second;
    float*              d_qpos;         /* nullable, device: 2 nq floats */
    float*              d_proj;         /* nullable, device: 2 map_n floats */
} clc_map_guided_job;
int clc_match_map_guided_dev(clc_ctx* ctx, const clc_map_guided_job* job, void* stream);
int clc_match_map_guided_batch_dev(clc_ctx* ctx, const clc_map_guided_job* jobs, int n_jobs, void* stream);

/* ---- tracking by projection through a cell grid: the same match without the whole-map sweep --------------------------------------------
 * clc_match_map_binned_dev takes clc_match_map_guided_dev's job and leaves clc_match_map_guided_dev's outputs, bit for bit: the rule
 * above is THE rule (query point, train point, gate, top-2, outputs, Rt).  What differs is which map rows a query meets.  The
 * projections are binned into a grid of cells and a query visits only the cells its window covers; every row it visits goes through
 * the unchanged gate, the window holds every row that can pass it, and the top-2 is a fold of keys
 * (distance << 22) + row by min / med3, which does not depend on the order the rows are met in.  (Later under ABI 4: new entry points
 * only; the guided entries keep their code.)
 *
 * THE CELL RULE, in fp64 with + - * /, floor, min, max in source order (coloc_amd/csrc/bin_math.h, host and device):
 *   rw    = (double)radius * (1.0 + 0x1p-10)               the window's half-width
 *   W     = 2.0 * max(cam.ppx, cam.ppy)                    the grid's extent on both axes, origin (0, 0)
 *   c     = max(rw, W / 64.0)                              the cell's side: never below rw
 *   k(v)  = (int)min(max(floor(v / c), -1.0), 64.0) + 1    1 .. 64 inside, 0 and 65 the ring; clamped BEFORE the conversion
 *   cell(x, y) = k(y) * 66 + k(x)                          66 * 66 = 4356 cells, row-major
 *   binned rows   map row i is binned iff it has a projection; its cell is cell((double)x_t, (double)y_t) of the floats the prep wrote.
 *   query window  kx in [k((double)x_q - rw), k((double)x_q + rw)], ky likewise: at most 3 x 3 cells, at most three contiguous runs of
 *                 the table sorted by cell.  A query whose point is NaN has no window and is answered -1.
 *   THE PLAN      host-side, from the job and the map's size alone.  BINNED iff radius >= 2^-10, 8 rw <= W, 0 < map_n <= 65 536 and
 *                 ppx, ppy finite and positive; otherwise SWEEP: the entry runs clc_match_map_guided_dev's path for that job, with the
 *                 same bits.
 *
 * clc_match_map_binned_dev / _batch_dev: outputs, errors and limits are clc_match_map_guided_dev's -- the same argument checks before
 * anything is enqueued, CLC_ERR_STATE / CLC_ERR_CAPACITY as there, an empty map gives every query -1, nq == 0 writes nothing.  Enqueue
 * only on `stream` (0: the context's), capturable once the context's scratch has its size, no host wait: the prep launch of the guided
 * entry, one workgroup per job that builds the table (histogram, scan, scatter), one match launch with 16 lanes per query.  Batch: n_jobs
 * in [0, CLC_MAX_BATCH], every job's result the single call's; the BINNED jobs share one prep, one bin and one match launch, the SWEEP
 * jobs go through the guided path together.
 *
 * clc_map_bin_build_dev: the inner step alone -- prep and bin for `job` -- with the table copied out: d_cell_start[4357] (device; entry
 * i = the rows in cells below i, entry 4356 = the binned rows) and d_cell_row[map_n] (device; the map rows in cell order, the order
 * inside a cell unspecified; entries at or past d_cell_start[4356] are not written).  Rows without a projection appear in no cell.  It
 * builds the table whatever the plan says of the radius; the job's checks are the match's, and further: a null or misaligned table or a
 * principal point that is not finite and positive: CLC_ERR_BAD_ARG; more than 65 536 map rows: CLC_ERR_CAPACITY.
 *
 * clc_map_binned_plan: what the entry would do for (cam, radius) on this context's map: info = { plan (0 SWEEP, 1 BINNED), cells per
 * axis (66), lanes per query (16), 0 }, *cell_side (nullable) = c.  A null context, camera or info: CLC_ERR_BAD_ARG. */
#define CLC_BIN_PLAN_SWEEP  0
#define CLC_BIN_PLAN_BINNED 1
int clc_match_map_binned_dev(clc_ctx* ctx, const clc_map_guided_job* job, void* stream);
int clc_match_map_binned_batch_dev(clc_ctx* ctx, const clc_map_guided_job* jobs, int n_jobs, void* stream);
int clc_map_bin_build_dev(clc_ctx* ctx, const clc_map_guided_job* job, int32_t* d_cell_start, int32_t* d_cell_row, void* stream);
int clc_map_binned_plan(const clc_ctx* ctx, const clc_camera_k3* cam, float radius, int32_t* info, double* cell_side);

/* ---- one-to-one matches: each train row keeps its best claimant -----------------------------------------------------------------------
 * K2NN answers each query on its own, so several queries can name ONE train row -- from the plain sweep, the map sweep, the ratio rule,
 * the guided and the binned match alike.  Downstream that costs a whole track (the TRACKS rule below drops a component with two nodes of
 * one camera), hands clc_track_prior_dev one landmark with two observations that no gate can tell apart, and is the division by zero
 * clc_map_align_dev guards.  This filter turns any (d_match, d_best) pair into a one-to-one d_match in place, on the device.  The
 * reference has no such step: like the guided match this is THIS library's statement, parity with nothing is pinned, and no existing
 * entry changes.  (Later under ABI 4: new entry points only.)
 *
 * THE RULE (coloc_amd/csrc/unique_math.h, host and device), for nq entries against a train set of nt rows:
 *   claim        entry q is a CLAIM on train row t = d_match[q] iff 0 <= t < nt and d_best[q] <= 512.
 *   sanitising   any other entry that is not -1 -- a row outside the train set, a distance no producer writes beside a match -- is NOT a
 *                claim and is set to -1.  The library never uses an unchecked index as an address.
 *   key          key(q) = (d_best[q] << 22) | q, 32 bits: the (distance << 22) + row key the binned match folds, with the query row as
 *                the index.  512 << 22 is 2^31, so it fits; nq > 2^22 is CLC_ERR_CAPACITY, refused before anything is allocated or
 *                enqueued.
 *   holder       holder(t) = the claimant of t with the smallest key: the smallest distance wins, a tie goes to the lowest query row, the
 *                way K2NN keeps the lowest index.
 *   outputs      d_match[q] stays iff holder(d_match[q]) == q, else -1.  d_owner[t] (nullable, nt int32) = holder(t), or -1 where nobody
 *                claims t.
 * So: no train row appears twice and d_owner[d_match[q]] == q for every kept q; the kept set is a subset of the input with exactly one
 * survivor per claimed row; applying the filter twice changes nothing; and nothing depends on scheduling -- it is an integer minimum.
 * This is deliberately NOT the mutual-nearest rule, which needs a second sweep with the roles swapped: this rule needs only the distances
 * the first sweep already has, so it also serves the gated producers (guided, map-guided, binned), which have no reverse sweep.
 * nq == 0: d_match is untouched and d_owner (if given) is all -1.  nt == 0: every entry becomes -1.
 *
 * clc_match_unique_dev / _batch_dev: the filter alone.  Enqueue only on `stream` (0: the context's), no host wait, capturable once the
 * context's scratch has its size (one call at the planned sizes before a capture).  AT MOST THREE enqueued operations per call whatever
 * the batch size: the claim words armed (one uint32 per train row per job, in a workspace of the context), the claim launch (one thread
 * per query, a 32-bit unsigned atomic minimum into the word of its row), the resolve launch (thread i: query i and train row i, both only
 * reading claim words).  The words are armed on EVERY call.  Batch: n_jobs in [0, CLC_MAX_TRACK_PAIRS] on one context, jobs on a grid
 * dimension, every job's result the single call's.
 * The producers whose job carries d_best -- clc_match_guided_dev, clc_match_map_guided_dev and their batches -- need no entry of their
 * own: set d_best in the job and call clc_match_unique_dev behind them on the same stream.
 *
 * The composed entries are their producer and then the filter on the same stream; d_match before the filter is exactly the producer's:
 *   clc_match_2nn_unique_dev         clc_match_2nn_dev (the context's formulation, unchanged), its distances in the context's scratch
 *   clc_match_map_unique_dev         clc_match_map_dev likewise; nt = the context's map rows
 *   clc_match_map_binned_unique_dev  clc_match_map_binned_dev with job->d_best, or the context's scratch where that is null; BINNED and
 *                                    SWEEP plans alike; nt = the context's map rows
 *   clc_match_2nn_unique             clc_match_2nn (host arrays, published blocks, the VERIFY re-sweep) with the filter in front of the
 *                                    download: the filter always stands behind the sweep whose result is returned.  h_owner: nullable, nt.
 * Errors follow each producer's rules.  Further, all before anything is allocated or enqueued: a null context or job, a null d_match or
 * d_best with nq > 0, a negative count, a pointer that is not 4-byte aligned (d_best: 2-byte), n_jobs out of range: CLC_ERR_BAD_ARG; a
 * context without matcher options: CLC_ERR_STATE; nq > 2^22: CLC_ERR_CAPACITY.
 * OUT OF SCOPE: a query set dealt out in slices -- clc_match_jobs_dev / _counted_dev and clc_mc_* -- because a claim must see every
 * query of the pair: call the pair entry per pair there.  clc_map_align_dev's internal sweep is as it was. */
typedef struct clc_unique_job {
    int32_t*        d_match;   /* nq, device, filtered IN PLACE */
    const uint16_t* d_best;    /* nq, device: the distances the producer wrote beside d_match */
    int             nq;
    int             nt;        /* rows of the train set (the planned capacity where its count lives on the device) */
    int32_t*        d_owner;   /* nullable, nt, device */
} clc_unique_job;
int clc_match_unique_dev(clc_ctx* ctx, const clc_unique_job* job, void* stream);
int clc_match_unique_batch_dev(clc_ctx* ctx, const clc_unique_job* jobs, int n_jobs, void* stream);   /* n_jobs in [0, CLC_MAX_TRACK_PAIRS] */
int clc_match_2nn_unique_dev(clc_ctx* ctx, const void* d_q, int nq, const void* d_t, int nt, int threshold, int32_t* d_match,
                             int32_t* d_owner, void* stream);
int clc_match_map_unique_dev(clc_ctx* ctx, const void* d_q, int nq, int threshold, int32_t* d_match, int32_t* d_owner, void* stream);
int clc_match_map_binned_unique_dev(clc_ctx* ctx, const clc_map_guided_job* job, int32_t* d_owner, void* stream);
int clc_match_2nn_unique(clc_ctx* ctx, const void* h_q, int nq, const void* h_t, int nt, int threshold, int32_t* h_match,
                         int32_t* h_owner /* nullable */);

/* ---- a tracked frame's pose from the prediction: the solve behind the match by projection -----------------------------------------------
 * clc_track_localize_dev runs Localize for every frame: the host waits for the track count, drives the a-contrario P3P solve round by
 * round, then refines.  With a predicted pose and tracks that all lie within `radius` of where that pose puts them (the guided / binned
 * match above), sampling has nothing left to find: the pose is a few robust Gauss-Newton steps from the prediction.  These entries
 * give pose, inliers and covariance from the prediction and the tracks in ONE solve launch behind the track gather, with no minimal
 * sample; the host waits for one record at the end and for nothing in between, the track count included.  The reference has no
 * counterpart -- intraPoseEstimator always calls Localize (coloc.hpp:223, Localizer.hpp:77-108) --: like the matches by projection this
 * is THIS library's statement, parity with nothing is pinned, and no existing entry changes.  (Later under ABI 4: new entry points
 * only.)
 *
 * THE RULE.
 *   inputs       N tracks (X_i, x_i) in the track list's order -- accepted queries ascending, x_i through get_ud_pixel: exactly what
 *                clc_track_build_dev writes --, K = { focal, 0, ppx; 0, focal, ppy; 0, 0, 1 }, the prior [R0|t0] (HOST, 12 doubles, the
 *                layout clc_track_job.Rt returns and clc_map_guided_job.Rt takes), gate (pixels; g2 = gate * gate is formed once on the
 *                host), huber_a (<= 0: 16), rounds (0: 4; legal 1 .. 8), max_iter per round (0: 50, as clc_pnp_refine), min_inliers
 *                (<= 0: 8, Localize's "more than 2.5 x 3" rule, as CLC_MAP_SIM_NO_MODEL).
 *   classify(p)  track i is IN iff zc_i > 0 and sq_i <= g2, with zc and sq = r0^2 + r1^2 exactly as the Levenberg-Marquardt pass computes
 *                them at the parameters p.  Any NaN gives "out"; a squared residual of exactly g2 is in.
 *   m_0          the tracks with zc_i > 0 under the prior: NO residual gate on the first round (a guided caller's tracks are within its
 *                radius by construction; for others the Huber tail bounds what an outlier can pull).
 *   round k      for k = 0 .. rounds - 1: if |m_k| < 4, stop.  p_{k+1} = the Levenberg-Marquardt of clc_pnp_refine from p_k over m_k:
 *                cost 1/2 sum rho, parameters [angle-axis | t], lambda reset to 1e-4 at the start of every round, steps x 0.1 (floor 1e-12)
 *                and x 10, the stop above 1e10, the function / gradient / parameter tests and "a failed 6 x 6 solve is a rejected step"
 *                all unchanged.  m_{k+1} = classify(p_{k+1}); if m_{k+1} == m_k, stop with converged = 1.
 *   outputs      Rt = the last p (the prior's own bits where no step was accepted); inlier_mask = classify of that pose over ALL tracks
 *                (a track dropped in one round can return in a later one); n_inliers = |mask|; cov = (J^T W J)^-1 and
 *                rmse = sqrt(cost / (2 n_inliers)) from the sums at that pose over that mask (cov zero where the 6 x 6 is not positive
 *                definite, as clc_pnp_refine); iterations summed over the rounds; rounds_run; converged;
 *                result = CLC_TRACK_PRIOR_OK when n_inliers >= max(min_inliers, 4), else CLC_TRACK_PRIOR_FEW: the pose is then the last p
 *                -- the prior itself when |m_0| < 4 or N < 4 --, cov is zero, and the call still returns CLC_OK.
 *   determinism  no floating-point atomics, sums reduced in a fixed order: two runs on the same inputs give the same bits.
 * FEW is the caller's signal to run clc_match_map_dev + clc_track_localize_dev for that frame: the library does not fall back on its own
 * (INTEGRATION.md 3n).  The first frame, and any frame after FEW, goes through clc_track_localize_dev.  The natural gate is the
 * error_max the camera's last a-contrario solve returned: the precision AC-RANSAC found, in pixels.
 *
 * clc_track_prior_dev: the frame exactly as clc_track_job names it, then the step.  The track launch of clc_track_localize_dev, then ONE
 * solve launch (one workgroup of 512 threads) on the context's stream, which reads the track count from DEVICE memory; one host wait,
 * on the pinned record the solve writes last.  Host outputs (nullable): Rt 12, cov 36, track_query / track_map / inlier_mask with room
 * for nq entries (n_tracks are written).  ORDERING: after_stream as clc_track_job.
 * clc_track_prior_batch_dev: n_jobs in [0, CLC_MAX_BATCH], job i on ctxs[i] (a context of its own each, one device), the map points
 * ctxs[0]'s; ONE track launch and ONE solve launch (a workgroup per job) on ctxs[0]'s stream; every job's result is the single call's,
 * bit for bit; jobs[i].status per job, the return value the first failure.
 * clc_pnp_refine_prior: the same solve on host arrays (one upload, one launch, the record); K as clc_pnp_refine reads it
 * ({ fx, skew, cx; 0, fy, cy; 0, 0, 1 }, anything else CLC_ERR_BAD_ARG); h_inlier_mask N bytes; every output pointer nullable.
 * Errors, all checked before anything is enqueued: a non-finite prior, gate or gate * gate not finite and positive, rounds outside
 * 0 .. 8, a negative max_iter, both or neither of d_kps / d_feat, a misaligned pointer, a non-positive focal, a null context or job,
 * n_jobs out of range: CLC_ERR_BAD_ARG; no map points, or fewer map points than map rows (clc_track_localize_dev's rule):
 * CLC_ERR_STATE.  More than 16 384 tracks: the solve works on none of the surplus and the entry returns CLC_ERR_CAPACITY after its wait
 * (clc_pnp_refine_prior: before anything is enqueued).  nq == 0 or no accepted query: CLC_OK, result = FEW, Rt = the prior. */
#define CLC_TRACK_PRIOR_OK  0
#define CLC_TRACK_PRIOR_FEW 1
typedef struct clc_track_prior_job {
    /* in: the frame, exactly clc_track_job's */
    const int32_t*      d_match;
    int                 nq;
    const uint32_t*     d_count;      /* nullable */
    const clc_keypoint* d_kps;        /* or */
    const float*        d_feat;
    int                 feat_stride;
    clc_camera_k3       cam;
    void*               after_stream; /* nullable */
    /* in: the step */
    double              Rt_prior[12];
    double              gate;         /* pixels */
    double              huber_a;      /* <= 0: 16 */
    int                 rounds;       /* 0: 4 */
    int                 max_iter;     /* per round; 0: 50 */
    int                 min_inliers;  /* <= 0: 8 */
    /* out (pointers nullable, host memory) */
    double*             Rt;
    double*             cov;
    int32_t*            track_query;
    int32_t*            track_map;
    uint8_t*            inlier_mask;
    int                 n_tracks, n_inliers, iterations, rounds_run, converged, result, status;
    double              rmse;
} clc_track_prior_job;
int clc_track_prior_dev(clc_ctx* ctx, clc_track_prior_job* job);
int clc_track_prior_batch_dev(clc_ctx* const* ctxs, clc_track_prior_job* jobs, int n_jobs);
int clc_pnp_refine_prior(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, const double* h_Rt_prior,
                         double gate, double huber_a, int rounds, int max_iter, int min_inliers, double* h_Rt, double* h_cov,
                         uint8_t* h_inlier_mask, int* n_inliers, double* rmse, int* iterations, int* rounds_run, int* converged,
                         int* result);

/* ---- the inter-camera step from device memory: ColoC::interPoseEstimator (coloc.hpp:296-340) without a host trip --------------------
 * What clc_inter_pose_batch computes, fed from the pair's d_match instead of host correspondences: the pair gather and the 'E' filter of
 * clc_pair_filter_dev, then -- on the device, in the operation order of the host path, so with its bits -- the chirality vote over the
 * four motions of E with the temporary map of the points in front of both cameras, the features that map shares with the global map,
 * its scale (colocUtils.hpp:184-211 behind the depth-ratio screen), the destination's first pose, and the refinement with its
 * covariance.  (Later under ABI 4: new entry points only.)
 *
 * job.pair: camera A = the SOURCE, camera B = the destination; the model is 'E'; its host outputs stay nullable.  The global map's
 * points are the context's (clc_set_map_points; a batch: ctxs[0]'s), map_n = their number.  The common features come from one of two
 * places, as in clc_inter_pose_job:
 *   THE REFERENCE'S CHAIN  d_first_desc + d_map_desc (DEVICE, rows of 64 B, 16-byte aligned; d_map_desc map_n rows in the map points'
 *       order): the descriptor of a temporary map point is the row of its correspondence in the block of the pair's camera with the
 *       lower id -- camera A's (pair_q) with lower_is_b == 0, camera B's (pair_t) otherwise --, gathered on the device and swept against
 *       the map's block (K2NN, threshold match_threshold, <= 0: 60);
 *   THE SHORTCUT  d_map_match_a (DEVICE, int32 per row of camera A, at least nq of them): camera A's own match against the map
 *       (clc_match_map_dev); an index outside [0, map_n) counts as "not a map feature".
 * Exactly one of the two: anything else, a null Rt_source or a misaligned pointer is CLC_ERR_BAD_ARG, no map points CLC_ERR_STATE; the
 * pair's own rules are clc_pair_filter_dev's.  The host waits for the pair count (as clc_pair_filter_dev does) and for ONE more number,
 * the points in front of both cameras; matches, correspondences, map and temporary map are never copied in either direction.  Outputs as clc_inter_pose_job (stage says how far the job got;
 * pair.status the job's status); ordering: pair.after_stream, as clc_track_job -- d_map_match_a and the descriptor blocks count among
 * the inputs it orders.
 *
 * clc_inter_pose_batch_dev: n <= CLC_MAX_BATCH jobs, job i on ctxs[i] (a context of its own each, one device); every job's result is
 * the single call's.
 *
 * clc_inter_front_dev: the first kernel alone, enqueue only on `stream` (capturable).  d_x1 / d_x2: n correspondences in undistorted
 * pixels; d_inliers (nullable: 0 .. n_inliers - 1): indices into them, an index outside [0, n) is never in front; cam_a / cam_b: focal,
 * ppx, ppy are read (K = { focal, 0, ppx; 0, focal, ppy; 0, 0, 1 }); h_motions: HOST, four candidate [R|t], 12 doubles each, passed by
 * value; d_rows / d_first (both or neither): d_first[w] = d_rows[correspondence of kept point w].  Writes, for the FIRST candidate with
 * the strictly largest number of inliers in front of both cameras, d_Xt (3 per point), d_x2f (2), d_corr -- in the inlier list's order,
 * room for n_inliers points each -- and d_record = { n_front, chosen candidate, stage, 1 } (stage CLC_INTER_NO_MODEL below 13 inliers,
 * CLC_INTER_NO_RELATIVE_POSE below 8 points in front: n_front = 0, chosen = -1). */
typedef struct clc_inter_dev_job {
    clc_pair_job   pair;          /* camera A = SOURCE, camera B = destination; the model is 'E' */
    /* in */
    const double*  Rt_source;     /* host, 12: [R|t] of the source camera */
    double         huber_a;       /* <= 0: 16 */
    int            lower_is_b;    /* the reference's chain: d_first_desc is camera B's block */
    const void*    d_first_desc;  /* DEVICE; with d_map_desc: the chain.  Both NULL: the shortcut */
    const void*    d_map_desc;    /* DEVICE: the global map's rows */
    const int32_t* d_map_match_a; /* DEVICE, the shortcut: camera A's own d_match against the map */
    int            match_threshold;
    /* out */
    double         Rt[12];
    double         cov[36];
    double         rmse, scale;
    int            n_front, n_common, n_refined, stage;
    int            n_map_matches;
} clc_inter_dev_job;
int clc_inter_pose_dev(clc_ctx* ctx, clc_inter_dev_job* job);
int clc_inter_pose_batch_dev(clc_ctx* const* ctxs, clc_inter_dev_job* jobs, int n_jobs);
int clc_inter_front_dev(clc_ctx* ctx, const double* d_x1, const double* d_x2, int n, const int32_t* d_inliers, int n_inliers,
                        const clc_camera_k3* cam_a, const clc_camera_k3* cam_b, const double* h_motions, const int32_t* d_rows,
                        double* d_Xt, double* d_x2f, int32_t* d_corr, int32_t* d_first, int32_t* d_record, void* stream);

/* ---- the map on the device: multi-view tracks and the seed pair's triangulation -----------------------------------------------------
 * What ColoC::initMap (coloc.hpp:151-199) runs once and ColoC::updateMap (coloc.hpp:394-459) whenever tracking thins out, between
 * filterMatches and setMapData: the tracks of Reconstructor::initializeTracks (Reconstructor.hpp:166-173: TracksBuilder Build, Filter,
 * ExportToSTL), the seed pair's landmarks of Reconstructor::triangulatePoints (:185-239) and the map database of
 * colocData::setupMapDatabase (colocData.hpp:89-121), from the pairs' correspondences where clc_pair_filter_batch_dev left them.  It
 * ends where reconstructScene writes initial.ply; the resectionCamera loop behind it is clc_map_build_grow_dev's (the section after
 * the next) and the bundle adjustment behind that loop clc_map_build_grow_ba_dev's (the section after that); no PLY.  (Later under
 * ABI 4: new entry points only.)
 *
 * TRACKS.  A node is a (camera, feature row) named by a match; an edge is a match (cam_a, q)-(cam_b, t) of a pair cam_a < cam_b; a
 * track is a connected component.  The rules are this project's statement of OpenMVG's TracksBuilder (an empty submodule in the
 * reference tree, so unpinned, as for the ratio matcher):
 *   - a component that holds two nodes of ONE camera is dropped whole (Filter), also where the conflict only arises through a third
 *     camera (A5-B7, B7-C2, C2-A9).  K2NN is not one-to-one, so this is common (clc_match_2nn_unique_dev gives lists that are);
 *   - a surviving track has at least two nodes (Filter(2): every edge joins two cameras, so every component has);
 *   - the survivors get ids 0, 1, ... in ascending order of their smallest node in (camera, row) order.  The SET of tracks does not
 *     depend on that rule, only their order does; nothing depends on scheduling.
 * An edge that names a row outside [0, rows[camera]) is ignored; repeated edges count once.
 * A pair's edges: entries 0 .. min(n, *d_n) - 1 (d_n nullable: a count in DEVICE memory, n the planned size) of the lists d_q / d_t
 * (DEVICE, int32) -- or, with d_index (nullable; DEVICE or pinned host memory), entries d_index[0 .. ) of lists of n_list entries: a
 * filter's inlier list over the pair lists it was given; an index outside [0, n_list) names no edge.
 *
 * clc_tracks_build_dev: the tracks alone, enqueue only on `stream`, no host synchronisation between its launches.  Its union-find
 * words live in ONE block of the context, shared with clc_map_build_dev: one tracks / map build in flight per context at a time (a
 * second one, on whatever stream, is ordered behind the first by the caller).  The block grows on demand: a call that needs more
 * nodes than any call before it synchronises the CONTEXT's stream and allocates anew -- such a call is not capturable and must not
 * run while an earlier build is still in flight on another stream; every later call of that size or less only enqueues and is
 * capturable (so: one call at the planned size before a capture).
 * d_track_feat[track][camera] (int32, job->n_cams per track) = that camera's row or -1; room for min(sum of n, (sum of rows) / 2)
 * tracks, all of it written (-1 past the tracks); *d_n_tracks (int32) the number of tracks, stored last.  n_cams in
 * [2, CLC_MAX_BATCH], n_pairs in [0, CLC_MAX_TRACK_PAIRS]; a pair with cam_a >= cam_b or a camera outside [0, n_cams), a negative count,
 * a misaligned pointer: CLC_ERR_BAD_ARG.
 *
 * clc_map_build_dev: tracks, then for every track that holds both cameras of pair seed_pair, in track-id order: the two rows'
 * positions (d_kps with the pow(1.2f, level) scaling or d_feat + feat_stride, as clc_pair_job) through get_ud_pixel in fp64 (the
 * host's bits), TriangulateDLT(P1, x1.homogeneous(), P2, x2.homogeneous(), &X) with P = K [R|t] (Reconstructor.hpp:223-225; the null
 * vector by a one-sided Jacobi, coloc_amd/csrc/map_math.h), and the reference's acceptance as written: dropped iff the depth
 * (R X + t)[2] is negative under BOTH poses (:227), or iff |X[2]| > 100 (:230) (or X is not finite).  The accepted points, in
 * track-id order, are the map: row i = { X, the track id (mapRegionIdx), the row in the LOWER seed camera (obs.begin(),
 * colocData.hpp:112-116) and that row's descriptor from the camera's block }.  It is installed as the context's map -- the state
 * clc_set_map + clc_set_map_points leave, for clc_match_map_dev / clc_track_localize_dev and the rest.  No copy command is issued and
 * no descriptor or point moves through the host: the host waits for ONE number, the map's row count, then enqueues the descriptor
 * gather and returns when it has run (no data moves; as clc_set_map returns behind its upload).  ORDERING: on return the map is
 * complete and none of the job's inputs is read any more -- a matcher call on any stream may follow at once, and the caller may
 * describe the next frame into the seed camera's block.  What the call cannot know is work on OTHER streams that still reads the
 * PREVIOUS map (d_m is rewritten in place, as by clc_set_map): such work is complete, or joined to the context's stream, before
 * the call.  Host outputs (nullable): track_feat (room as d_track_feat), map_track / map_row (room for min(that, maxkp) entries), X (3
 * doubles each), from pinned mirrors the kernels write.  Rt_seed_a / Rt_seed_b: [R|t] of the seed pair's cam_a / cam_b
 * (relativePoseToAbsolute, :247-257, is the caller's: clc_map_init_batch_dev applies it).  Every camera below n_cams gives its 2-D
 * side and camera; the descriptor block (rows of 64 B, 16-byte aligned) is read for the lower seed camera.  after_stream: as
 * clc_track_job.  Fewer than two cameras, a bad pair, seed_pair outside the pairs, a misaligned pointer, both or neither of d_kps /
 * d_feat: CLC_ERR_BAD_ARG; a context without matcher options: CLC_ERR_STATE; more map rows than MatcherOptions.maxkp:
 * CLC_ERR_CAPACITY, and the previous map stays as it was; no accepted point: CLC_OK, map_n = 0 and no map points.
 *
 * clc_map_init_batch_dev: the composition initMap calls, and the first half of updateMap's (coloc.hpp:394-429; the whole of it, with
 * the tail that brings the new map to the old map's scale, is clc_map_update_batch_dev in the next section).  pair_jobs[p] on ctxs[p] (a context of its own each) is the pair
 * job->tracks.pairs[p].cam_a < cam_b (the other fields of tracks.pairs are filled in here; tracks.n_pairs == n_pairs): the filters
 * run as clc_pair_filter_batch_dev under 'E'; a pair enters the tracks by the rules of HIPRobustMatcher::computeRelativePoseDev -- at
 * least 2.5 x 5 inliers and a successful chirality vote (RobustMatcher.hpp:176-183; the host vote of clc_inter_pose_batch, fed from
 * the pinned mirrors); its edges are its inliers' pair_q / pair_t, read by the kernel from the context's block through the pinned
 * inlier list.  The seed is the pair with strictly the most inliers, the first in pair order (Reconstructor.hpp:112-118); its [R|t]
 * are seed_poses of (origin_R, origin_C, the vote's rotation and centre, scale).  Then clc_map_build_dev on ctxs[0].  Out: seed_pair
 * (-1: no pair entered -- CLC_OK, the map is left alone, map_n = -1), Rt_seed_a / Rt_seed_b, entered[p]. */
#define CLC_MAX_TRACK_PAIRS 28   /* CLC_MAX_BATCH cameras, every pair once */
typedef struct clc_tracks_pair {
    int32_t        cam_a, cam_b;  /* cam_a < cam_b */
    const int32_t* d_q;           /* rows of camera a */
    const int32_t* d_t;           /* rows of camera b */
    int            n;             /* edges (the planned size where d_n is given) */
    const int32_t* d_n;           /* nullable */
    const int32_t* d_index;       /* nullable */
    int            n_list;        /* with d_index: entries of d_q / d_t */
} clc_tracks_pair;
typedef struct clc_tracks_job {
    int                    n_cams;
    int                    rows[CLC_MAX_BATCH];  /* row capacity per camera */
    int                    n_pairs;
    const clc_tracks_pair* pairs;                /* host memory */
} clc_tracks_job;
typedef struct clc_map_camera {
    const clc_keypoint* d_kps;        /* or */
    const float*        d_feat;
    int                 feat_stride;
    clc_camera_k3       cam;
    const void*         d_desc;       /* rows[camera] x 64 B */
} clc_map_camera;
typedef struct clc_map_job {
    /* in */
    clc_tracks_job  tracks;
    clc_map_camera  cams[CLC_MAX_BATCH];
    int             seed_pair;        /* index into tracks.pairs (clc_map_init_batch_dev: out) */
    double          Rt_seed_a[12];    /* (clc_map_init_batch_dev: out) */
    double          Rt_seed_b[12];
    void*           after_stream;     /* nullable */
    double          origin_R[9];      /* clc_map_init_batch_dev only: the origin pose (rotation, centre) and the baseline's scale */
    double          origin_C[3];
    double          scale;
    /* out (pointers nullable, host memory) */
    int32_t*        track_feat;
    int32_t*        map_track;
    int32_t*        map_row;
    double*         X;
    int             n_tracks, map_n, status;
    int             entered[CLC_MAX_TRACK_PAIRS];   /* clc_map_init_batch_dev */
} clc_map_job;
int clc_tracks_build_dev(clc_ctx* ctx, const clc_tracks_job* job, int32_t* d_track_feat, int32_t* d_n_tracks, void* stream);
int clc_map_build_dev(clc_ctx* ctx, clc_map_job* job);
int clc_map_init_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job);

/* ---- the map replaced on the device at the old map's scale: updateMap's tail ---------------------------------------------------------
 * What ColoC::updateMap (coloc.hpp:435-459) runs after reconstructScene and setupMapDatabase, before data = updateData / setMapData:
 * matchMapFeatures(old map, new map) under threshold 60 (GPUMatcher.hpp:157-163), matchMaps keeping every match
 * (HIPRobustMatcher.hpp:627-672), computeScaleDifference over consecutive common features (colocUtils.hpp:184-211) and rescaleMap of
 * the new scene, landmarks and pose centres (:213-223).  A new map comes with an arbitrary baseline; this tail keeps the cameras'
 * trajectory at one scale across map updates.  It needs the OLD map's descriptor rows after the new ones exist, so the new rows are
 * gathered into a second buffer and the two change places.  (Later under ABI 4: new entry points only.)
 *
 * clc_map_align_dev: the step on a new map already in device memory -- new row i = row d_rows[i] of d_desc (d_rows NULL: row i),
 * its landmark d_X[3 i ..].
 *   COMMON FEATURES: the K2NN matches with Q = the context's installed map (map_n rows = n_old) and T = the new rows, threshold <= 0:
 *     60, listed in ascending old row as computeMatches emits them; an index outside [0, n_new) is no match.  With n_old == 0 or
 *     n_new == 0 no sweep is launched and the list is empty.
 *   SCALE: for list entries k and k + 1 (k = 0 .. n_common - 2) one term, (float)|oldX[q_k+1] - oldX[q_k]| / (float)|newX[t_k+1] -
 *     newX[t_k]| (scale_term, coloc_amd/csrc/inter_math.h).  A term whose denominator fails the d2 > 1e-9f guard is skipped: K2NN is
 *     not one-to-one, two consecutive old rows matched to ONE new row are common, and the reference divides by zero there.  The kept
 *     terms (n_terms of them) are summed by one lane in list order -- the bits depend on the order -- and divided by n_terms
 *     (scale_from_sum).  Fewer than two common features, no kept term, or a mean that is not positive and finite: scale = 1.0 and
 *     status = CLC_MAP_ALIGN_NO_SCALE.  (The reference returns 1.0 for the empty list and NaN for a single common feature; this call
 *     gives 1.0 in both cases.)
 *   RESCALE: X_new[i] = d_X[i] * scale, each component one multiply, into the context's staging buffer and -- where X was asked for --
 *     a pinned mirror.  d_X itself is not written.
 *   INSTALL (install != 0): the gathered rows and the rescaled points become the context's map by changing places with the previous
 *     map's buffers; map rows = map points = n_new.  ORDERING as clc_map_build_dev: the call returns when its last launch has run, a
 *     matcher call on any stream may follow at once; work on other streams that still reads the PREVIOUS map (or, still, the one
 *     before it, whose buffers are the ones rewritten here) is complete, or joined to the context's stream, before the call.
 *     n_new == 0 installs the empty map as clc_map_build_dev does (no map points), scale 1.0, CLC_MAP_ALIGN_NO_SCALE.
 *   install == 0: report only, the context's map is left exactly as it was.
 * The host waits for ONE word, the pinned record { scale, n_common, n_terms, status }, released last behind a system-scope fence; no
 * descriptor, point or match is copied in either direction: match / X (nullable) come from pinned mirrors the kernel writes.
 * after_stream: as clc_map_job.  ERRORS: no installed map with points (no clc_set_map / build, no map points, or fewer points than
 * rows): CLC_ERR_STATE; a context without matcher options: CLC_ERR_STATE; n_new > MatcherOptions.maxkp: CLC_ERR_CAPACITY; a negative
 * count, a null d_desc / d_X with n_new > 0, d_desc not 16-byte aligned, d_rows / d_X misaligned: CLC_ERR_BAD_ARG.  On every error
 * the previous map serves exactly as before.
 *
 * clc_map_update_batch_dev: the composition updateMap calls.  Everything clc_map_init_batch_dev does up to and including the seed
 * triangulation, the capacity check and the host outputs; then, instead of the gather into the matcher's map, the align step with
 * d_desc = the lower seed camera's block, d_rows = the map's row list, d_X = the staged points, install = 1.  Of `align` only
 * threshold and match are read; its out fields are written.  On return job->X holds the RESCALED landmarks and job->Rt_seed_a /
 * Rt_seed_b the rescaled poses (rescale_pose, coloc_amd/csrc/map_math.h: C = -R^T t, C' = C * scale, t' = -R C'), align->scale what
 * was applied.  No pair entered: exactly as clc_map_init_batch_dev -- CLC_OK, seed_pair = -1, map_n = -1, the map untouched -- with
 * align->status = CLC_MAP_ALIGN_NO_SCALE, scale 1.0.  No previous map with points on ctxs[0]: CLC_ERR_STATE before any filter is
 * launched. */
enum { CLC_MAP_ALIGN_OK = 0, CLC_MAP_ALIGN_NO_SCALE = 1 };
typedef struct clc_map_align {
    /* in */
    const void*    d_desc;       /* descriptor block, rows of 64 B, 16-byte aligned */
    const int32_t* d_rows;       /* nullable: new map row i = row d_rows[i] of d_desc; NULL: row i */
    const double*  d_X;          /* n_new x 3, NOT written */
    int            n_new;
    int            threshold;    /* <= 0: 60 (GPUMatcher.hpp:162) */
    int            install;      /* 0: report only, the context's map is left exactly as it was */
    void*          after_stream; /* nullable, as clc_map_job */
    /* out */
    int32_t*       match;        /* nullable host, n_old entries: new row matched by old row q, or -1 */
    double*        X;            /* nullable host, n_new x 3: the rescaled points */
    int            n_old, n_common, n_terms, status;
    double         scale;
} clc_map_align;
int clc_map_align_dev(clc_ctx* ctx, clc_map_align* job);
int clc_map_update_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_align* align);

/* ---- the same step under an a-contrario similarity (new entries under ABI 4) ----------------------------------------------------------
 * OUR OWN STATEMENT, an addition with OpenMVG parity unpinned: it finishes what matchMaps set out to do (its geometric filter is
 * commented out, RobustMatcher.hpp:247-293) and replaces the mean of distance ratios, into which one wrong common feature puts an
 * arbitrary ratio, by the similarity NEW -> OLD of clc_sim3_acransac over the common features.  clc_map_align_dev, the
 * clc_map_update_*_batch_dev entries and matchMaps are unchanged.
 *
 * clc_map_align_sim_dev: the inputs of clc_map_align_dev plus apply, max_iteration (0: 256), seed and precision (as clc_sim3_acransac).
 *   COMMON FEATURES: found exactly as clc_map_align_dev finds them -- the same gather, the same sweep, the same list in ascending old row.
 *   GATHER: one launch of the ordered gather writes X_new | X_old of every common feature into the solve's blocks and leaves the
 *     bounding box of those X_old and then the count in a pinned record.  FIRST HOST WAIT: that record (the NFA tables need the count,
 *     alpha0 the box).  More than 16 384 common features: CLC_ERR_CAPACITY before anything is installed.
 *   SOLVE: the rounds and the refit of clc_sim3_acransac on those pairs, read where the gather left them.
 *   TRANSFORM: one launch over all n_new points into the context's staging buffer and -- where X was asked for -- a pinned mirror:
 *     CLC_SIM_APPLY_SCALE  X' = X * s, one multiply per component; poses go through rescale_pose(s) (the old behaviour, the robust s);
 *     CLC_SIM_APPLY_FULL   X' = s R X + t, every row ((A0 X + A1 Y) + A2 Z) + A3 with A = [sR | t] (sim3_apply_point); a camera
 *                          [R_c | t_c] becomes R_c' = R_c R^T, t_c' = s t_c - R_c' t (sim3_apply_pose), its centre moves to s R C + t.
 *     SECOND HOST WAIT: the transform's record, released last.
 *   NO MODEL (fewer than 4 common features, the acceptance rule failing, a degenerate box): status = CLC_MAP_SIM_NO_MODEL, s = 1, R = I,
 *     t = 0 and the points are installed with their bits unchanged -- the counterpart of CLC_MAP_ALIGN_NO_SCALE.
 *   OUTPUTS: n_old, n_common, n_inliers, inlier (nullable host, n_old bytes of room: 1 for every common feature the model keeps, in list
 *     order), match, X, s, R, t, error_max, min_nfa, iterations, refit, status.  INSTALL, ORDERING, ERRORS and capacity as
 *     clc_map_align_dev (apply outside the two values: CLC_ERR_BAD_ARG); on every error the previous map serves exactly as before.  The
 *     scratch lies in the alignment blocks and the solve's own workspace; no descriptor, point or match is copied in either direction.
 *
 * clc_map_update_sim_batch_dev: the composition.  It is clc_map_update_batch_dev (grow == ba == NULL), clc_map_update_grow_batch_dev
 * (grow given) or clc_map_update_grow_ba_batch_dev (grow and ba given; ba needs grow: CLC_ERR_BAD_ARG otherwise) with the step above
 * in place of the align step: of `sim` threshold, apply, max_iteration, seed, precision, match and inlier are read, its out fields
 * written.  job->X holds the transformed landmarks; the seed poses -- and with grow the resected cameras' -- are transformed under the
 * same apply rule.  No entering pair, no previous map: as in those calls, with status CLC_MAP_SIM_NO_MODEL, s = 1. */
enum { CLC_MAP_SIM_OK = 0, CLC_MAP_SIM_NO_MODEL = 1 };
enum { CLC_SIM_APPLY_SCALE = 0, CLC_SIM_APPLY_FULL = 1 };
typedef struct clc_map_align_sim {
    /* in */
    const void*    d_desc;       /* descriptor block, rows of 64 B, 16-byte aligned */
    const int32_t* d_rows;       /* nullable: new map row i = row d_rows[i] of d_desc; NULL: row i */
    const double*  d_X;          /* n_new x 3, NOT written */
    int            n_new;
    int            threshold;    /* <= 0: 60 (GPUMatcher.hpp:162) */
    int            install;      /* 0: report only, the context's map is left exactly as it was */
    void*          after_stream; /* nullable, as clc_map_job */
    int            apply;        /* CLC_SIM_APPLY_SCALE / CLC_SIM_APPLY_FULL */
    int            max_iteration;/* 0: 256 */
    uint64_t       seed;
    double         precision;    /* +inf: a-contrario threshold */
    /* out */
    int32_t*       match;        /* nullable host, n_old entries: new row matched by old row q, or -1 */
    double*        X;            /* nullable host, n_new x 3: the transformed points */
    uint8_t*       inlier;       /* nullable host, n_old bytes of room: the flags of the n_common common features, in list order */
    int            n_old, n_common, n_inliers, iterations, refit, status;
    double         s, R[9], t[3], error_max, min_nfa;
} clc_map_align_sim;
int clc_map_align_sim_dev(clc_ctx* ctx, clc_map_align_sim* job);
/* (clc_map_update_sim_batch_dev is declared behind clc_map_grow and clc_map_ba, below) */

/* ---- the map grown past the seed pair: resect the other cameras, add their tracks ---------------------------------------------------
 * What Reconstructor::reconstructScene runs after the seed triangulation: `for (auto resectionId : resectionList)
 * resectionCamera(resectionId)` (Reconstructor.hpp:153-154, 259-415), and setupMapDatabase (colocData.hpp:89-121) over the landmarks
 * that loop leaves.  The bundle adjustment behind the loop (:160-161) is the next section's (clc_map_build_grow_ba_dev); the PLY files
 * are NOT covered.  OpenMVG is an empty submodule in the reference
 * tree: as for the tracks and the ratio matcher, the rules below are this project's statement of SfM_Localizer::Localize,
 * TriangulateDLT and AngleBetweenRay, and their parity with OpenMVG is unpinned.  (Later under ABI 4: new entry points only.)
 *
 * STATE, per track t (Landmarks is a map keyed by track id): a landmark X[t] and an observation mask obs[t], one bit per camera; 0 =
 * no landmark.  After the seed triangulation the accepted seed tracks have obs = { seed cam_a, seed cam_b }.  The VALID cameras start
 * as the two seed cameras.  The other cameras are taken in ascending order (:135-139); the k-th of them, camera I:
 *   1. RESECTION LIST (:261-303): the tracks with track_feat[t][I] >= 0 and obs[t] != 0 in ascending track id; pt3D = X[t], pt2D =
 *      get_ud_pixel of the row's position (both position forms of clc_map_camera).  An empty list: the camera fails
 *      (CLC_GROW_NO_TRACKS, :274-277).  More than 16 384 entries: CLC_GROW_CAPACITY, nothing is truncated.
 *   2. SOLVE (:305-307): the a-contrario solve of clc_pnp_acransac on that list -- K of the camera, max_iteration, precision, seed + k
 *      -- through the same launch path, so with its bits.  Success iff more than 2.5 x 3 inliers (HIP_SfM_Localizer::Localize).
 *      DEVIATION 1: the reference stores the pose and goes on even when the resection failed (:316), which would triangulate against
 *      an identity pose.  Here a failed camera is SKIPPED (CLC_GROW_NO_POSE): it does not become valid and adds nothing.
 *   3. GROW (:329-414), I now valid, for every track t with track_feat[t][I] >= 0, each independent of the others:
 *      - obs[t] != 0: the candidate set is { I };
 *      - otherwise the valid cameras J != I with track_feat[t][J] >= 0 in ascending J: until a landmark exists, TriangulateDLT of the
 *        two undistorted pixels under P = K [R|t], accepted iff the ray angle is > 2 degrees, the depth under I > 0, the depth under
 *        J > 0 and |X[2]| < 1000 (:383; grow_point, coloc_amd/csrc/map_math.h); on acceptance X[t] = X and I becomes a candidate;
 *        every J visited, before or after acceptance, is a candidate (:360, :391);
 *      - with a landmark: bit J of obs[t] is set for every candidate J with depth of X[t] under J > 0 and |X[t][2]| < 1000 (:402-411).
 *      RAY ANGLE: between R_I^T b_I and R_J^T b_J, b = ((x_ud - ppx) / focal, (y_ud - ppy) / focal, 1) of the UNDISTORTED pixel,
 *      decided without acos: dot < cos(2 deg) * sqrt(n_I * n_J), one literal constant and the plain sums of map_math.h, so host and
 *      device agree bit for bit.  DEVIATION 2: the two `residual` values the reference computes and never reads are not computed.
 * THE MAP after the last camera: rows in ascending track id over the tracks with obs != 0 -- new landmarks INTERLEAVE with the
 * seed's --, row i = { X, track id, the camera of the LOWEST set bit of obs (obs.begin()), that camera's row, that row's descriptor }.
 * A resected camera below the seed's cam_a takes over the descriptor of every landmark it observes.
 *
 * clc_map_build_grow_dev: clc_map_build_dev with the loop above between the seed triangulation and the install.  job's outputs
 * (map_track, map_row, X, map_n) describe the GROWN map; grow's per-camera outputs are indexed by camera (seed cameras: status
 * CLC_GROW_OK, resected 0, Rt = their seed pose; a camera that failed: Rt zeros).  Every camera with rows needs its d_desc block
 * (CLC_ERR_BAD_ARG otherwise).  The capacity check against MatcherOptions.maxkp is made on the grown map: CLC_ERR_CAPACITY, and the
 * previous map stays.  The host waits, per resected camera, for the resection count and the solve's rounds, and after the last camera
 * for one more word, the grown map's row count; no descriptor, point or track moves through the host.  ORDERING, after_stream and
 * the other errors: as clc_map_build_dev.  With two cameras there is nothing to resect and every output equals clc_map_build_dev's.
 *
 * clc_map_init_grow_batch_dev: clc_map_init_batch_dev with clc_map_build_grow_dev in place of clc_map_build_dev.
 *
 * clc_map_update_grow_batch_dev: clc_map_update_batch_dev on the GROWN stage: the align step's new rows are gathered by the stage's
 * per-row camera list, the capacity check is the grown map's (CLC_ERR_CAPACITY: the previous map stays), and align's rescale
 * multiplies the centres of the resected cameras' poses in grow->Rt as well as the seed poses' (rescaleMap, colocUtils.hpp:213-223).
 *
 * clc_map_resect_build_dev: step 1 alone for `camera` on the per-track state the context's last grown build left (the state AFTER
 * its last camera), enqueue only on `stream`: d_X (3 N) / d_x (2 N) / d_track / d_row (N int32; nullable) with room for
 * job->tracks.rows[camera] entries, *d_n = N.  Of job, tracks.n_cams, tracks.rows[camera] and cams[camera]'s 2-D side and camera are
 * read.  A camera outside [0, n_cams), a null job or d_n, a misaligned pointer: CLC_ERR_BAD_ARG; no grown build on the context since
 * its block was last rewritten (any tracks / map build), or one of another camera count: CLC_ERR_STATE. */
enum { CLC_GROW_OK = 0, CLC_GROW_NO_TRACKS = 1, CLC_GROW_NO_POSE = 2, CLC_GROW_CAPACITY = 3 };
typedef struct clc_map_grow {
    /* in */
    int      max_iteration;            /* 0: 256 */
    uint64_t seed;                     /* k-th resected camera: seed + k */
    double   precision;                /* +inf: a-contrario threshold */
    /* out, per camera index (seed cameras: status CLC_GROW_OK, resected 0, Rt = their seed pose) */
    int      resected[CLC_MAX_BATCH];  /* 1: the camera became valid through a resection */
    int      status[CLC_MAX_BATCH];
    int      n_corr[CLC_MAX_BATCH], n_inliers[CLC_MAX_BATCH];
    double   error_max[CLC_MAX_BATCH];
    double   Rt[CLC_MAX_BATCH][12];
    int      n_seed_rows, n_added;     /* map rows before / landmarks added by the grow */
    /* out, nullable host memory, room as clc_map_job.map_track */
    int32_t* map_cam;                  /* camera of the row's descriptor / map_row */
    uint8_t* map_obs;                  /* observation mask of the row */
} clc_map_grow;
int clc_map_build_grow_dev(clc_ctx* ctx, clc_map_job* job, clc_map_grow* grow);
int clc_map_init_grow_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_grow* grow);
int clc_map_update_grow_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_align* align,
                                  clc_map_grow* grow);
int clc_map_resect_build_dev(clc_ctx* ctx, const clc_map_job* job, int camera, double* d_X, double* d_x, int32_t* d_track, int32_t* d_row,
                             int32_t* d_n, void* stream);

/* ---- the grown map bundle-adjusted: every valid camera's pose and every landmark, by Schur Levenberg-Marquardt ----------------------
 * What Reconstructor::reconstructScene ends with: `if (Adjust) refiner.refinePose(*scene, ba_refine_options, rmse, cov)`
 * (Reconstructor.hpp:160-161; both call sites pass Adjust = true) under intrinsics NONE, extrinsics ADJUST_ALL, structure ADJUST_ALL
 * and ceres::HuberLoss(Square(4.0)) (Refiner.hpp:47-239).  Ceres is absent from the reference tree, so -- as for clc_pnp_refine -- this
 * is a Levenberg-Marquardt of this project's on the same cost, and iterate parity is unpinned.  (Later under ABI 4: new entry points
 * only.)  The arithmetic is stated once, host + device, in coloc_amd/csrc/ba_math.h; the kernels are coloc_amd/csrc/map_ba.hip.
 *
 * COST  1/2 sum rho(|r|^2) over every set bit of obs[t] that names a camera of cam_mask: r = x_ud - (focal (R X + t).hnormalized() +
 *   pp), x_ud the UNDISTORTED pixel (get_ud_pixel, as the grow uses it), rho(s) = s for s <= a^2, 2 a sqrt(s) - a^2 beyond, weights 1 /
 *   a / |r| (clc_pnp_refine's), a = huber_a, 16 where huber_a <= 0.  Intrinsics are constant.  DEVIATION 1: Ceres' Radial_K3 functor
 *   distorts inside the projection, here the observation is undistorted instead; the two agree at k = 0.
 * PARAMETERS  per camera [angle-axis | t], per landmark X; NO block is held constant, as in the reference.  The seven gauge directions
 *   (the similarity that moves cameras and points together) are left to the damping: only gauge-invariant quantities -- the cost, the
 *   reprojections -- mean anything across two runs of different arithmetic.
 * STEP  the Schur complement on the landmarks: S = U + lambda diag(U) - sum_t W (V_t + lambda diag V_t)^-1 W^T over the 6 n_cams <=
 *   48 camera unknowns, dense Cholesky, landmarks by back-substitution.  lambda starts at 1e-4; an accepted step multiplies it by 0.1
 *   (floor 1e-12), a rejected one by 10; a step is rejected when its cost is not finite or not lower, or when a factorisation fails.  A
 *   trial point at depth <= 0 under an observing camera costs +inf.  A landmark with ONE observation stays in (the reference hands it to
 *   Ceres): its V has rank 2 and the damping makes it invertible.
 * STOP  CLC_BA_OK: relative cost decrease < function_tolerance (0: 1e-8, Refiner.hpp:167), or clc_pnp_refine's gradient / parameter
 *   tests; CLC_BA_MAX_ITERATIONS after max_iterations steps (0: 500, Refiner.hpp:159), rejected ones counted; CLC_BA_STALLED at lambda >
 *   1e10.  The result is the last ACCEPTED iterate: cost_final <= cost_initial always; with no accepted step nothing is written.
 *   rmse = sqrt(cost_final / (2 n_obs)) (Refiner.hpp:223).  n_points counts the points with an observation that counts, n_cams the
 *   cameras of cam_mask.  DEVIATION 2: the 6 x 6 covariance block the reference computes here is never read by reconstructScene; it is
 *   not computed.
 * CLC_BA_BAD_START: the cost at the start is not finite (a point at depth <= 0 under an observing camera).  CLC_BA_EMPTY: no
 *   observation counts.  Both return CLC_OK, write nothing, and a composition installs the map unadjusted.
 * DETERMINISM  no floating-point atomics.  The points that carry an observation are first compacted in ascending index; every sum over
 *   points is formed over that list -- 128 consecutive entries per workgroup in order, the workgroups' sums in order.  Two runs on one
 *   input give the same bits; appending or interleaving points with obs = 0 changes no bit, and such points are not touched.
 *
 * clc_ba_dev: the step alone on arrays in device memory.  Rt[c] of the cameras in cam_mask and d_X are read and -- when a step was
 * accepted -- rewritten; cameras outside cam_mask, points without a bit of cam_mask and d_obs / d_x are never written; x of (t, c) is
 * read only where bit c of d_obs[t] is set.  The launches are enqueue-only on the CONTEXT's stream -- an iteration is a chain of five
 * short launches, no kernel waits for another workgroup -- in rounds of several iterations; per round the host waits for ONE pinned
 * record { state, iterations, cost_initial, cost, lambda, poses }, released last behind a system-scope fence.  No array moves through
 * the host.  ORDERING: on return every launch has run and the arrays are final.  after_stream: as clc_map_job -- the launches are
 * ordered behind that stream's work by one event.  The scratch lives in one block of the context that grows on demand: a call that
 * needs more than any call before it synchronises the context's stream and allocates anew.  ERRORS (CLC_ERR_BAD_ARG): a null job,
 * n_cams outside [1, CLC_MAX_BATCH], a negative n_points / max_iterations / function_tolerance, a null or misaligned pointer with
 * n_points > 0, a focal <= 0 of a camera in cam_mask.
 *
 * clc_map_build_grow_ba_dev / clc_map_init_grow_ba_batch_dev / clc_map_update_grow_ba_batch_dev: their _grow_ namesakes with the step
 * between the last camera's grow and the compaction into map rows, over tracks 0 .. n_tracks - 1 of the per-track state (X[t], obs[t])
 * and the valid cameras, pixels through get_ud_pixel from the cameras' 2-D sides.  The discrete outputs -- map_track, map_row,
 * map_cam, map_obs, map_n, n_added, every resection field -- are those of the call without the step; job->X, grow->Rt and
 * job->Rt_seed_a / Rt_seed_b come back refined, and in the update form the align step then rescales the refined points and centres.
 * With no resected camera the two seed cameras and their tracks are adjusted.  Of `ba` max_iterations, huber_a and
 * function_tolerance are read.  A null ba, a negative count or tolerance: CLC_ERR_BAD_ARG before anything is launched; on every error
 * the previous map serves as before.  Ordering, after_stream and the other errors: as the _grow_ calls. */
enum { CLC_BA_OK = 0, CLC_BA_MAX_ITERATIONS = 1, CLC_BA_STALLED = 2 /* lambda > 1e10 */, CLC_BA_BAD_START = 3, CLC_BA_EMPTY = 4 };
typedef struct clc_map_ba {
    /* in */
    int    max_iterations;       /* 0: 500 */
    double huber_a;              /* <= 0: 16 */
    double function_tolerance;   /* 0: 1e-8 */
    /* out */
    int    status, iterations, n_cams, n_points, n_obs;
    double cost_initial, cost_final, rmse;
} clc_map_ba;
typedef struct clc_ba_job {          /* the step alone, on arrays the caller holds in device memory */
    int             n_cams;
    uint32_t        cam_mask;                  /* bit c: camera c is adjusted and its observations count */
    clc_camera_k3   cam[CLC_MAX_BATCH];        /* focal, ppx, ppy are read */
    double          Rt[CLC_MAX_BATCH][12];     /* in / out */
    int             n_points;
    double*         d_X;                       /* n_points x 3, in / out */
    const uint32_t* d_obs;                     /* n_points masks, 0 = no point */
    const double*   d_x;                       /* n_points x n_cams x 2 undistorted pixels, read where the bit is set */
    void*           after_stream;              /* nullable */
    clc_map_ba      ba;
} clc_ba_job;
int clc_ba_dev(clc_ctx* ctx, clc_ba_job* job);
int clc_map_build_grow_ba_dev(clc_ctx* ctx, clc_map_job* job, clc_map_grow* grow, clc_map_ba* ba);
int clc_map_init_grow_ba_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_grow* grow,
                                   clc_map_ba* ba);
int clc_map_update_grow_ba_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_align* align,
                                     clc_map_grow* grow, clc_map_ba* ba);
/* the composition under the a-contrario similarity (clc_map_align_sim above) */
int clc_map_update_sim_batch_dev(clc_ctx* const* ctxs, clc_pair_job* pair_jobs, int n_pairs, clc_map_job* job, clc_map_align_sim* sim,
                                 clc_map_grow* grow /* nullable */, clc_map_ba* ba /* nullable, needs grow */);

/* ---- the map extended in place: untracked matches of two posed views become new landmarks -----------------------------------------------
 * Every entry above that produces landmarks REPLACES the map: new landmark identities, a new scale, and clc_map_align_dev / clc_sim3_* to
 * tie the new map to the old one.  Between rebuilds the frame loop already holds what it takes to ADD landmarks where the cameras now
 * look: two views with poses (clc_track_prior_dev / clc_track_localize_dev) and each view's map match (clc_match_map_binned_unique_dev),
 * which says which keypoints are landmarks already.  clc_map_extend_dev joins them and appends to the context's map: old rows keep their
 * index, their descriptor and their coordinates, so nothing has to be aligned and every list that names map rows stays valid.  The
 * reference has no such step: like the guided, binned, unique and prior entries this is THIS library's statement, parity with nothing
 * is pinned, and no existing entry changes.  (Later under ABI 4: new entry points only.)
 *
 * THE RULE (coloc_amd/csrc/extend_math.h, host and device, over guided_math.h, unique_math.h and map_math.h as they stand).  View A is
 * the query side, view B the train side.  A view: n descriptor rows of 64 bytes (d_desc), clipped by d_count[0] where given; positions
 * as d_kps or d_feat + feat_stride, exactly one; its clc_camera_k3; its pose Rt (HOST, 12 doubles, [R|t] row-major, world to camera);
 * d_track (nullable, n int32 on the device): the map row of every keypoint or -1, as clc_match_map_* leaves it; null = no row tracked.
 *   1 F          clc_fundamental_from_poses: R = R_b R_a^T, t = t_b - R t_a, E = [t]x R, F = K_b^-T E K_a^-1 with K = { focal, 0, ppx; 0,
 *                focal, ppy; 0, 0, 1 }, in fp64, one fixed operation order, no contraction, on the host.  x_b^T F x_a = 0 in undistorted
 *                pixels: clc_guided_job.F's orientation and units.  It comes back in job.F.
 *   2 guided     clc_match_guided_dev's rule and launches under that F with `band` and `threshold`, the distances kept.
 *   3 mask       entry q with t = match[q] >= 0 becomes -1 if d_track_a[q] >= 0 (q is a landmark already), if d_track_b[t] >= 0 (q's
 *                best row inside the band is a landmark already: q is most likely an unmatched observation of that landmark, and its
 *                second choice would plant a duplicate -- which is why the mask stands BEHIND the sweep and not in its gate), or if
 *                best[q] > max_distance (the guided rule accepts a lone candidate at any distance).  max_distance in [0, 512].
 *   4 one-to-one clc_match_unique_dev's rule and launches on the masked list, nt = B's rows.
 *   5 point      for every surviving (q, t): both positions through get_ud_pixel in fp64 (the track kernel's bits), then the grow rule
 *                of one landmark (Reconstructor.hpp:383; grow_point, map_math.h) with camera A in the place of the resected camera:
 *                accepted iff the ray angle is over 2 degrees, X is finite, both depths are positive and |X[2]| < 1000.
 *   6 append     the accepted entries in ASCENDING q become map rows map_n + k, k = 0, 1, ..., while map_n + k < MatcherOptions.maxkp.
 *                Row map_n + k holds X in the map's points and A's descriptor row q in the map's rows (A is the lower camera: the rule
 *                of the grown map); (q, t) goes into the output lists.  Entries past the capacity are dropped and counted (n_dropped),
 *                not an error: the order is fixed, so the truncation is reproducible.  Old rows are never rewritten.  update_tracks != 0:
 *                d_track_a[q] and d_track_b[t] of every APPENDED entry are set to its new row, so a later job that shares a view skips
 *                them; no other entry of d_track_* is written.
 *   7 Degenerate cases add nothing and return CLC_OK, each by rules 1 - 6: two views with one centre where t comes out 0 (F = 0, no
 *     query has a line), a.n == 0 or b.n == 0, a map at capacity (everything accepted is dropped and counted).
 *
 * clc_map_extend_dev runs on the CONTEXT's stream (after_stream: as clc_map_job, one event, no host synchronisation): the guided prep
 * and sweep, the mask (one thread per query), the filter's three launches, the point launch (one thread per query) and ONE workgroup
 * that appends by the ordered compaction and publishes { n_added, n_dropped } in pinned memory last, behind a system-scope fence.  The
 * host waits for that one word, once per call.  OUTPUTS: d_new_q / d_new_t (nullable, device, room for a.n) and new_q / new_t / X
 * (nullable, host, room for a.n entries / 3 a.n doubles): the appended (q, t) and their points, n_added of each; F; map_n_before (the
 * map's rows when the job ran), n_guided (entries the guided match accepted, before the mask), n_added, n_dropped, status.
 * The context's map points are brought to MatcherOptions.maxkp rows first, contents kept; a call at a size no call before it had may
 * grow scratch, which synchronises the context's stream.
 * ORDERING, as clc_map_build_dev: on return the map serves clc_match_map_*, clc_match_map_guided_* / _binned_*, clc_track_* with
 * map_n_before + n_added rows.  Work on other streams that reads the map while the call runs is the caller's to order; the old rows are
 * not written, so such work is correct under either count.
 * clc_map_extend_batch_dev: n_jobs in [0, CLC_MAX_TRACK_PAIRS] on one context, enqueued in order on the one stream; job k sees job
 * k - 1's rows and d_track updates, the running row count lives in a device word, and the host still waits once.  The results equal
 * the single calls made in that order.
 * ERRORS, all before anything is enqueued: a null context, job, descriptor block (n > 0) or a negative n, both or neither position
 * form, a misaligned pointer (descriptor rows: 16 bytes), a non-positive focal, a band that is not finite and positive, max_distance
 * outside [0, 512], n_jobs out of range: CLC_ERR_BAD_ARG; a context without matcher options, without a map (no clc_set_map / build),
 * or whose map points are not exactly its map rows (the partially-owned state clc_track_localize_dev refuses): CLC_ERR_STATE -- a map
 * of 0 rows with its points cleared is an empty map and is extendable; n > 2^22: CLC_ERR_CAPACITY.  The map is as it was.
 *
 * clc_fundamental_from_poses: rule 1 alone, host arithmetic, no context.  Null pointer or a focal that is not positive: CLC_ERR_BAD_ARG.
 * clc_append_map_points: n more points behind the points of a context that holds ONLY points (the localizer's, whose tracks name the
 * matcher's rows): the points it has are kept, the new ones follow.  A context that holds map rows is extended by clc_map_extend_dev
 * alone (CLC_ERR_STATE), so rows and points cannot part ways.  Synchronises the context's stream, as clc_set_map_points. */
typedef struct clc_extend_view {
    const void*         d_desc;         /* n rows of 64 bytes, 16-byte aligned */
    int                 n;
    const uint32_t*     d_count;        /* nullable, as clc_pair_job */
    const clc_keypoint* d_kps;          /* or */
    const float*        d_feat;
    int                 feat_stride;
    clc_camera_k3       cam;
    double              Rt[12];         /* host: the view's pose */
    int32_t*            d_track;        /* nullable, n, device: map row or -1; written where update_tracks != 0 */
} clc_extend_view;
typedef struct clc_map_extend {
    /* in */
    clc_extend_view a, b;
    float           band;               /* pixels */
    int             threshold;
    int             max_distance;       /* [0, 512] */
    int             update_tracks;
    void*           after_stream;       /* nullable */
    /* out, nullable: device, room for a.n */
    int32_t*        d_new_q;
    int32_t*        d_new_t;
    /* out, nullable: host, room for a.n (X: 3 a.n) */
    int32_t*        new_q;
    int32_t*        new_t;
    double*         X;
    /* out */
    double          F[9];
    int             map_n_before, n_guided, n_added, n_dropped, status;
} clc_map_extend;
int clc_map_extend_dev(clc_ctx* ctx, clc_map_extend* job);
int clc_map_extend_batch_dev(clc_ctx* ctx, clc_map_extend* jobs, int n_jobs);   /* n_jobs in [0, CLC_MAX_TRACK_PAIRS], in order, one stream */
int clc_fundamental_from_poses(const clc_camera_k3* cam_a, const double* Rt_a, const clc_camera_k3* cam_b, const double* Rt_b, double* F);
int clc_append_map_points(clc_ctx* ctx, const double* h_X, int n);

/* ---- the map culled in place: observation statistics per row, drop, compact, remap ----------------------------------------------------
 * clc_map_extend_dev only ever adds rows; once the map holds MatcherOptions.maxkp of them it counts what it could not add.  A rebuild
 * (clc_map_update_*) forgets old rows, at the price of new identities and a new scale.  The other half of map maintenance is here: the
 * context keeps, per map row, how often the row's landmark projected into a frame (visible), how often the frame's map match then found
 * it (found) and when it was last in view (last_view), as a by-product of the frame's own match; clc_map_cull_dev drops rows by those
 * counters, compacts rows, points and counters in order and returns the remap, under which every list that names map rows stays valid.
 * The reference has no such step: like the guided, binned, unique, prior and extend entries this is THIS library's statement, parity
 * with nothing is pinned, and no existing entry changes.  (Later under ABI 4: new entry points only.)
 *
 * THE RULE (coloc_amd/csrc/cull_math.h, host and device, over proj_math.h and get_ud_pixel as they stand).
 *   STATE    three uint32 per map row -- visible, found, last_view -- on the device; epoch (uint32) and stat_rows (the rows the counters
 *            cover) on the host side of the context.
 *   RESET    whatever REPLACES the map's rows (clc_set_map, the installs of clc_map_build_* / clc_map_init_* / clc_map_update_* /
 *            clc_map_align_*, an empty map installed) sets stat_rows = 0 and epoch = 0: row identities are new.
 *   COVER    every observe, cull or clc_map_stats_get call begins by giving rows [stat_rows, map_n) -- the rows clc_map_extend_dev
 *            appended -- visible = found = 0 and last_view = epoch (as it stands before the call increments it); then stat_rows = map_n.
 *   IN VIEW  lo = margin, hi_x = (float)(width - 1) - margin, hi_y = (float)(height - 1) - margin, formed once on the host;
 *            cull_in_view(u, v) = u >= lo && u <= hi_x && v >= lo && v <= hi_y in float.  NaN is false: a landmark without a projection
 *            is never in view.  The rectangle is tested in UNDISTORTED pixels, a stated deviation (the one the projection gate of
 *            clc_match_map_guided_dev makes).
 *   OBSERVE  one view: p(r) = proj_point(Rt, { focal, ppx, ppy }, X[r]).  in_view(r) = cull_in_view(p(r)).  hit(r) iff some keypoint
 *            q < n (clipped by d_count[0] where given) has d_track[q] == r and proj_in_radius(xq, yq, p(r), gate * gate), (xq, yq) the
 *            keypoint through get_ud_pixel in fp64 rounded once to float: the bits the prep launch of clc_match_map_guided_dev
 *            produces.  An entry of d_track outside [0, map_n) names no row.  visible[r] += in_view(r); found[r] += in_view(r) &&
 *            hit(r), so found <= visible always; last_view[r] = epoch where in_view(r).  ONE call is ONE epoch, whether it carries one
 *            view or a batch: epoch is incremented once BEFORE stamping, and a row counts once per view of the batch that sees it.
 *   DROP     cull_drops = flagged || (visible >= min_visible && (uint64)found * den < (uint64)num * visible)
 *                                 || (max_idle > 0 && (uint32)(epoch - last_view) > max_idle).
 *            Rows younger than min_visible are safe from the ratio test; max_idle == 0 switches the idle test off; d_flagged (nullable,
 *            one byte per row, device) is the caller's own list -- say, landmarks with a large residual after clc_ba_dev.  The customary
 *            rule is min_visible 8, num / den 1 / 4, max_idle 0 (clc_map_cull_rule_default): a quarter of the frames that should see a
 *            point.  These values are UNTUNED.
 *   REMAP    remap[r] = the number of kept rows below r where row r is kept, -1 otherwise: kept rows stay in ASCENDING old order.  New
 *            row remap[r] takes old row r's point (3 doubles), descriptor (64 bytes) and three counters, bit for bit.  A track-list
 *            entry e becomes remap[e] if 0 <= e < map_n_before, -1 otherwise.
 *
 * clc_map_observe_dev / clc_map_observe_batch_dev (n_views in [0, CLC_MAX_BATCH], one job per view) enqueue on the CONTEXT's stream
 * behind each job's after_stream (one event, as clc_map_job) and return: there is NO host wait, this runs every frame for every camera.
 * Two launches whatever the batch: one thread per (keypoint, view) for the hits -- it reads d_track[q] and recomputes that row's
 * proj_point, the same function, hence the same bits -- and one thread per (map row, view) for in_view and the counters, which are
 * 32-bit integer adds and commute.  d_counts (nullable, device, 2 int32 per view): { n_in_view, n_hit } of the view.  On return
 * job.epoch is the call's epoch and job.map_n the rows it covered.
 * clc_map_cull_dev is a chain on the context's stream in which nothing waits for another workgroup: ONE workgroup of 1 024 runs
 * cull_drops and the ordered compaction and writes the remap; a wide gather moves rows, points and counters into the context's OTHER
 * buffers (never in place); a launch remaps up to CLC_MAX_BATCH track lists in place; { n_kept, n_dropped } comes out in ONE pinned word
 * last.  The host waits for that word once, then installs by buffer swaps, exactly as clc_map_update_batch_dev installs.  OUTPUTS: d_remap
 * (nullable, device, room for map_n_before), h_remap (nullable, host, the same), map_n_before, n_kept, n_dropped, and of the dropped rows
 * how many fell to each clause (n_flagged, n_ratio, n_idle: the first clause that fires in the order written), status.
 * A cull rewrites the row numbering: the per-track state of the last grown build ends (clc_map_resect_build_dev answers
 * CLC_ERR_STATE), and whatever the CALLER holds by row index -- d_owner lists, the cell lists of clc_map_bin_build_dev, host-side
 * databases -- must follow the remap or be rebuilt.  The context itself caches nothing else across calls: the binned table and the
 * projections are rebuilt by every match call.
 * DEGENERATE cases, each by the rules and CLC_OK: a map of 0 rows (n_kept = 0); nothing dropped (the identity remap); everything dropped
 * (the map has 0 rows and its points are cleared: the extendable empty map of clc_map_extend_dev).
 * ORDERING: on return of clc_map_cull_dev the map serves every entry with n_kept rows.  Work on other streams that reads the map while
 * the call runs is the caller's to order.
 * ERRORS, all before anything is enqueued, the map and the statistics as they were: a null context or job, den <= 0, num < 0,
 * min_visible < 1, a gate or margin that is negative or not finite (or whose square is not), a non-positive width / height / focal,
 * both or neither position form, a non-finite Rt, a misaligned pointer, more lists or views than CLC_MAX_BATCH, a negative n:
 * CLC_ERR_BAD_ARG; a context without matcher options, without a map, or whose points are not exactly its rows (the state
 * clc_track_localize_dev refuses): CLC_ERR_STATE.
 *
 * clc_map_stats_get: the counters out for tests and tools (pointers nullable; room for map_n words each); covers new rows first and
 * synchronises the context's stream.  A context without a map: rows = 0.
 * clc_cull_map_points: the companion of clc_append_map_points for a context that holds ONLY points (the localizer's): the points
 * compacted by a host remap of n == its points.  The kept entries must read 0, 1, 2, ... in ascending order, else CLC_ERR_BAD_ARG; a
 * context that holds rows is culled by clc_map_cull_dev alone (CLC_ERR_STATE), so rows and points cannot part ways.  Synchronises. */
typedef struct clc_observe_view {
    int                 n;              /* planned keypoints */
    const uint32_t*     d_count;        /* nullable, as clc_track_job */
    const clc_keypoint* d_kps;          /* or */
    const float*        d_feat;
    int                 feat_stride;
    clc_camera_k3       cam;
    double              Rt[12];         /* host: the frame's pose */
    const int32_t*      d_track;        /* nullable, n, device: the frame's map match (map row or -1); null: nothing is found */
    int32_t*            d_counts;       /* nullable, device, 2: { n_in_view, n_hit } */
} clc_observe_view;
typedef struct clc_map_observe {
    /* in */
    clc_observe_view view;
    int              width, height;     /* the image */
    float            gate;              /* pixels: a hit lies within it of the landmark's projection */
    float            margin;            /* pixels */
    void*            after_stream;      /* nullable */
    /* out */
    uint32_t         epoch;
    int              map_n, status;
} clc_map_observe;
typedef struct clc_map_cull {
    /* in */
    int              min_visible, num, den;
    uint32_t         max_idle;
    const uint8_t*   d_flagged;         /* nullable, device, one byte per map row */
    int32_t*         d_track[CLC_MAX_BATCH];   /* lists that name map rows, device, rewritten in place */
    int              track_n[CLC_MAX_BATCH];
    int              n_lists;
    void*            after_stream;      /* nullable */
    /* out, nullable: room for map_n_before */
    int32_t*         d_remap;
    int32_t*         h_remap;
    /* out */
    int              map_n_before, n_kept, n_dropped, n_flagged, n_ratio, n_idle, status;
} clc_map_cull;
int clc_map_observe_dev(clc_ctx* ctx, clc_map_observe* job);
int clc_map_observe_batch_dev(clc_ctx* ctx, clc_map_observe* jobs, int n_views);   /* n_views in [0, CLC_MAX_BATCH]: ONE epoch */
int clc_map_cull_dev(clc_ctx* ctx, clc_map_cull* job);
int clc_map_cull_rule_default(clc_map_cull* job);                                   /* min_visible 8, num / den 1 / 4, max_idle 0 */
int clc_map_stats_get(clc_ctx* ctx, uint32_t* h_visible, uint32_t* h_found, uint32_t* h_last_view, uint32_t* epoch, int* rows);
int clc_cull_map_points(clc_ctx* ctx, const int32_t* h_remap, int n);

/* ---- fusion (host arithmetic; no GPU work) ---------------------------------------------------------
 * Covariance intersection of two 3-D position estimates as CoLoC fuses intra- and inter-camera poses
 * (include/coloc/CovIntersection.hpp:24-49, called at include/coloc/coloc.hpp:362-389): omega in [0,1]
 * minimising trace(inv(inv(CA) + inv(CB) - inv(omega CA + (1-omega) CB))) to 1e-3, then the fused
 * covariance (9, row-major) and position (3).  Same code as coloc_amd/host/HIPCovIntersection.hpp, exported
 * for hosts that bind the C ABI only.  ctx may be NULL. */
int clc_cov_intersection(const double* CA, const double* CB, const double* ca, const double* cb,
                         double* omega, double* cov_fused, double* pos_fused);

#ifdef __cplusplus
}
#endif
#endif /* COLOC_HIP_H */

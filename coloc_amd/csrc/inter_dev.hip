// inter_dev.hip -- the inter-camera step of ColoC::interPoseEstimator (reference include/coloc/coloc.hpp:296-340) from device memory
// (include/coloc_hip.h: clc_inter_pose_dev, clc_inter_pose_batch_dev, clc_inter_front_dev).  clc_inter_pose_batch (inter_pose.hip) takes
// the pair's correspondences on the host and runs the two halves of the geometry there (inter_geometry.cpp); here the pair never leaves
// the GPU: the pair gather and the five-point filter of clc_pair_filter_batch_dev, then
//   inter_front_kernel   inter_relative: the chirality vote over the four motions of E, the closed-form two-ray depths, the ordered
//                        compaction of the points in front of both cameras -> the temporary map Xt, x2f, corr, the descriptor row of
//                        each kept point, and a pinned record {n_front, chosen motion, stage}
//   gather_rows_kernel + the K2NN sweep (map_sweep_enqueue, inter_pose.hip; the reference's chain only)
//   inter_scale_kernel   the common-feature walk and inter_scale_pose: ratios, median, screen, the consecutive-distance scale rule, the
//                        composed first pose and the temporary map in world coordinates, straight into the refinement's layout
//   pnp_refine_kernel    (pnp.hip) behind a device go / no-go word
// Both kernels follow gather.hip: one launch for a batch, blockIdx.y = job, ONE workgroup per job (inliers <= 16 384, map_n a few
// thousand: latency-bound), the ordered compaction of wg_compact.h.  All arithmetic is fp64 and is the statements of inter_math.h, the ones
// inter_geometry.cpp runs on the host: the results have the host's bits by construction.  The host waits for ONE number per job,
// n_front (the sweep's train count and the refinement's N are host arguments); nothing sized by N or map_n is copied in either direction.
#include "clc_ctx.h"
#include "inter_math.h"
#include "wg_compact.h"
#include "../host/HIPRobustMatcher.hpp"      // hipgeom::motion_from_essential (host arithmetic: nine numbers in, four motions out)

#include <algorithm>
#include <cstring>
#include <vector>

namespace clc {

namespace {

constexpr int kInterThreads = 1024;
constexpr int kSumChunk = 1024;              // terms of the scale rule staged in LDS per pass of the sequential sum

// one camera of a pair as the kernels take it: K = { focal, 0, ppx; 0, focal, ppy; 0, 0, 1 } (Pinhole_Intrinsic_Radial_K3::K())
struct InterCam { double focal, ppx, ppy; };

struct FrontJobDev {
    double R[2][9], t[4][3];                 // the four motions of E: candidate c = [ R[c & 1] | t[c] ] (motion_from_essential's order)
    InterCam k1, k2;
    const double* x1; const double* x2;      // the pair's correspondences, undistorted pixels (n of them)
    const int32_t* inliers;                  // the filter's inlier list (nullable: 0 .. n_inliers - 1)
    const int32_t* rows;                     // nullable: correspondence -> descriptor row of the camera with the lower id (pair_q / pair_t)
    double* Xt; double* x2f; int32_t* corr; int32_t* first;      // out (room for n_inliers points each; first nullable)
    int32_t* rec;                            // out: { n_front, chosen, stage, ready } -- device or pinned memory
    int32_t* list;                           // nullable scratch (n_inliers): the vote leaves the list here, the compaction reads it from
                                             // device memory instead of a second time from the filter's pinned block
    int32_t n, n_inliers;
};
// By value: a job of E's motions is 376 B, eight fit the 4 KB kernarg segment beside its hidden arguments.  full: job 0 takes four
// caller-chosen motions [R|t] (3 x 4 row-major) from cand0 instead (clc_inter_front_dev).
struct FrontJobs { FrontJobDev j[kMaxBatch]; double cand0[4][12]; int32_t full; };
static_assert(sizeof(FrontJobs) <= 4096 - 256, "FrontJobs is passed as a kernel argument: it must stay within the 4 KB kernarg segment");

struct ScaleJobDev {
    double Rs[12];                           // the source camera's [R|t]
    double Rb[9], tb[3];                     // the motion the chirality vote chose
    InterCam k2;
    const double* Xt; const int32_t* corr; int32_t nf;
    const int32_t* match;                    // the chain: d_match[map_n], global map point -> temporary map point or -1 (else null)
    const int32_t* map_match_a; const int32_t* pair_q;       // the shortcut: camera A's own match against the map, read through pair_q[corr[k]]
    int32_t* cg; int32_t* ck; int32_t* kg; int32_t* kk; double* ratio; double* term;      // scratch: max(map_n, nf) entries each
    double* Rt; double* Xw; double* K; int32_t* valid;       // out: the refinement's d_Rt_in (12), d_X (3 nf), d_K (16), d_valid
    InterScaleRec* rec;                      // out, pinned
};
struct ScaleJobs { ScaleJobDev j[kMaxBatch]; const double* map_X; int32_t map_n; };
static_assert(sizeof(ScaleJobs) <= 4096 - 256, "ScaleJobs is passed as a kernel argument: it must stay within the 4 KB kernarg segment");

// pixel -> normalised camera plane: K[0] = K[4] = focal, K[1] = 0 (inter_math.h keeps the product)
__device__ __forceinline__ void cam_plane(const InterCam& c, const double x, const double y, double* n) { normalise_px(c.focal, 0.0, c.ppx, c.focal, c.ppy, x, y, n); }

// candidate c of the job as [R|t], 3 x 4 row-major (c is the same in every thread)
__device__ __forceinline__ void candidate(const FrontJobs& jobs, const FrontJobDev& jb, const int c, double* Rt)
{
    if (jobs.full) { for (int e = 0; e < 12; ++e) Rt[e] = jobs.cand0[c][e]; return; }
    for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) Rt[4 * r + q] = jb.R[c & 1][3 * r + q]; Rt[4 * r + 3] = jb.t[c][r]; }
}

__global__ __launch_bounds__(kInterThreads) void inter_front_kernel(const FrontJobs jobs)
{
    const FrontJobDev& jb = jobs.j[blockIdx.y];
    __shared__ uint32_t s_wave[kInterThreads / 64];
    __shared__ uint32_t s_cnt[4][kInterThreads / 64];
    __shared__ int s_best, s_best_cnt;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int ni = jb.n_inliers;
    int stage = CLC_INTER_OK;
    if (ni < 13) stage = CLC_INTER_NO_MODEL;             // (the same in every thread)
    uint32_t n_front = 0;
    if (stage == CLC_INTER_OK) {
        if (lane == 0) for (int c = 0; c < 4; ++c) s_cnt[c][wave] = 0;
        // the chirality vote: per candidate, the inliers in front of both cameras (each wave keeps its own counts: no atomics)
        for (int k0 = 0; k0 < ni; k0 += kInterThreads) {
            const int k = k0 + (int)tid;
            int i = -1;
            if (k < ni) { i = jb.inliers ? jb.inliers[k] : k; if (i < 0 || i >= jb.n) i = -1; }       // (an index outside the block: never in front)
            if (jb.list && k < ni) jb.list[k] = i;
            double n1[2] = { 0.0, 0.0 }, n2[2] = { 0.0, 0.0 };
            if (i >= 0) {
                cam_plane(jb.k1, jb.x1[2 * (size_t)i], jb.x1[2 * (size_t)i + 1], n1);
                cam_plane(jb.k2, jb.x2[2 * (size_t)i], jb.x2[2 * (size_t)i + 1], n2);
            }
            for (int c = 0; c < 4; ++c) {
                double Rt[12], d1;
                candidate(jobs, jb, c, Rt);
                const bool front = i >= 0 && two_ray_depths(Rt, n1, n2, &d1);
                const uint64_t b = __ballot(front);
                if (lane == 0) s_cnt[c][wave] += (uint32_t)__popcll(b);
            }
        }
        __syncthreads();
        if (tid == 0) {
            // the FIRST candidate with the strictly largest count (the host's cnt > best_cnt)
            int best = -1, best_cnt = -1;
            for (int c = 0; c < 4; ++c) {
                int cnt = 0;
                for (int w = 0; w < kInterThreads / 64; ++w) cnt += (int)s_cnt[c][w];
                if (cnt > best_cnt) { best_cnt = cnt; best = c; }
            }
            s_best = best; s_best_cnt = best_cnt;
        }
        __syncthreads();
        if (s_best < 0 || s_best_cnt < 8) stage = CLC_INTER_NO_RELATIVE_POSE;
    }
    if (stage == CLC_INTER_OK) {
        // the temporary map (source camera's frame, unit baseline): the winner's front points in the inlier list's order
        double Rt[12];
        candidate(jobs, jb, s_best, Rt);
        uint32_t base = 0;
        for (int k0 = 0; k0 < ni; k0 += kInterThreads) {
            const int k = k0 + (int)tid;
            int i = -1;
            if (k < ni) { i = jb.list ? jb.list[k] : (jb.inliers ? jb.inliers[k] : k); if (i < 0 || i >= jb.n) i = -1; }       // (list[k]: this thread's own store)
            double n1[2] = { 0.0, 0.0 }, n2[2] = { 0.0, 0.0 }, d1 = 0.0, u2[2] = { 0.0, 0.0 };
            bool front = false;
            if (i >= 0) {
                u2[0] = jb.x2[2 * (size_t)i]; u2[1] = jb.x2[2 * (size_t)i + 1];
                cam_plane(jb.k1, jb.x1[2 * (size_t)i], jb.x1[2 * (size_t)i + 1], n1);
                cam_plane(jb.k2, u2[0], u2[1], n2);
                front = two_ray_depths(Rt, n1, n2, &d1);
            }
            uint32_t total;
            const uint32_t w = base + ordered_slot<kInterThreads>(front, s_wave, &total);
            if (front) {                                 // (w < n_inliers: the blocks hold that many)
                jb.Xt[3 * (size_t)w] = n1[0] * d1; jb.Xt[3 * (size_t)w + 1] = n1[1] * d1; jb.Xt[3 * (size_t)w + 2] = d1;
                jb.x2f[2 * (size_t)w] = u2[0]; jb.x2f[2 * (size_t)w + 1] = u2[1];
                jb.corr[w] = i;
                if (jb.first) jb.first[w] = jb.rows ? jb.rows[i] : i;
            }
            base += total;
        }
        n_front = base;
    }
    // the record comes out last: every wave's stores are complete and visible system-wide before the word the host polls changes
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        jb.rec[0] = (int32_t)n_front;
        jb.rec[1] = stage == CLC_INTER_OK ? s_best : -1;
        jb.rec[2] = stage;
        __hip_atomic_store(&jb.rec[3], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The k-th smallest (k from 0) of n NON-NEGATIVE doubles, exactly: a radix select on the bit patterns (which order like the values), eight
// passes of eight bits, a 256-bin LDS histogram per pass; wave 0 finds the bin that holds rank k by a scan over the lanes' four-bin sums.
__device__ double radix_select(const double* __restrict__ v, const uint32_t n, uint32_t k, uint32_t* s_hist, uint32_t* s_pick)
{
    const uint32_t tid = threadIdx.x;
    uint64_t prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += kInterThreads) {
            const uint64_t key = (uint64_t)__double_as_longlong(v[i]);
            if ((key & mask) == prefix) atomicAdd(&s_hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {
            const uint32_t h0 = s_hist[4 * tid], h1 = s_hist[4 * tid + 1], h2 = s_hist[4 * tid + 2], h3 = s_hist[4 * tid + 3];
            uint32_t incl = h0 + h1 + h2 + h3;
            const uint32_t own = incl;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(incl, d, 64);
                if ((int)tid >= d) incl += up;
            }
            const uint32_t excl = incl - own;
            if (excl <= k && k < incl) {                 // exactly one lane (k < n = the total)
                uint32_t r = k - excl, bin = 4 * tid;
                if (r >= h0) { r -= h0; ++bin; if (r >= h1) { r -= h1; ++bin; if (r >= h2) { r -= h2; ++bin; } } }
                s_pick[0] = bin; s_pick[1] = r;
            }
        }
        __syncthreads();
        prefix |= (uint64_t)s_pick[0] << shift;
        mask |= (uint64_t)255u << shift;
        k = s_pick[1];
        __syncthreads();                                 // (s_pick and s_hist are written again by the next pass)
    }
    return __longlong_as_double((long long)prefix);
}

__global__ __launch_bounds__(kInterThreads) void inter_scale_kernel(const ScaleJobs jobs)
{
    const ScaleJobDev& jb = jobs.j[blockIdx.y];
    __shared__ uint32_t s_wave[kInterThreads / 64];
    __shared__ uint32_t s_hist[256], s_pick[2];
    __shared__ double s_term[kSumChunk];
    __shared__ double s_scale;
    __shared__ int s_stage;
    const uint32_t tid = threadIdx.x;
    const double* Rs = jb.Rs;
    const double* Xt = jb.Xt;
    const uint32_t nf = jb.nf > 0 ? (uint32_t)jb.nf : 0u, map_n = jobs.map_n > 0 ? (uint32_t)jobs.map_n : 0u;
    int stage = CLC_INTER_OK;
    // 1. the features the temporary map shares with the global map, in the order the scale rule walks them: ascending map point q (the
    //    chain: commonFeatures of the sweep) or ascending front position (the shortcut), and their depth ratios
    const uint32_t n_walk = jb.match ? map_n : nf;
    uint32_t n_com = 0, n_raw = 0;
    for (uint32_t e0 = 0; e0 < n_walk; e0 += kInterThreads) {
        const uint32_t e = e0 + tid;
        int32_t gi = -1, k = -1;
        bool raw = false;
        if (e < n_walk) {
            if (jb.match) { k = jb.match[e]; gi = (int32_t)e; raw = k >= 0; }
            else { k = (int32_t)e; gi = jb.map_match_a[jb.pair_q[jb.corr[e]]]; }
        }
        const bool ok = k >= 0 && (uint32_t)k < nf && gi >= 0 && (uint32_t)gi < map_n;      // (an index outside the map: not a map feature)
        if (jb.match) n_raw += (uint32_t)__syncthreads_count(raw);
        uint32_t total;
        const uint32_t c = n_com + ordered_slot<kInterThreads>(ok, s_wave, &total);
        if (ok) {
            jb.cg[c] = gi; jb.ck[c] = k;
            jb.ratio[c] = depth_ratio(Rs, jobs.map_X + 3 * (size_t)gi, Xt + 3 * (size_t)k);
        }
        n_com += total;
    }
    uint32_t n_common = n_com, n_keep = 0;
    if (n_com < 8) stage = CLC_INTER_NO_SCALE;
    __syncthreads();                                     // the lists of this workgroup are read back below (global memory, one workgroup)
    if (stage == CLC_INTER_OK) {
        // 2. the median of the ratios (the two middle order statistics), the screen |ratio / med - 1| < 0.2
        const double hi = radix_select(jb.ratio, n_com, n_com / 2, s_hist, s_pick);
        double med = hi;
        if (!(n_com & 1u)) { const double lo = radix_select(jb.ratio, n_com, n_com / 2 - 1, s_hist, s_pick); med = 0.5 * (lo + hi); }
        for (uint32_t c0 = 0; c0 < n_com; c0 += kInterThreads) {
            const uint32_t c = c0 + tid;
            const bool ok = c < n_com && fabs(jb.ratio[c] / med - 1.0) < 0.2;
            uint32_t total;
            const uint32_t w = n_keep + ordered_slot<kInterThreads>(ok, s_wave, &total);
            if (ok) { jb.kg[w] = jb.cg[c]; jb.kk[w] = jb.ck[c]; }
            n_keep += total;
        }
        n_common = n_keep;
        if (n_keep < 8) stage = CLC_INTER_NO_SCALE;
        __syncthreads();
    }
    if (stage == CLC_INTER_OK) {
        // 3. colocUtils.hpp:201-204 over consecutive kept features: the terms in parallel, their SUM by one lane in list order (the host's
        //    sum is sequential: the bits depend on it).  A term that the rule's guard drops is stored as -1 (scale_term).
        const uint32_t n_terms = n_keep - 1;
        for (uint32_t k = tid; k < n_terms; k += kInterThreads) {
            jb.term[k] = scale_term(jobs.map_X + 3 * (size_t)jb.kg[k], jobs.map_X + 3 * (size_t)jb.kg[k + 1], Xt + 3 * (size_t)jb.kk[k], Xt + 3 * (size_t)jb.kk[k + 1]);
        }
        __syncthreads();
        double sum = 0.0; uint32_t good = 0;                         // (thread 0's)
        for (uint32_t k0 = 0; k0 < n_terms; k0 += kSumChunk) {
            const uint32_t m = n_terms - k0 < (uint32_t)kSumChunk ? n_terms - k0 : (uint32_t)kSumChunk;
            for (uint32_t k = tid; k < m; k += kInterThreads) s_term[k] = jb.term[k0 + k];
            __syncthreads();
            if (tid == 0)
                for (uint32_t k = 0; k < m; ++k) { const double v = s_term[k]; if (!(v < 0.0)) { sum += v; ++good; } }
            __syncthreads();
        }
        if (tid == 0) { double scale; s_stage = scale_from_sum(sum, good, &scale); s_scale = scale; }
        __syncthreads();
        stage = s_stage;
    }
    double scale = 0.0;
    if (stage == CLC_INTER_OK) {
        scale = s_scale;
        // the destination's pose through the source
        if (tid < 12) jb.Rt[tid] = compose_pose_entry(jb.Rb, jb.tb, Rs, scale, (int)tid >> 2, (int)tid & 3);
        if (tid >= 64 && tid < 80) {
            const int e = (int)tid - 64;
            jb.K[e] = (e == 0 || e == 4) ? jb.k2.focal : (e == 2 ? jb.k2.ppx : (e == 5 ? jb.k2.ppy : (e == 8 ? 1.0 : 0.0)));
        }
        // the temporary map in world coordinates
        for (uint32_t k = tid; k < nf; k += kInterThreads) world_point(Rs, scale, Xt + 3 * (size_t)k, jb.Xw + 3 * (size_t)k);
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        *jb.valid = stage == CLC_INTER_OK ? 0 : -1;      // the refinement's go / no-go word
        jb.rec->stage = stage; jb.rec->n_common = (int32_t)n_common; jb.rec->n_map_matches = (int32_t)n_raw; jb.rec->scale = scale;
        __hip_atomic_store(&jb.rec->ready, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// a context's blocks of this step, for `cap` correspondences against `map_n` map rows (InterDev / InterPin, clc_layout.h)
struct InterView : InterDev, InterPin {};
int ensure_inter(clc_ctx* ctx, const size_t cap, const size_t map_n, InterView& v)
{
    int rc = carve_block(ctx, ctx->d_inter, 1, 4, true, "growing the inter-camera block", [&](Carve& c) { v.InterDev::carve(c, cap, map_n, sizeof(RefineOut)); });
    if (rc == CLC_OK)
        rc = carve_block(ctx, ctx->h_inter, 0, 1, true, "growing the pinned inter-camera records",
                         [&](Carve& c) { v.InterPin::carve(c, sizeof(InterScaleRec), sizeof(RefineOut)); });
    return rc;
}

InterCam cam_of(const clc_camera_k3& c) { return InterCam{ c.focal, c.ppx, c.ppy }; }

void motions_of(const double* E9, double cand[4][12])
{
    openMVG::Mat3 E;
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) E(i, j) = E9[3 * i + j];
    std::vector<openMVG::geometry::Pose3> poses;
    coloc::hipgeom::motion_from_essential(E, &poses);
    for (int c = 0; c < 4; ++c) {
        const openMVG::Mat3& R = poses[(size_t)c].rotation();
        const openMVG::Vec3 t = poses[(size_t)c].translation();
        for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) cand[c][4 * r + q] = R(r, q); cand[c][4 * r + 3] = t[r]; }
    }
}

int inter_batch(clc_ctx* const* ctxs, clc_inter_dev_job* jobs, const int n_jobs)
{
    clc_ctx* c0 = ctxs[0];
    for (int i = 0; i < n_jobs; ++i) {
        clc_inter_dev_job& jb = jobs[i];
        memset(jb.Rt, 0, sizeof jb.Rt); memset(jb.cov, 0, sizeof jb.cov);
        jb.rmse = 0.0; jb.scale = 0.0; jb.n_front = 0; jb.n_common = 0; jb.n_refined = 0; jb.n_map_matches = 0; jb.stage = CLC_INTER_NO_MODEL;
        const int chain = (jb.d_first_desc != nullptr) + (jb.d_map_desc != nullptr);
        if (!jb.Rt_source || chain == 1 || (chain == 2) == (jb.d_map_match_a != nullptr) ||
            (((uintptr_t)jb.d_first_desc | (uintptr_t)jb.d_map_desc) & 15u) || ((uintptr_t)jb.d_map_match_a & 3u))
            return fail(ctxs[i], CLC_ERR_BAD_ARG, "inter_pose_dev: a job needs Rt_source and EITHER d_first_desc + d_map_desc (16-byte aligned) OR d_map_match_a");
    }
    if (c0->map_X_n < 0) return fail(c0, CLC_ERR_STATE, "inter_pose_dev before set_map_points");
    const int map_n = c0->map_X_n;
    // 1. the pair gather and the five-point filters, exactly as clc_pair_filter_batch_dev runs them (pose_batch.hip)
    std::vector<clc_pair_job> pj((size_t)n_jobs);
    std::vector<double> Es((size_t)9 * n_jobs, 0.0);
    std::vector<const int32_t*> d_inl((size_t)n_jobs, nullptr);
    for (int i = 0; i < n_jobs; ++i) { pj[(size_t)i] = jobs[i].pair; if (!pj[(size_t)i].M) pj[(size_t)i].M = &Es[(size_t)9 * i]; }
    int worst = pair_filter_essential(ctxs, pj.data(), n_jobs, d_inl.data());
    for (int i = 0; i < n_jobs; ++i) {
        clc_pair_job& o = jobs[i].pair; const clc_pair_job& r = pj[(size_t)i];
        o.n_pairs = r.n_pairs; o.n_inliers = r.n_inliers; o.iterations = r.iterations; o.status = r.status; o.error_max = r.error_max; o.min_nfa = r.min_nfa;
    }
    CLC_HIP(c0, hipSetDevice(c0->device));
    hipStream_t st = c0->stream;
    // 2. + 3. the four motions of every job's E, the front launch(es) of the batch
    std::vector<InterView> view((size_t)n_jobs);
    std::vector<int> live;
    std::vector<double> cand((size_t)48 * n_jobs, 0.0);              // job i's four motions [R|t]
    FrontJobs fj{};
    // A failure once launches are in flight: they still write the jobs' blocks and pinned records, so every stream is drained first
    // (ignoring what the drains report), and every job that has no result yet carries the failure instead of CLC_OK.
    std::vector<char> done((size_t)n_jobs, 0);
    const auto abort_all = [&](const int rc) {
        for (int i = 0; i < n_jobs; ++i) (void)hipStreamSynchronize(ctxs[i]->stream);
        for (const int i : live) if (!done[(size_t)i]) { jobs[i].pair.status = rc; jobs[i].stage = CLC_INTER_NO_REFINEMENT; }
        return rc;
    };
    for (int i = 0; i < n_jobs; ++i) {
        clc_inter_dev_job& jb = jobs[i];
        const clc_pair_job& p = pj[(size_t)i];
        if (p.status != CLC_OK || p.n_inliers < 13 || !d_inl[(size_t)i]) continue;                // CLC_INTER_NO_MODEL
        const int N = std::min(p.n_pairs, std::min(p.nq, kAcrMaxN));
        const int rc = ensure_inter(ctxs[i], (size_t)N, jb.d_first_desc ? (size_t)map_n : 0, view[(size_t)i]);
        if (rc != CLC_OK) { jb.pair.status = rc; if (worst == CLC_OK) worst = rc; continue; }
        const InterView& v = view[(size_t)i];
        const GatherView g(ctxs[i]->pair, kPairLayout);
        FrontJobDev& f = fj.j[live.size()];
        double (*mo)[12] = (double (*)[12])&cand[(size_t)48 * i];
        motions_of(p.M, mo);
        // (motion_from_essential: candidate c = two rotations x two signs of t, its own translation each)
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 3; ++r) { f.t[c][r] = mo[c][4 * r + 3]; for (int q = 0; q < 3; ++q) { if (c < 2) f.R[c][3 * r + q] = mo[c][4 * r + q]; else mo[c][4 * r + q] = f.R[c & 1][3 * r + q]; } }
        f.k1 = cam_of(p.cam_a); f.k2 = cam_of(p.cam_b);
        f.x1 = g.a; f.x2 = g.b; f.inliers = d_inl[(size_t)i]; f.rows = jb.lower_is_b ? g.t : g.q;
        f.Xt = v.Xt; f.x2f = v.x2f; f.corr = v.corr; f.first = jb.d_first_desc ? v.first : nullptr;
        f.rec = v.h_front; f.n = N; f.n_inliers = p.n_inliers; f.list = v.kk;
        memset(v.h_front, 0, 16);
        __atomic_store_n(&v.h_scale->ready, 0, __ATOMIC_RELAXED);
        __atomic_store_n(&v.h_ref->ready, 0, __ATOMIC_RELAXED);
        // (the inlier list lies in the context's pinned block, where the round that completed the filter left it before its word: the
        // vote reads it there once and leaves it in v.kk, free until the scale kernel; the pair block was written on st)
        live.push_back(i);
    }
    if (live.empty()) return worst;
    hipLaunchKernelGGL(inter_front_kernel, dim3(1, (unsigned)live.size()), dim3(kInterThreads), 0, st, fj);
    CLC_HIP(c0, hipGetLastError());
    // the reference's chain sweeps on the job's own stream: those streams behind the front launch
    std::vector<hipStream_t> own;
    for (const int i : live) if (jobs[i].d_first_desc && ctxs[i]->stream != st) own.push_back(ctxs[i]->stream);
    hipError_t e = own.empty() ? hipSuccess : order_behind(c0->ev_track, st, own.data(), own.size());
    if (e != hipSuccess) return abort_all(fail(c0, CLC_ERR_HIP, "inter_pose_dev: ordering the sweeps behind the front launch", e));
    // 4. the one wait this path adds: the jobs' pinned n_front words
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int> go;
    ScaleJobs sj{};
    sj.map_X = c0->d_map_X.as<double>(); sj.map_n = map_n;
    for (size_t l = 0; l < live.size(); ++l) {
        const int i = live[l];
        clc_inter_dev_job& jb = jobs[i];
        const InterView& v = view[(size_t)i];
        const int rc = wait_pinned(c0, &v.h_front[3], 0, st, t0, 5, "inter_pose_dev: the front launch left no record");
        if (rc != CLC_OK) { if (ctxs[i] != c0) (void)fail(ctxs[i], rc, clc_last_error_string(c0)); return abort_all(rc); }
        jb.stage = v.h_front[2];
        if (jb.stage != CLC_INTER_OK) { done[(size_t)i] = 1; continue; }
        const int nf = v.h_front[0], chosen = v.h_front[1];
        if (chosen < 0 || chosen > 3 || nf < 8 || nf > fj.j[l].n_inliers) return abort_all(fail(ctxs[i], CLC_ERR_HIP, "inter_pose_dev: a front record out of range"));
        jb.n_front = nf;
        // 5. the reference's chain: the temporary map's descriptor rows by the index list the front kernel left, then the K2NN sweep
        //    (Q = global map, T = temporary map), on the job's own stream behind the front launch
        if (jb.d_first_desc) {
            hipStream_t sweep = ctxs[i]->stream;
            const int rk = map_sweep_enqueue(ctxs[i], jb.d_first_desc, v.first, nf, jb.d_map_desc, map_n, (uint4*)v.rows, v.match, jb.match_threshold, sweep);
            if (rk != CLC_OK) return abort_all(rk);
            e = sweep != st ? order_behind(ctxs[i]->ev_track, sweep, &st, 1) : hipSuccess;
            if (e != hipSuccess) return abort_all(fail(ctxs[i], CLC_ERR_HIP, "inter_pose_dev: ordering the scale launch behind the sweep", e));
        }
        ScaleJobDev& s = sj.j[go.size()];
        memcpy(s.Rs, jb.Rt_source, sizeof s.Rs);
        const double* Rt = &cand[(size_t)48 * i + 12 * (size_t)chosen];
        for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) s.Rb[3 * r + q] = Rt[4 * r + q]; s.tb[r] = Rt[4 * r + 3]; }
        s.k2 = cam_of(pj[(size_t)i].cam_b);
        s.Xt = v.Xt; s.corr = v.corr; s.nf = nf;
        s.match = jb.d_first_desc ? v.match : nullptr;
        s.map_match_a = jb.d_map_match_a; s.pair_q = GatherView(ctxs[i]->pair, kPairLayout).q;
        s.cg = v.cg; s.ck = v.ck; s.kg = v.kg; s.kk = v.kk; s.ratio = v.ratio; s.term = v.term;
        s.Rt = v.Rt; s.Xw = v.Xw; s.K = v.K; s.valid = v.valid; s.rec = v.h_scale;
        go.push_back(i);
    }
    if (go.empty()) return worst;
    // 6. ONE scale launch, 7. the refinements behind it on the jobs' own streams, gated by the device go / no-go word
    hipLaunchKernelGGL(inter_scale_kernel, dim3(1, (unsigned)go.size()), dim3(kInterThreads), 0, st, sj);
    if ((e = hipGetLastError()) != hipSuccess) return abort_all(fail(c0, CLC_ERR_HIP, "inter_pose_dev: the scale launch", e));
    own.clear();
    for (const int i : go) if (ctxs[i]->stream != st) own.push_back(ctxs[i]->stream);
    e = own.empty() ? hipSuccess : order_behind(c0->ev_group, st, own.data(), own.size());
    if (e != hipSuccess) return abort_all(fail(c0, CLC_ERR_HIP, "inter_pose_dev: ordering the refinements behind the scale launch", e));
    for (const int i : go) {
        clc_inter_dev_job& jb = jobs[i];
        const InterView& v = view[(size_t)i];
        e = launch_pnp_refine(v.Rt, v.Xw, v.x2f, nullptr, jb.n_front, v.K, jb.huber_a > 0.0 ? jb.huber_a : 16.0, 50, v.ref, ctxs[i]->stream,
                              &ctxs[i]->prof, v.valid, v.h_ref);
        if (e != hipSuccess) return abort_all(fail(ctxs[i], CLC_ERR_HIP, "inter_pose_dev: enqueueing the refinement", e));
    }
    // collect through the pinned records (the refinement's comes out behind the scale kernel's)
    const auto t1 = std::chrono::steady_clock::now();
    for (const int i : go) {
        clc_inter_dev_job& jb = jobs[i];
        const InterView& v = view[(size_t)i];
        int rc = wait_pinned(ctxs[i], &v.h_ref->ready, 0, ctxs[i]->stream, t1, 5, "inter_pose_dev: refinement did not complete");
        if (rc == CLC_OK) rc = wait_pinned(ctxs[i], &v.h_scale->ready, 0, st, t1, 5, "inter_pose_dev: the scale launch left no record");
        if (rc != CLC_OK) return abort_all(rc);
        done[(size_t)i] = 1;
        jb.stage = v.h_scale->stage; jb.n_common = v.h_scale->n_common; jb.n_map_matches = v.h_scale->n_map_matches;
        if (jb.stage != CLC_INTER_OK) continue;
        jb.scale = v.h_scale->scale;
        take_refined(jb, *v.h_ref);
    }
    return worst;
}

} // namespace

} // namespace clc

using namespace clc;

extern "C" {

int clc_inter_pose_batch_dev(clc_ctx* const* ctxs, clc_inter_dev_job* jobs, int n_jobs)
{
    if (n_jobs < 0 || (n_jobs > 0 && (!ctxs || !jobs))) return CLC_ERR_BAD_ARG;
    if (n_jobs == 0) return CLC_OK;
    if (n_jobs > kMaxBatch) return ctxs[0] ? fail(ctxs[0], CLC_ERR_CAPACITY, "inter_pose_batch_dev: more than CLC_MAX_BATCH jobs") : CLC_ERR_BAD_ARG;
    const int rc0 = check_batch_contexts(ctxs, n_jobs, "inter_pose_batch_dev: every job needs a context of its own");
    if (rc0 != CLC_OK) return rc0;
    return inter_batch(ctxs, jobs, n_jobs);
}

int clc_inter_pose_dev(clc_ctx* ctx, clc_inter_dev_job* job)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "inter_pose_dev: null context / job");
    return inter_batch(&ctx, job, 1);
}

int clc_inter_front_dev(clc_ctx* ctx, const double* d_x1, const double* d_x2, int n, const int32_t* d_inliers, int n_inliers,
                        const clc_camera_k3* cam_a, const clc_camera_k3* cam_b, const double* h_motions, const int32_t* d_rows,
                        double* d_Xt, double* d_x2f, int32_t* d_corr, int32_t* d_first, int32_t* d_record, void* stream)
{
    if (!ctx || !cam_a || !cam_b || !h_motions || !d_record || n < 0 || n_inliers < 0 || (d_first != nullptr) != (d_rows != nullptr))
        return fail(ctx, CLC_ERR_BAD_ARG, "inter_front: bad argument");
    if (n_inliers > 0 && (!d_x1 || !d_x2 || !d_Xt || !d_x2f || !d_corr)) return fail(ctx, CLC_ERR_BAD_ARG, "inter_front: null block");
    if (n_inliers > kAcrMaxN) return fail(ctx, CLC_ERR_CAPACITY, "inter_front: more than 16384 inliers");
    if (!(cam_a->focal > 0.0) || !(cam_b->focal > 0.0)) return fail(ctx, CLC_ERR_BAD_ARG, "inter_front: focal must be positive");
    if ((((uintptr_t)d_x1 | (uintptr_t)d_x2 | (uintptr_t)d_Xt | (uintptr_t)d_x2f) & 7u) ||
        (((uintptr_t)d_inliers | (uintptr_t)d_rows | (uintptr_t)d_corr | (uintptr_t)d_first | (uintptr_t)d_record) & 3u))
        return fail(ctx, CLC_ERR_BAD_ARG, "inter_front: misaligned device pointer");
    FrontJobs fj{};
    FrontJobDev& f = fj.j[0];
    memcpy(fj.cand0, h_motions, sizeof fj.cand0);
    fj.full = 1;
    f.k1 = cam_of(*cam_a); f.k2 = cam_of(*cam_b);
    f.x1 = d_x1; f.x2 = d_x2; f.inliers = d_inliers; f.rows = d_rows;
    f.Xt = d_Xt; f.x2f = d_x2f; f.corr = d_corr; f.first = d_first; f.rec = d_record; f.list = nullptr;
    f.n = n; f.n_inliers = n_inliers;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(inter_front_kernel, dim3(1, 1), dim3(kInterThreads), 0, pick(ctx, stream), fj);
    CLC_HIP(ctx, hipGetLastError());
    return CLC_OK;
}

} // extern "C"

// pnp.hip -- batched-hypothesis reprojection scoring for PnP / RANSAC on gfx950 (MI355X).
//
// What it replaces: inside openMVG::sfm::SfM_Localizer::Localize (called at reference
// include/coloc/Localizer.hpp:93 with P3P_KE_CVPR17, max_iteration = 256, :82-84) every RANSAC
// iteration evaluates the pixel reprojection error of each candidate [R|t] over all N 2D-3D
// correspondences on one CPU thread.  Here ALL H hypotheses (<= 256 iterations x <= 4 P3P roots)
// are scored in one launch: grid = (point tiles) x (hypotheses), the 12 pose doubles and the 9
// intrinsics are wave-uniform scalar loads, points are read coalesced (and stay L2-resident
// across hypotheses: N x 40 B).
//
//   err[h][i] = || x_i - hnormalized( K (R_h X_i + t_h) ) ||^2      (fp64, pixels^2)
//
// fp64 throughout, operation order identical to the oracle (oracle/clc_oracle.c
// orc_pnp_residuals) and no FMA contraction, so the residual matrix is reproduced exactly; the
// fused score kernel reduces in a different order than a sequential sum, hence the 1e-12
// relative tolerance on `cost` in the tests.
#include "clc_internal.h"
#include "p3p.h"
#include "pose_lm.h"
#include "fivept_wave.h"

namespace clc {

__device__ __forceinline__ double reproj_err(const double* __restrict__ P, const double* __restrict__ K,
                                             const double Xw, const double Yw, const double Zw,
                                             const double u_obs, const double v_obs)
{
    const double xc = ((P[0] * Xw + P[1] * Yw) + P[2] * Zw) + P[3];
    const double yc = ((P[4] * Xw + P[5] * Yw) + P[6] * Zw) + P[7];
    const double zc = ((P[8] * Xw + P[9] * Yw) + P[10] * Zw) + P[11];
    const double u = (K[0] * xc + K[1] * yc) + K[2] * zc;
    const double v = (K[3] * xc + K[4] * yc) + K[5] * zc;
    const double w = (K[6] * xc + K[7] * yc) + K[8] * zc;
    const double du = u_obs - u / w;
    const double dv = v_obs - v / w;
    return du * du + dv * dv;
}

__global__ __launch_bounds__(256) void pnp_residual_kernel(const double* __restrict__ Rt, const double* __restrict__ X,
                                                           const double* __restrict__ x, const int N,
                                                           const double* __restrict__ K, double* __restrict__ err)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int h = blockIdx.y;
    if (i >= N) return;
    const double* P = Rt + (size_t)12 * h;
    err[(size_t)h * N + i] = reproj_err(P, K, X[3 * i], X[3 * i + 1], X[3 * i + 2], x[2 * i], x[2 * i + 1]);
}

// one workgroup per hypothesis: inlier count (exact) + truncated cost (tree-reduced)
__global__ __launch_bounds__(256) void pnp_score_kernel(const double* __restrict__ Rt, const double* __restrict__ X,
                                                        const double* __restrict__ x, const int N,
                                                        const double* __restrict__ K, const double thr2,
                                                        int32_t* __restrict__ count, double* __restrict__ cost)
{
    __shared__ double s_cost[256];
    __shared__ int s_cnt[256];
    const int h = blockIdx.x;
    const double* P = Rt + (size_t)12 * h;
    int cnt = 0;
    double c = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        const double e = reproj_err(P, K, X[3 * i], X[3 * i + 1], X[3 * i + 2], x[2 * i], x[2 * i + 1]);
        if (e < thr2) { ++cnt; c += e; }
        else c += thr2;
    }
    s_cost[threadIdx.x] = c;
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            s_cost[threadIdx.x] += s_cost[threadIdx.x + st];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (count) count[h] = s_cnt[0];
        if (cost) cost[h] = s_cost[0];
    }
}

// ---- batched minimal solver: one P3P problem per FOUR lanes ------------------------------------------
// samples: S x 3 point indices.  The four lanes of a sample all build the quartic and solve it in closed form (the
// same instructions on the same numbers), then lane r polishes root r and turns it into pose slot r of the sample
// (H = 4 S slots).  Slots without a valid pose are NaN so that they score worst (every comparison with NaN is false:
// 0 inliers, cost = N * thr2).  One lane per sample doing the four roots in turn took 13-15 us; the per-root half of
// the chain now runs four wide.
__global__ __launch_bounds__(64) void p3p_kernel(const double* __restrict__ X, const double* __restrict__ x,
                                                 const double* __restrict__ K, const int32_t* __restrict__ samples,
                                                 const int S, const int N, double* __restrict__ Rt,
                                                 const int solve_blocks, const double* __restrict__ stage_src,
                                                 double* __restrict__ stage_dst, const int stage_n,
                                                 const int32_t* __restrict__ n_dev = nullptr)
{
    if ((int)blockIdx.x >= solve_blocks) {
        // staging duty (clc_pnp_ransac / clc_pnp_localize): X, x, K and samples above are the caller's PINNED HOST
        // buffer, read here straight over PCIe; these extra workgroups copy it into device memory for the scoring
        // launches that follow (which read every point a thousand times) -- no separate host-to-device copy command
        const int nb = (int)gridDim.x - solve_blocks;
        for (int i = ((int)blockIdx.x - solve_blocks) * 64 + (int)threadIdx.x; i < stage_n; i += nb * 64) stage_dst[i] = stage_src[i];
        return;
    }
    const int gid = blockIdx.x * 64 + threadIdx.x;
    const int sidx = gid >> 2, root = gid & 3;
    if (sidx >= S || (n_dev && sidx >= *n_dev)) return;
    // slots without a valid pose are NaN (p3p.h p3p_sample_root: the solve of one root, force-inlined here and into acr_round_kernel; the two
    // copies are held to the same bits by tests/test_gpu_acransac.py::test_pose_many_seeds_same_bits_as_p3p_kernel, the gate to re-run
    // on every compiler bump)
    p3p_sample_root(X, x, K, samples[3 * sidx], samples[3 * sidx + 1], samples[3 * sidx + 2], N, root, Rt + (size_t)48 * sidx + 12 * root);
}

// best hypothesis: most inliers, then lowest cost, then lowest index -- and its inlier mask, in ONE
// launch: every workgroup recomputes the (cheap, deterministic) argmax over the <= 64k hypotheses, so no
// inter-workgroup hand-off is needed; workgroup 0 also publishes {h, count, cost, pose}.
__device__ __forceinline__ bool hyp_better(const int32_t* __restrict__ count, const double* __restrict__ cost, int b, int a)
{
    return count[b] > count[a] || (count[b] == count[a] && (cost[b] < cost[a] || (cost[b] == cost[a] && b < a)));
}

__global__ __launch_bounds__(256) void pnp_select_mask_kernel(const double* __restrict__ Rt, const int32_t* __restrict__ count,
                                                              const double* __restrict__ cost, const int H,
                                                              const double* __restrict__ X, const double* __restrict__ x, const int N,
                                                              const double* __restrict__ K, const double thr2,
                                                              uint8_t* __restrict__ mask, PnpResult* __restrict__ res,
                                                              uint8_t* __restrict__ h_mask, PnpResult* __restrict__ h_res)
{
    // h_mask / h_res (nullable): the caller's pinned host buffer -- the record and the mask are written there as well,
    // so that the host needs no device-to-host copy command after the launch
    __shared__ int s_h[256];
    int bh = -1;
    for (int h = threadIdx.x; h < H; h += 256)
        if (bh < 0 || hyp_better(count, cost, h, bh)) bh = h;
    s_h[threadIdx.x] = bh;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const int a = s_h[threadIdx.x], b = s_h[threadIdx.x + st];
            s_h[threadIdx.x] = a < 0 ? b : ((b >= 0 && hyp_better(count, cost, b, a)) ? b : a);
        }
        __syncthreads();
    }
    const int h = s_h[0];
    const bool ok = h >= 0 && count[h] > 0;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0) {
        if (threadIdx.x < 12) {
            const double v = ok ? Rt[(size_t)12 * h + threadIdx.x] : 0.0;
            res->Rt[threadIdx.x] = v;
            if (h_res) h_res->Rt[threadIdx.x] = v;
        }
        if (threadIdx.x == 12) {
            const int32_t hh = ok ? h : -1, cc = ok ? count[h] : 0;
            const double qq = ok ? cost[h] : 0.0;
            res->h = hh; res->count = cc; res->cost = qq;
            if (h_res) { h_res->h = hh; h_res->count = cc; h_res->cost = qq; }
        }
    }
    if (i >= N) return;
    uint8_t m = 0;
    if (ok) {
        const double e = reproj_err(Rt + (size_t)12 * h, K, X[3 * i], X[3 * i + 1], X[3 * i + 2], x[2 * i], x[2 * i + 1]);
        m = e < thr2 ? 1 : 0;
    }
    mask[i] = m;
    if (h_mask) h_mask[i] = m;
}

// ---- single-pose refinement + 6x6 covariance ------------------------
// The Levenberg-Marquardt pass, its bookkeeping and the record are pose_lm.h's (shared with pose_prior.hip).  This kernel's own: the
// optional byte mask, the record of a chained solve that found no pose (valid < 0), the number of points used as the 29th sum, and
// where the record goes (out_host: the caller's pinned buffer, no device-to-host copy command; else out_dev).
__global__ __launch_bounds__(kPoseThreads) void pnp_refine_kernel(const double* __restrict__ Rt_in, const double* __restrict__ X,
                                                                  const double* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                  const int N, const double* __restrict__ K, const double huber_a,
                                                                  const int max_iter, const int32_t* __restrict__ valid,
                                                                  RefineOut* __restrict__ out_dev, RefineOut* __restrict__ out_host)
{
#pragma clang fp contract(fast)
    RefineOut* const out = out_host ? out_host : out_dev;
    const int tid = threadIdx.x;
    if (valid && *valid < 0) {          // chained after clc_pnp_ransac that found no pose: nothing to refine
        if (tid < 12) out->Rt[tid] = 0.0;
        if (tid < 36) out->cov[tid] = 0.0;
        if (tid == 0) { out->cost = 0.0; out->rmse = 0.0; out->iterations = 0; out->n_used = 0; }
        pose_publish(tid, &out->ready);
        return;
    }
    extern __shared__ double red[];     // pose_reduce's scratch (kPoseRedBytes)
    __shared__ PoseLds s;
    const PoseCam cam = { K[0], K[1], K[2], K[4], K[5], huber_a, huber_a * huber_a };
    pose_start(s, tid, Rt_in);

    auto pass = [&](const double* par) {
        pose_rotation(s, tid, par);
        double acc[kPoseSums];
#pragma unroll
        for (int i = 0; i < kPoseSums; ++i) acc[i] = 0.0;
        for (int i = tid; i < N; i += kPoseThreads) {
            if (mask && !mask[i]) continue;
            const PosePoint p = pose_residual(s, par, cam, X, x, i);
            acc[28] += 1.0;
            pose_accumulate(s, cam, p, acc);
        }
        pose_reduce(s, red, tid, acc);
    };

    // ONE call site of pass(): the first trip evaluates the start s.par, every later one the trial s.try_; the bookkeeping around it
    // is the loop  "step -> [flag] -> evaluate -> accept / reject"  unrolled by half a turn.
    LmState lm;
    bool initial = true;
    for (;;) {
        pass(initial ? s.par : s.try_);
        if (initial) {
            pose_keep_sums(s, tid);
            lm.cost = s.A[27];
            initial = false;
        } else {
            bool accepted;
            if (lm_judge(s, tid, lm, accepted)) break;
        }
        if (lm_next_step(s, tid, lm, max_iter)) break;
    }
    // s.A holds the sums at s.par
    pose_cov_column(s, tid, true, out->cov);
    if (tid == 0) {
        pose_Rt(s, out->Rt);
        const double n_used = s.A[28];
        out->cost = s.A[27];
        out->rmse = pose_rmse(s.A[27], n_used);
        out->iterations = lm.it;
        out->n_used = (int32_t)n_used;
    }
    pose_publish(tid, &out->ready);
}

hipError_t launch_pnp_refine(const double* d_Rt_in, const double* d_X, const double* d_x, const uint8_t* d_mask, int N,
                             const double* d_K, double huber_a, int max_iter, void* d_out, hipStream_t stream, Profiler* prof,
                             const int32_t* d_valid, void* h_out)
{
    if (N <= 0) return hipSuccess;
    const hipError_t e = pose_allow_lds<pnp_refine_kernel>();
    if (e != hipSuccess) return e;
    prof_mark(prof, CLC_KERNEL_PNP_SCORE, true, stream);
    hipLaunchKernelGGL(pnp_refine_kernel, dim3(1), dim3(kPoseThreads), kPoseRedBytes, stream, d_Rt_in, d_X, d_x, d_mask, N, d_K, huber_a, max_iter,
                       d_valid, (RefineOut*)d_out, (RefineOut*)h_out);
    prof_mark(prof, CLC_KERNEL_PNP_SCORE, false, stream);
    return hipGetLastError();
}

hipError_t launch_pnp_ransac(const double* d_X, const double* d_x, int N, const double* d_K, const int32_t* d_samples,
                             int S, double thr2, double* d_Rt /* 48*S */, int32_t* d_count, double* d_cost,
                             uint8_t* d_mask, void* d_result, hipStream_t stream, Profiler* prof, const PnpHostStage* hs)
{
    if (S <= 0 || N <= 0) return hipSuccess;
    prof_mark(prof, CLC_KERNEL_PNP_SCORE, true, stream);
    const int solve_blocks = (4 * S + 63) / 64;
    if (hs) {
        // inputs still sit in the pinned host buffer: the solver lanes read their three points from there, extra
        // workgroups stage everything into d_X.. for the launches below
        int stage_blocks = (hs->n_doubles + 255) / 256;
        if (stage_blocks > 64) stage_blocks = 64;
        const double* hX = hs->src;
        const double* hx = hX + (size_t)3 * N;
        const double* hK = hx + (size_t)2 * N;
        const int32_t* hSamples = (const int32_t*)(hK + 16);
        hipLaunchKernelGGL(p3p_kernel, dim3(solve_blocks + stage_blocks), dim3(64), 0, stream, hX, hx, hK, hSamples, S, N, d_Rt,
                           solve_blocks, hs->src, const_cast<double*>(d_X), hs->n_doubles, (const int32_t*)nullptr);
    } else {
        hipLaunchKernelGGL(p3p_kernel, dim3(solve_blocks), dim3(64), 0, stream, d_X, d_x, d_K, d_samples, S, N, d_Rt, solve_blocks,
                           (const double*)nullptr, (double*)nullptr, 0, (const int32_t*)nullptr);
    }
    hipLaunchKernelGGL(pnp_score_kernel, dim3(4 * S), dim3(256), 0, stream, (const double*)d_Rt, d_X, d_x, N, d_K, thr2, d_count, d_cost);
    hipLaunchKernelGGL(pnp_select_mask_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, (const double*)d_Rt,
                       (const int32_t*)d_count, (const double*)d_cost, 4 * S, d_X, d_x, N, d_K, thr2, d_mask, (PnpResult*)d_result,
                       hs ? hs->h_mask : nullptr, hs ? (PnpResult*)hs->h_result : nullptr);
    prof_mark(prof, CLC_KERNEL_PNP_SCORE, false, stream);
    return hipGetLastError();
}

// ---- two-view scoring: symmetric epipolar distance of H fundamental matrices ----------
// The error model RobustMatcher::filterEssential gives AC-RANSAC (reference include/coloc/RobustMatcher.hpp:161-168,
// openMVG SymmetricEpipolarDistanceError on pixel coordinates with F = K2^-T E K1^-1).  Same batched shape as
// the PnP scoring: all hypotheses x all correspondences in one launch; operation order = oracle's (exact).
__device__ __forceinline__ double epipolar_err(const double* __restrict__ f, double u1, double v1, double u2, double v2)
{
    const double a0 = (f[0] * u1 + f[1] * v1) + f[2];
    const double a1 = (f[3] * u1 + f[4] * v1) + f[5];
    const double a2 = (f[6] * u1 + f[7] * v1) + f[8];
    const double b0 = (f[0] * u2 + f[3] * v2) + f[6];
    const double b1 = (f[1] * u2 + f[4] * v2) + f[7];
    const double d = (u2 * a0 + v2 * a1) + a2;
    return (d * d) * (1.0 / (a0 * a0 + a1 * a1) + 1.0 / (b0 * b0 + b1 * b1)) / 4.0;
}

__global__ __launch_bounds__(256) void epipolar_residual_kernel(const double* __restrict__ F, const double* __restrict__ x1,
                                                                const double* __restrict__ x2, const int N, double* __restrict__ err)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    err[(size_t)blockIdx.y * N + i] = epipolar_err(F + (size_t)9 * blockIdx.y, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1]);
}

__global__ __launch_bounds__(256) void epipolar_score_kernel(const double* __restrict__ F, const double* __restrict__ x1,
                                                             const double* __restrict__ x2, const int N, const double thr2,
                                                             int32_t* __restrict__ count, double* __restrict__ cost)
{
    __shared__ double s_cost[256];
    __shared__ int s_cnt[256];
    const double* f = F + (size_t)9 * blockIdx.x;
    int cnt = 0;
    double c = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        const double e = epipolar_err(f, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1]);
        if (e < thr2) { ++cnt; c += e; }
        else c += thr2;
    }
    s_cost[threadIdx.x] = c;
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) { s_cost[threadIdx.x] += s_cost[threadIdx.x + st]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + st]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { if (count) count[blockIdx.x] = s_cnt[0]; if (cost) cost[blockIdx.x] = s_cost[0]; }
}

// ---- essential-matrix RANSAC: five-point problems, one per lane ---------------------------
// samples: S x 5 correspondence indices.  Each lane normalises its 5 point pairs with K1^-1 / K2^-1, solves the
// five-point problem (csrc/fivept.h, <= 10 real solutions) and writes 10 slots of {F = K2^-T E K1^-1 (9), E (9)};
// unused slots are NaN so that they score worst.  The arrays of the solver live in scratch memory: this kernel is
// latency-bound by design (256 lanes), the scoring that follows is the data-parallel part.
__global__ __launch_bounds__(64) void fivept_kernel(const double* __restrict__ x1, const double* __restrict__ x2,
                                                    const double* __restrict__ K1, const double* __restrict__ K2,
                                                    const int32_t* __restrict__ samples, const int S, const int N,
                                                    double* __restrict__ FE /* S x 10 x 18 */, const int32_t* __restrict__ n_dev = nullptr)
{
    // ONE sample per wave: the solver is full of data-dependent steps (pivoting, iterations that stop on convergence), and 64
    // different problems in one wave serialise every divergent branch -- measured 4.8 ms for 256 samples with a problem per
    // lane.  The wave's lanes share the work of their problem instead (csrc/fivept_wave.h); lane 0 writes the result.  The body is
    // fpw::models_of_sample: one not-inlined function shared with the a-contrario round's own solve (acransac.hip).
    const int sidx = blockIdx.x;
    if (sidx >= S || (n_dev && sidx >= *n_dev)) return;
    const int32_t* sp = samples + 5 * sidx;
    fpw::models_of_sample(x1, x2, K1, K2, sp[0], sp[1], sp[2], sp[3], sp[4], N, FE + (size_t)180 * sidx);
}

// score the F part of every slot (stride 18 doubles)
__global__ __launch_bounds__(256) void epipolar_score_strided_kernel(const double* __restrict__ FE, const double* __restrict__ x1,
                                                                     const double* __restrict__ x2, const int N, const double thr2,
                                                                     int32_t* __restrict__ count, double* __restrict__ cost)
{
    __shared__ double s_cost[256];
    __shared__ int s_cnt[256];
    const double* f = FE + (size_t)18 * blockIdx.x;
    int cnt = 0;
    double c = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) {
        const double e = epipolar_err(f, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1]);
        if (e < thr2) { ++cnt; c += e; }
        else c += thr2;
    }
    s_cost[threadIdx.x] = c;
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) { s_cost[threadIdx.x] += s_cost[threadIdx.x + st]; s_cnt[threadIdx.x] += s_cnt[threadIdx.x + st]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { count[blockIdx.x] = s_cnt[0]; cost[blockIdx.x] = s_cost[0]; }
}

__global__ __launch_bounds__(256) void epipolar_select_mask_kernel(const double* __restrict__ FE, const int32_t* __restrict__ count,
                                                                   const double* __restrict__ cost, const int H,
                                                                   const double* __restrict__ x1, const double* __restrict__ x2,
                                                                   const int N, const double thr2, uint8_t* __restrict__ mask,
                                                                   EpiResult* __restrict__ res)
{
    __shared__ int s_h[256];
    int bh = -1;
    for (int h = threadIdx.x; h < H; h += 256)
        if (bh < 0 || hyp_better(count, cost, h, bh)) bh = h;
    s_h[threadIdx.x] = bh;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const int a = s_h[threadIdx.x], b = s_h[threadIdx.x + st];
            s_h[threadIdx.x] = a < 0 ? b : ((b >= 0 && hyp_better(count, cost, b, a)) ? b : a);
        }
        __syncthreads();
    }
    const int h = s_h[0];
    const bool ok = h >= 0 && count[h] > 0;
    const double* f = FE + (size_t)18 * (ok ? h : 0);
    if (blockIdx.x == 0) {
        if (threadIdx.x < 9) { res->F[threadIdx.x] = ok ? f[threadIdx.x] : 0.0; res->E[threadIdx.x] = ok ? f[9 + threadIdx.x] : 0.0; }
        if (threadIdx.x == 9) { res->h = ok ? h : -1; res->count = ok ? count[h] : 0; res->cost = ok ? cost[h] : 0.0; }
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    mask[i] = (ok && epipolar_err(f, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1]) < thr2) ? 1 : 0;
}

hipError_t launch_essential_ransac(const double* d_x1, const double* d_x2, int N, const double* d_K1, const double* d_K2,
                                   const int32_t* d_samples, int S, double thr2, double* d_FE, int32_t* d_count, double* d_cost,
                                   uint8_t* d_mask, void* d_result, hipStream_t stream, Profiler* prof)
{
    if (S <= 0 || N <= 0) return hipSuccess;
    prof_mark(prof, CLC_KERNEL_PNP_SCORE, true, stream);
    hipLaunchKernelGGL(fivept_kernel, dim3(S), dim3(64), 0, stream, d_x1, d_x2, d_K1, d_K2, d_samples, S, N, d_FE, (const int32_t*)nullptr);
    hipLaunchKernelGGL(epipolar_score_strided_kernel, dim3(10 * S), dim3(256), 0, stream, (const double*)d_FE, d_x1, d_x2, N, thr2,
                       d_count, d_cost);
    hipLaunchKernelGGL(epipolar_select_mask_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, (const double*)d_FE,
                       (const int32_t*)d_count, (const double*)d_cost, 10 * S, d_x1, d_x2, N, thr2, d_mask, (EpiResult*)d_result);
    prof_mark(prof, CLC_KERNEL_PNP_SCORE, false, stream);
    return hipGetLastError();
}

hipError_t launch_epipolar(const double* d_F, int H, const double* d_x1, const double* d_x2, int N, double thr2, double* d_err,
                           int32_t* d_count, double* d_cost, hipStream_t stream, Profiler* prof)
{
    if (H <= 0 || N <= 0) return hipSuccess;
    prof_mark(prof, CLC_KERNEL_PNP_RESIDUALS, true, stream);
    if (d_err) hipLaunchKernelGGL(epipolar_residual_kernel, dim3((N + 255) / 256, H), dim3(256), 0, stream, d_F, d_x1, d_x2, N, d_err);
    else hipLaunchKernelGGL(epipolar_score_kernel, dim3(H), dim3(256), 0, stream, d_F, d_x1, d_x2, N, thr2, d_count, d_cost);
    prof_mark(prof, CLC_KERNEL_PNP_RESIDUALS, false, stream);
    return hipGetLastError();
}

hipError_t launch_pnp_residuals(const double* d_Rt, int H, const double* d_X, const double* d_x, int N,
                                const double* d_K, double* d_err, hipStream_t stream, Profiler* prof)
{
    if (H <= 0 || N <= 0) return hipSuccess;
    prof_mark(prof, CLC_KERNEL_PNP_RESIDUALS, true, stream);
    hipLaunchKernelGGL(pnp_residual_kernel, dim3((N + 255) / 256, H), dim3(256), 0, stream, d_Rt, d_X, d_x, N, d_K, d_err);
    prof_mark(prof, CLC_KERNEL_PNP_RESIDUALS, false, stream);
    return hipGetLastError();
}

hipError_t launch_pnp_score(const double* d_Rt, int H, const double* d_X, const double* d_x, int N,
                            const double* d_K, double thr2, int32_t* d_count, double* d_cost, hipStream_t stream,
                            Profiler* prof)
{
    if (H <= 0) return hipSuccess;
    prof_mark(prof, CLC_KERNEL_PNP_SCORE, true, stream);
    hipLaunchKernelGGL(pnp_score_kernel, dim3(H), dim3(256), 0, stream, d_Rt, d_X, d_x, N, d_K, thr2, d_count, d_cost);
    prof_mark(prof, CLC_KERNEL_PNP_SCORE, false, stream);
    return hipGetLastError();
}

} // namespace clc

// pose_prior.hip -- a tracked frame's pose from the PREDICTED pose and the tracks, without a minimal sample (include/coloc_hip.h:
// clc_track_prior_dev / clc_track_prior_batch_dev / clc_pnp_refine_prior, THE RULE there).  The project's own statement: the reference's
// intraPoseEstimator always calls Localize (coloc.hpp:223, Localizer.hpp:77-108).
//
// One workgroup of 512 threads per job (blockIdx.x = job), the shape of pnp_refine_kernel (pnp.hip), and that kernel's pass: residual,
// 2 x 6 Jacobian and 29 sums per pass, reduced in a fixed order through LDS, a 6 x 6 Cholesky solve by lane 0.  What is new around it:
//   the mask     is the kernel's own.  Thread t owns tracks t, t + 512, ... (at most 32 of the 16 384 a block holds), so a round's mask, the
//                classification at the parameters just evaluated and the one at the current parameters are three 32-bit words per thread
//                in registers -- no mask in LDS or global memory inside the loop; the bytes go out once, at the end.
//   classify     rides the pass: zc and sq of EVERY track are computed anyway before a masked-out track is skipped, so "in" is taken from
//                the very numbers the pass uses.  The three counts the rounds need (|mask|, |in|, |in xor mask|) travel in the 29th sum
//                as one exact double, n_mask + 2^16 n_in + 2^32 n_differ (each <= 16 384): no reduction of their own.
//   the count    N is read from the gather's DEVICE word (nothing on the host depends on it), clamped to the block's capacity.
// Sums in a fixed order, no floating-point atomics: two runs on the same inputs give the same bits, and a job's result does not depend
// on the jobs beside it.
#include "clc_ctx.h"
#include "so3.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

namespace clc {

namespace {

constexpr int kPriorSums = 29;        // 21 (upper JtWJ) + 6 (JtWr) + 1 (cost) + 1 (the three counts, packed)
constexpr int kPriorThreads = 512;
static_assert(kAcrMaxN <= 32 * kPriorThreads, "a thread's tracks must fit its 32-bit mask words");
constexpr double kInOne = 65536.0, kDifferOne = 4294967296.0;

__device__ __forceinline__ int prior_n_mask(const double packed) { return (int)((unsigned long long)packed & 0xFFFFull); }
__device__ __forceinline__ int prior_n_in(const double packed) { return (int)(((unsigned long long)packed >> 16) & 0xFFFFull); }
__device__ __forceinline__ int prior_n_differ(const double packed) { return (int)((unsigned long long)packed >> 32); }

__global__ __launch_bounds__(kPriorThreads) void pose_prior_kernel(const PriorJobs jobs)
{
    // fused multiply-adds as in pnp_refine_kernel (the result is held to a 50-digit reference by tolerance, tests/pose_prior_mp.py)
#pragma clang fp contract(fast)
    const PriorJobDev& jb = jobs.j[blockIdx.x];
    PriorOut* const out = jb.out;
    extern __shared__ double red[];     // [kPriorSums][kPriorThreads] reduction scratch (dynamic: 116 KB)
    __shared__ double s_par[6], s_try[6], s_R[9], s_dR[3][9], s_part[kPriorSums][16], s_tot[kPriorSums];
    __shared__ double s_A[kPriorSums];  // the sums at the CURRENT parameters s_par over the round's mask
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    int n_raw = jb.n_dev ? *jb.n_dev : jb.n;
    if (n_raw < 0) n_raw = 0;
    const int cap = jb.cap < kAcrMaxN ? jb.cap : kAcrMaxN;
    const int N = n_raw > cap ? (cap > 0 ? cap : 0) : n_raw;
    const double* __restrict__ X = jb.X;
    const double* __restrict__ x = jb.x;
    const double fx = jb.fx, sk = jb.sk, cx = jb.cx, fy = jb.fy, cy = jb.cy;
    const double huber_a = jb.huber_a, b2 = huber_a * huber_a, g2 = jb.g2;
    const int max_iter = jb.max_iter;
    if (tid == 0) {
        double R0[9] = { jb.Rt[0], jb.Rt[1], jb.Rt[2], jb.Rt[4], jb.Rt[5], jb.Rt[6], jb.Rt[8], jb.Rt[9], jb.Rt[10] };
        double w[3];
        log_so3(R0, w);
        s_par[0] = w[0]; s_par[1] = w[1]; s_par[2] = w[2]; s_par[3] = jb.Rt[3]; s_par[4] = jb.Rt[7]; s_par[5] = jb.Rt[11];
    }
    __syncthreads();

    // bit k of a word <-> track tid + 512 k.  m_bits: the round's mask; c_new: classify at the parameters of the pass just made;
    // c_cur: classify at s_par
    uint32_t m_bits = 0, c_new = 0, c_cur = 0;

    // pnp_refine_kernel's pass at parameters `par` over the tracks of m_bits -- front: over the tracks in front of the camera, which
    // become m_bits (the first pass: m_0) -- with every track classified on the way
    auto pass = [&](const double* par, const bool front) {
        if (tid < 64) {
            double Rl[9];
            rodrigues(par, Rl);
            if (tid < 9) s_R[tid] = Rl[tid];
            if (tid < 27) s_dR[tid / 9][tid % 9] = d_rodrigues_entry(par, Rl, tid / 9, tid % 9);
        }
        __syncthreads();
        double acc[kPriorSums];
#pragma unroll
        for (int i = 0; i < kPriorSums; ++i) acc[i] = 0.0;
        uint32_t cls = 0, msk = front ? 0u : m_bits;
        uint32_t bit = 1u;
        for (int i = tid; i < N; i += kPriorThreads, bit <<= 1) {
            const double X0 = X[3 * i], X1 = X[3 * i + 1], X2 = X[3 * i + 2];
            const double xc = s_R[0] * X0 + s_R[1] * X1 + s_R[2] * X2 + par[3];
            const double yc = s_R[3] * X0 + s_R[4] * X1 + s_R[5] * X2 + par[4];
            const double zc = s_R[6] * X0 + s_R[7] * X1 + s_R[8] * X2 + par[5];
            const double iz = 1.0 / zc, xn = xc * iz, yn = yc * iz;
            const double r0 = x[2 * i] - (fx * xn + sk * yn + cx), r1 = x[2 * i + 1] - (fy * yn + cy);
            const double sq = r0 * r0 + r1 * r1;
            const bool in = zc > 0.0 && sq <= g2;                            // classify: any NaN is "out", exactly g2 is "in"
            const bool used = front ? zc > 0.0 : (msk & bit) != 0u;
            if (in) cls |= bit;
            if (front && used) msk |= bit;
            acc[28] += (used ? 1.0 : 0.0) + (in ? kInOne : 0.0) + (in != used ? kDifferOne : 0.0);
            if (!used) continue;
            double rho = sq, wgt = 1.0;                                      // rho(s), rho'(s)
            if (sq > b2) {                                                   // Huber tail
                const double r = sqrt(sq);
                rho = 2.0 * huber_a * r - b2;
                wgt = huber_a / r;
            }
            acc[27] += 0.5 * rho;
            // d(proj)/d(xc,yc,zc)
            const double pu0 = fx * iz, pu1 = sk * iz, pu2 = -(fx * xn + sk * yn) * iz;
            const double pv1 = fy * iz, pv2 = -fy * yn * iz;
            double Ju[6], Jv[6];      // Jacobian of the PROJECTION (residual = obs - proj -> J_r = -J)
            // the 27 derivative entries are read from LDS per point (a broadcast read); hoisted out of the loop they take 54 VGPRs and
            // push the kernel over its 256-register budget into scratch -- the opaque offset stops that (pnp_refine_kernel's finding)
            int dro = 0;
            asm volatile("" : "+v"(dro));
            const double (*dRp)[9] = reinterpret_cast<const double (*)[9]>(&s_dR[0][0] + dro);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double d0 = dRp[k][0] * X0 + dRp[k][1] * X1 + dRp[k][2] * X2;
                const double d1 = dRp[k][3] * X0 + dRp[k][4] * X1 + dRp[k][5] * X2;
                const double d2 = dRp[k][6] * X0 + dRp[k][7] * X1 + dRp[k][8] * X2;
                Ju[k] = pu0 * d0 + pu1 * d1 + pu2 * d2;
                Jv[k] = pv1 * d1 + pv2 * d2;
            }
            Ju[3] = pu0; Ju[4] = pu1; Ju[5] = pu2;
            Jv[3] = 0.0; Jv[4] = pv1; Jv[5] = pv2;
            int idx = 0;
#pragma unroll
            for (int a_ = 0; a_ < 6; ++a_) {
#pragma unroll
                for (int b_ = a_; b_ < 6; ++b_) acc[idx++] += wgt * (Ju[a_] * Ju[b_] + Jv[a_] * Jv[b_]);
            }
#pragma unroll
            for (int a_ = 0; a_ < 6; ++a_) acc[21 + a_] += wgt * (Ju[a_] * r0 + Jv[a_] * r1);   // = -J_r^T W r : descent rhs
        }
        c_new = cls;
        if (front) m_bits = msk;
        // the 29 sums over the 512 threads THROUGH LDS, transposed (pnp_refine_kernel's measured reduction: ~3 k cycles against 16-18 k
        // for the shuffle tree): red[sum][thread], then 29 x 16 threads add 32 each, then 29 threads add the 16 partial results
#pragma unroll
        for (int i = 0; i < kPriorSums; ++i) red[i * kPriorThreads + tid] = acc[i];
        __syncthreads();
        if (tid < kPriorSums * 16) {
            const int i = tid >> 4, part = tid & 15;
            const double* src = red + i * kPriorThreads + part;
            double v = 0.0;
#pragma unroll 8
            for (int k = 0; k < kPriorThreads / 16; ++k) v += src[16 * k];
            s_part[i][part] = v;
        }
        __syncthreads();
        if (tid < kPriorSums) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) v += s_part[tid][k];
            s_tot[tid] = v;
        }
        __syncthreads();
    };

    // ONE call site of pass() (inlined: a second copy costs spilled VGPRs at the 256-register budget of a 512-thread workgroup).  What a
    // trip evaluates: START -- s_par over a round's mask, the sums its Levenberg-Marquardt starts from; TRIAL -- s_try, pnp_refine_kernel's
    // loop "step -> [flag] -> evaluate -> accept / reject"; FINAL -- s_par over classify(s_par) where the last sums are over another mask.
    enum { START, TRIAL, FINAL };
    int phase = START, it = 0, it_total = 0, round = 0, rounds_run = 0;
    bool front = true, moved = false, converged = false;
    double lambda = 1e-4, cost = 0.0;
    for (;;) {
        pass(phase == TRIAL ? s_try : s_par, front);
        front = false;
        bool ended = false;                                   // the round's minimisation is over (or there is none: fewer than 4 tracks)
        if (phase != TRIAL) {
            if (tid < kPriorSums) s_A[tid] = s_tot[tid];
            __syncthreads();
            c_cur = c_new;
            if (phase == FINAL) break;
            cost = s_A[27];
            lambda = 1e-4;                                    // reset at the start of every round
            it = 0;
            phase = TRIAL;
            if (prior_n_mask(s_A[28]) < 4) ended = true;
            else ++rounds_run;
        } else {
            const double new_cost = s_tot[27];
            if (new_cost < cost) {
                const double rel = (cost - new_cost) / fmax(cost, 1e-300);
                if (tid < 6) s_par[tid] = s_try[tid];
                if (tid < kPriorSums) s_A[tid] = s_tot[tid];
                cost = new_cost;
                lambda = fmax(lambda * 0.1, 1e-12);
                c_cur = c_new;
                moved = true;
                __syncthreads();
                if (rel < 1e-8) ended = true;                 // function tolerance 1e-8
            } else {
                lambda *= 10.0;
                __syncthreads();
                if (lambda > 1e10) { ended = true; --it; }   // (the stop above 1e10 is not counted, as in pnp_refine_kernel)
            }
            ++it;
        }
        // the next step (a failed factorization counts as a rejected step: lambda up, try again)
        while (!ended) {
            if (!(it < max_iter)) { ended = true; break; }
            if (tid == 0) {
                double g[6], d[6];
                for (int a_ = 0; a_ < 6; ++a_) g[a_] = s_A[21 + a_];
                const bool ok = solve6(s_A, g, lambda, d);
                double gn = 0, dn = 0, pn = 0;
                for (int a_ = 0; a_ < 6; ++a_) { gn = fmax(gn, fabs(g[a_])); dn += d[a_] * d[a_]; pn += s_par[a_] * s_par[a_]; }
                // gradient / parameter tolerance 1e-8
                s_flag = !ok ? 2 : ((gn < 1e-8 * fmax(1.0, cost) || sqrt(dn) < 1e-8 * (sqrt(pn) + 1e-8)) ? 1 : 0);
                for (int a_ = 0; a_ < 6; ++a_) s_try[a_] = s_par[a_] + (ok ? d[a_] : 0.0);
            }
            __syncthreads();
            const int flag = s_flag;
            if (flag == 1) { ended = true; break; }
            if (flag == 2) {
                lambda *= 10.0;
                if (lambda > 1e10) { ended = true; break; }
                __syncthreads();
                ++it;
                continue;
            }
            break;
        }
        if (!ended) continue;
        // the round is over: s_A holds the sums at s_par over m_bits, c_cur = classify(s_par)
        it_total += it;
        const double counts = s_A[28];
        const bool ran = prior_n_mask(counts) >= 4;
        if (prior_n_differ(counts) == 0) { converged = ran; break; }      // the mask is stable: these sums are the final ones
        m_bits = c_cur;
        ++round;
        phase = (ran && round < jb.rounds && prior_n_in(counts) >= 4) ? START : FINAL;
    }

    // s_A: the sums at s_par over classify(s_par) = c_cur
    const int n_in = prior_n_in(s_A[28]);
    const int need = jb.min_inliers > 4 ? jb.min_inliers : 4;
    const bool few = n_in < need;
    if (tid < 6) {
        if (few || !invert6_column(s_A, tid, out->cov)) for (int r = 0; r < 6; ++r) out->cov[6 * r + tid] = 0.0;
    }
    if (tid == 0) {
        if (moved) {
            double R[9];
            rodrigues(s_par, R);
            for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) out->Rt[4 * i + j] = R[3 * i + j]; out->Rt[4 * i + 3] = s_par[3 + i]; }
        } else {
            for (int i = 0; i < 12; ++i) out->Rt[i] = jb.Rt[i];          // no step was accepted: the prior, bit for bit
        }
        out->cost = s_A[27];
        out->rmse = n_in > 0 ? sqrt(s_A[27] / (2.0 * (double)n_in)) : 0.0;
        out->n_tracks = n_raw;
        out->n_inliers = n_in;
        out->iterations = it_total;
        out->rounds_run = rounds_run;
        out->converged = converged ? 1 : 0;
        out->result = few ? 1 : 0;
        out->capacity = n_raw > cap ? 1 : 0;
    }
    if (jb.h_mask) {
        uint32_t bit = 1u;
        for (int i = tid; i < N; i += kPriorThreads, bit <<= 1) jb.h_mask[i] = (c_cur & bit) ? 1 : 0;
    }
    __threadfence_system();                 // every writer: its stores to the pinned record and mask have left
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&out->ready, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

} // namespace

hipError_t launch_pose_prior(const PriorJobs& jobs, const int n_jobs, hipStream_t stream)
{
    if (n_jobs < 1 || n_jobs > kMaxBatch) return hipErrorInvalidValue;
    constexpr size_t kRedBytes = sizeof(double) * kPriorSums * kPriorThreads;
    static bool attr_set[64] = {};      // per device: more than the 64 KB a kernel gets by default
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_set[dev]) {
        const hipError_t e = hipFuncSetAttribute((const void*)pose_prior_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRedBytes);
        if (e != hipSuccess) return e;
        attr_set[dev] = true;
    }
    hipLaunchKernelGGL(pose_prior_kernel, dim3(n_jobs), dim3(kPriorThreads), kRedBytes, stream, jobs);
    return hipGetLastError();
}

} // namespace clc

using namespace clc;

namespace {

// The step's arguments, checked (CLC_ERR_BAD_ARG on `who`) and with their defaults, into the kernel's job
int prior_step(clc_ctx* ctx, const char* who, const double* Rt, const double gate, const double huber_a, const int rounds, const int max_iter,
               const int min_inliers, PriorJobDev& d)
{
    const auto bad = [&](const char* what) { return fail(ctx, CLC_ERR_BAD_ARG, (std::string(who) + what).c_str()); };
    for (int i = 0; i < 12; ++i) if (!std::isfinite(Rt[i])) return bad(": the prior is not finite");
    const double g2 = gate * gate;
    if (!(std::isfinite(gate) && gate > 0.0 && std::isfinite(g2) && g2 > 0.0)) return bad(": gate and gate * gate must be finite and positive");
    if (rounds < 0 || rounds > 8) return bad(": rounds outside 0 .. 8");
    if (max_iter < 0) return bad(": negative max_iter");
    memcpy(d.Rt, Rt, sizeof d.Rt);
    d.g2 = g2;
    d.huber_a = huber_a > 0.0 ? huber_a : 16.0;          // ceres::HuberLoss(Square(4.0)), as clc_pnp_refine
    d.rounds = rounds ? rounds : 4;
    d.max_iter = max_iter ? max_iter : 50;
    d.min_inliers = min_inliers > 0 ? min_inliers : 8;
    return CLC_OK;
}

void prior_reset(clc_track_prior_job& jb)
{
    bool finite = true;
    for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(jb.Rt_prior[i]);
    if (jb.Rt) { if (finite) memcpy(jb.Rt, jb.Rt_prior, sizeof(double) * 12); else memset(jb.Rt, 0, sizeof(double) * 12); }
    if (jb.cov) memset(jb.cov, 0, sizeof(double) * 36);
    jb.n_tracks = 0; jb.n_inliers = 0; jb.iterations = 0; jb.rounds_run = 0; jb.converged = 0; jb.result = CLC_TRACK_PRIOR_FEW;
    jb.status = CLC_OK; jb.rmse = 0.0;
}

// Every job of a batch: the checks, the blocks, ONE gather launch, ONE solve launch on ctxs[0]'s stream, one wait per record
int track_prior(clc_ctx* const* ctxs, clc_track_prior_job* jobs, const int n_jobs)
{
    clc_ctx* c0 = ctxs[0];
    TrackJobs pack{};
    PriorJobs solve{};
    for (int i = 0; i < n_jobs; ++i) prior_reset(jobs[i]);
    // everything is checked before anything is enqueued
    for (int i = 0; i < n_jobs; ++i) {
        clc_track_prior_job& jb = jobs[i];
        clc_track_job frame{};
        frame.d_match = jb.d_match; frame.nq = jb.nq; frame.d_count = jb.d_count; frame.d_kps = jb.d_kps; frame.d_feat = jb.d_feat;
        frame.feat_stride = jb.feat_stride; frame.cam = jb.cam;
        int rc = gather_inputs(c0, frame, pack.j[i], "track_prior: bad argument");
        if (rc == CLC_OK) rc = prior_step(c0, "track_prior", jb.Rt_prior, jb.gate, jb.huber_a, jb.rounds, jb.max_iter, jb.min_inliers, solve.j[i]);
        if (rc != CLC_OK) {
            if (ctxs[i] != c0) (void)fail(ctxs[i], rc, clc_last_error_string(c0));
            jb.status = rc;
            return rc;
        }
    }
    CLC_HIP(c0, hipSetDevice(c0->device));
    hipStream_t st = c0->stream;
    PriorPin pins[kMaxBatch];
    for (int i = 0; i < n_jobs; ++i) {
        const size_t cap = (size_t)std::min(jobs[i].nq, kAcrMaxN);
        int rc = ensure_gather(ctxs[i], ctxs[i]->trk, cap, kTrackLayout);
        if (rc == CLC_OK) rc = ensure_pinned(ctxs[i], [&](Carve& c) { pins[i].carve(c, cap, sizeof(PriorOut)); });
        if (rc != CLC_OK) {
            if (ctxs[i] != c0) (void)fail(c0, rc, clc_last_error_string(ctxs[i]));
            jobs[i].status = rc;
            return rc;
        }
    }
    // behind whatever produced the inputs: an event on the producer's stream, no host synchronisation
    for (int i = 0; i < n_jobs; ++i) {
        hipStream_t prod = (hipStream_t)jobs[i].after_stream;
        if (prod && prod != st) CLC_HIP(ctxs[i], order_behind(ctxs[i]->ev_track, prod, &st, 1));
    }
    pack.map_X = c0->d_map_X.as<double>(); pack.map_n = c0->map_X_n;
    for (int i = 0; i < n_jobs; ++i) {
        const clc_track_prior_job& jb = jobs[i];
        const GatherView v(ctxs[i]->trk, kTrackLayout);
        TrackJobDev& d = pack.j[i];
        d.n = v.n; d.h_n = nullptr;                           // the count stays on the device: nothing on the host depends on it
        d.cap = std::min(jb.nq, kAcrMaxN);
        d.X = v.a; d.x = v.b; d.query = v.q; d.map = v.t;
        d.h_query = jb.track_query ? v.h_q : nullptr;
        d.h_map = jb.track_map ? v.h_t : nullptr;
        PriorJobDev& s = solve.j[i];
        s.X = v.a; s.x = v.b; s.n_dev = v.n; s.n = 0; s.cap = d.cap;
        s.fx = jb.cam.focal; s.sk = 0.0; s.cx = jb.cam.ppx; s.fy = jb.cam.focal; s.cy = jb.cam.ppy;      // Pinhole_Intrinsic_Radial_K3::K()
        s.h_mask = pins[i].mask; s.out = (PriorOut*)pins[i].rec;
        __atomic_store_n(&s.out->ready, 0, __ATOMIC_RELAXED);
    }
    CLC_HIP(c0, launch_gather(pack, n_jobs, st));
    CLC_HIP(c0, launch_pose_prior(solve, n_jobs, st));
    // the one wait: the record, which the solve writes last (the stream synchronisation as the fallback, which also surfaces errors)
    const auto t0 = std::chrono::steady_clock::now();
    int first = CLC_OK;
    for (int i = 0; i < n_jobs; ++i) {
        const PriorOut* rec = solve.j[i].out;
        if (const int rc = wait_pinned(c0, &rec->ready, (int32_t)0, st, t0, 5, "track_prior: the solve left no record")) return rc;
        clc_track_prior_job& jb = jobs[i];
        jb.n_tracks = rec->n_tracks;
        if (rec->capacity) {
            jb.status = fail(ctxs[i], CLC_ERR_CAPACITY, "track_prior: more than 16384 tracks");
            if (first == CLC_OK) first = jb.status;
            continue;
        }
        if (jb.Rt) memcpy(jb.Rt, rec->Rt, sizeof rec->Rt);
        if (jb.cov) memcpy(jb.cov, rec->cov, sizeof rec->cov);
        jb.n_inliers = rec->n_inliers; jb.iterations = rec->iterations; jb.rounds_run = rec->rounds_run; jb.converged = rec->converged;
        jb.result = rec->result; jb.rmse = rec->rmse;
        // the gather wrote the track mirrors before the solve started, the solve its mask before the record
        const GatherView v(ctxs[i]->trk, kTrackLayout);
        const size_t n = (size_t)std::min(std::max(rec->n_tracks, 0), solve.j[i].cap);
        if (jb.track_query && n) memcpy(jb.track_query, v.h_q, sizeof(int32_t) * n);
        if (jb.track_map && n) memcpy(jb.track_map, v.h_t, sizeof(int32_t) * n);
        if (jb.inlier_mask && n) memcpy(jb.inlier_mask, solve.j[i].h_mask, n);
    }
    return first;
}

} // namespace

extern "C" {

int clc_track_prior_batch_dev(clc_ctx* const* ctxs, clc_track_prior_job* jobs, int n_jobs)
{
    if (n_jobs < 0 || n_jobs > CLC_MAX_BATCH || (n_jobs > 0 && (!ctxs || !jobs))) return CLC_ERR_BAD_ARG;
    if (n_jobs == 0) return CLC_OK;
    const int rc0 = check_batch_contexts(ctxs, n_jobs, "track_prior_batch: every job needs a context of its own");
    if (rc0 != CLC_OK) return rc0;
    return track_prior(ctxs, jobs, n_jobs);
}

int clc_track_prior_dev(clc_ctx* ctx, clc_track_prior_job* job)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "track_prior: null context / job");
    return track_prior(&ctx, job, 1);
}

int clc_pnp_refine_prior(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, const double* h_Rt_prior,
                         double gate, double huber_a, int rounds, int max_iter, int min_inliers, double* h_Rt, double* h_cov,
                         uint8_t* h_inlier_mask, int* n_inliers, double* rmse, int* iterations, int* rounds_run, int* converged,
                         int* result)
{
    if (!ctx || N < 0 || !h_K || !h_Rt_prior || (N > 0 && (!h_X || !h_x))) return fail(ctx, CLC_ERR_BAD_ARG, "pnp_refine_prior: bad argument");
    if (!pose_K_ok(h_K)) return fail(ctx, CLC_ERR_BAD_ARG, "pnp_refine_prior: K must be { fx, skew, cx; 0, fy, cy; 0, 0, 1 }");
    PriorJobs solve{};
    PriorJobDev& s = solve.j[0];
    const int rc0 = prior_step(ctx, "pnp_refine_prior", h_Rt_prior, gate, huber_a, rounds, max_iter, min_inliers, s);
    if (rc0 != CLC_OK) return rc0;
    if (N > kAcrMaxN) return fail(ctx, CLC_ERR_CAPACITY, "pnp_refine_prior: more than 16384 correspondences");
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    PriorHostDev dv; PriorHostPin pin;
    int rc = ensure_pnp(ctx, [&](Carve& c) { dv.carve(c, (size_t)N); });
    if (rc == CLC_OK) rc = ensure_pinned(ctx, [&](Carve& c) { pin.carve(c, (size_t)N, sizeof(PriorOut)); });
    if (rc != CLC_OK) return rc;
    if (N > 0) {
        memcpy(pin.in.X, h_X, sizeof(double) * 3 * N);
        memcpy(pin.in.x, h_x, sizeof(double) * 2 * N);
        CLC_HIP(ctx, hipMemcpyAsync(dv.in.X, pin.in.X, pin.in.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    s.X = dv.in.X; s.x = dv.in.x; s.n_dev = nullptr; s.n = N; s.cap = N;
    s.fx = h_K[0]; s.sk = h_K[1]; s.cx = h_K[2]; s.fy = h_K[4]; s.cy = h_K[5];
    s.h_mask = pin.out.mask; s.out = (PriorOut*)pin.out.rec;
    __atomic_store_n(&s.out->ready, 0, __ATOMIC_RELAXED);
    CLC_HIP(ctx, launch_pose_prior(solve, 1, ctx->stream));
    if (const int rcw = wait_pinned(ctx, &s.out->ready, (int32_t)0, ctx->stream, std::chrono::steady_clock::now(), 5, "pnp_refine_prior: the solve left no record"))
        return rcw;
    const PriorOut& r = *s.out;
    if (h_Rt) memcpy(h_Rt, r.Rt, sizeof r.Rt);
    if (h_cov) memcpy(h_cov, r.cov, sizeof r.cov);
    if (h_inlier_mask && N > 0) memcpy(h_inlier_mask, pin.out.mask, (size_t)N);
    if (n_inliers) *n_inliers = r.n_inliers;
    if (rmse) *rmse = r.rmse;
    if (iterations) *iterations = r.iterations;
    if (rounds_run) *rounds_run = r.rounds_run;
    if (converged) *converged = r.converged;
    if (result) *result = r.result;
    return CLC_OK;
}

} // extern "C"

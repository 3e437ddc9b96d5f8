// pose_prior.hip -- a tracked frame's pose from the PREDICTED pose and the tracks, without a minimal sample (include/coloc_hip.h:
// clc_track_prior_dev / clc_track_prior_batch_dev / clc_pnp_refine_prior, THE RULE there).  The project's own statement: the reference's
// intraPoseEstimator always calls Localize (coloc.hpp:223, Localizer.hpp:77-108).
//
// One workgroup of 512 threads per job (blockIdx.x = job).  The Levenberg-Marquardt pass, its bookkeeping and the record are pose_lm.h's
// (shared with pnp_refine_kernel, pnp.hip).  What is this kernel's own around them:
//   the mask     Thread t owns tracks t, t + 512, ... (at most 32 of the 16 384 a block holds), so a round's mask, the classification at
//                the parameters just evaluated and the one at the current parameters are three 32-bit words per thread in registers --
//                no mask in LDS or global memory inside the loop; the bytes go out once, at the end.
//   classify     rides the pass: zc and sq of EVERY track are computed anyway before a masked-out track is skipped, so "in" is taken from
//                the very numbers the pass uses.  The three counts the rounds need (|mask|, |in|, |in xor mask|) travel in the 29th sum
//                as one exact double, n_mask + 2^16 n_in + 2^32 n_differ (each <= 16 384): no reduction of their own.
//   the count    N is read from the gather's DEVICE word (nothing on the host depends on it), clamped to the block's capacity.
//   the rounds   START / TRIAL / FINAL below; few, moved, converged, capacity in the record.
// A job's result does not depend on the jobs beside it.
#include "clc_ctx.h"
#include "pose_lm.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

namespace clc {

namespace {

static_assert(kAcrMaxN <= 32 * kPoseThreads, "a thread's tracks must fit its 32-bit mask words");
constexpr double kInOne = 65536.0, kDifferOne = 4294967296.0;

__device__ __forceinline__ int prior_n_mask(const double packed) { return (int)((unsigned long long)packed & 0xFFFFull); }
__device__ __forceinline__ int prior_n_in(const double packed) { return (int)(((unsigned long long)packed >> 16) & 0xFFFFull); }
__device__ __forceinline__ int prior_n_differ(const double packed) { return (int)((unsigned long long)packed >> 32); }

__global__ __launch_bounds__(kPoseThreads) void pose_prior_kernel(const PriorJobs jobs)
{
#pragma clang fp contract(fast)
    const PriorJobDev& jb = jobs.j[blockIdx.x];
    PriorOut* const out = jb.out;
    extern __shared__ double red[];     // pose_reduce's scratch (kPoseRedBytes)
    __shared__ PoseLds s;               // s.A: the sums at the CURRENT parameters s.par over the round's mask
    const int tid = threadIdx.x;
    int n_raw = jb.n_dev ? *jb.n_dev : jb.n;
    if (n_raw < 0) n_raw = 0;
    const int cap = jb.cap < kAcrMaxN ? jb.cap : kAcrMaxN;
    const int N = n_raw > cap ? (cap > 0 ? cap : 0) : n_raw;
    const double* __restrict__ X = jb.X;
    const double* __restrict__ x = jb.x;
    const PoseCam cam = { jb.fx, jb.sk, jb.cx, jb.fy, jb.cy, jb.huber_a, jb.huber_a * jb.huber_a };
    const double g2 = jb.g2;
    const int max_iter = jb.max_iter;
    pose_start(s, tid, jb.Rt);

    // bit k of a word <-> track tid + 512 k.  m_bits: the round's mask; c_new: classify at the parameters of the pass just made;
    // c_cur: classify at s.par
    uint32_t m_bits = 0, c_new = 0, c_cur = 0;

    // the pass at parameters `par` over the tracks of m_bits -- front: over the tracks in front of the camera, which become m_bits
    // (the first pass: m_0) -- with every track classified on the way
    auto pass = [&](const double* par, const bool front) {
        pose_rotation(s, tid, par);
        double acc[kPoseSums];
#pragma unroll
        for (int i = 0; i < kPoseSums; ++i) acc[i] = 0.0;
        uint32_t cls = 0, msk = front ? 0u : m_bits;
        uint32_t bit = 1u;
        for (int i = tid; i < N; i += kPoseThreads, bit <<= 1) {
            const PosePoint p = pose_residual(s, par, cam, X, x, i);
            const bool in = p.zc > 0.0 && p.sq <= g2;                        // classify: any NaN is "out", exactly g2 is "in"
            const bool used = front ? p.zc > 0.0 : (msk & bit) != 0u;
            if (in) cls |= bit;
            if (front && used) msk |= bit;
            acc[28] += (used ? 1.0 : 0.0) + (in ? kInOne : 0.0) + (in != used ? kDifferOne : 0.0);
            if (!used) continue;
            pose_accumulate(s, cam, p, acc);
        }
        c_new = cls;
        if (front) m_bits = msk;
        pose_reduce(s, red, tid, acc);
    };

    // ONE call site of pass().  What a trip evaluates: START -- s.par over a round's mask, the sums its Levenberg-Marquardt starts
    // from; TRIAL -- s.try_, the loop "step -> [flag] -> evaluate -> accept / reject"; FINAL -- s.par over classify(s.par) where the
    // last sums are over another mask.
    enum { START, TRIAL, FINAL };
    int phase = START, it_total = 0, round = 0, rounds_run = 0;
    bool front = true, moved = false, converged = false;
    LmState lm;
    for (;;) {
        pass(phase == TRIAL ? s.try_ : s.par, front);
        front = false;
        bool ended = false;                                   // the round's minimisation is over (or there is none: fewer than 4 tracks)
        if (phase != TRIAL) {
            pose_keep_sums(s, tid);
            c_cur = c_new;
            if (phase == FINAL) break;
            lm = LmState();                                   // lambda and the count start again with every round
            lm.cost = s.A[27];
            phase = TRIAL;
            if (prior_n_mask(s.A[28]) < 4) ended = true;
            else ++rounds_run;
        } else {
            bool accepted;
            ended = lm_judge(s, tid, lm, accepted);
            if (accepted) { c_cur = c_new; moved = true; }
        }
        if (!ended) ended = lm_next_step(s, tid, lm, max_iter);
        if (!ended) continue;
        // the round is over: s.A holds the sums at s.par over m_bits, c_cur = classify(s.par)
        it_total += lm.it;
        const double counts = s.A[28];
        const bool ran = prior_n_mask(counts) >= 4;
        if (prior_n_differ(counts) == 0) { converged = ran; break; }      // the mask is stable: these sums are the final ones
        m_bits = c_cur;
        ++round;
        phase = (ran && round < jb.rounds && prior_n_in(counts) >= 4) ? START : FINAL;
    }

    // s.A: the sums at s.par over classify(s.par) = c_cur
    const int n_in = prior_n_in(s.A[28]);
    const int need = jb.min_inliers > 4 ? jb.min_inliers : 4;
    const bool few = n_in < need;
    pose_cov_column(s, tid, !few, out->cov);
    if (tid == 0) {
        if (moved) pose_Rt(s, out->Rt);
        else for (int i = 0; i < 12; ++i) out->Rt[i] = jb.Rt[i];          // no step was accepted: the prior, bit for bit
        out->cost = s.A[27];
        out->rmse = pose_rmse(s.A[27], (double)n_in);
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
        for (int i = tid; i < N; i += kPoseThreads, bit <<= 1) jb.h_mask[i] = (c_cur & bit) ? 1 : 0;
    }
    pose_publish(tid, &out->ready);
}

} // namespace

hipError_t launch_pose_prior(const PriorJobs& jobs, const int n_jobs, hipStream_t stream)
{
    if (n_jobs < 1 || n_jobs > kMaxBatch) return hipErrorInvalidValue;
    const hipError_t e = pose_allow_lds<pose_prior_kernel>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pose_prior_kernel, dim3(n_jobs), dim3(kPoseThreads), kPoseRedBytes, stream, jobs);
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

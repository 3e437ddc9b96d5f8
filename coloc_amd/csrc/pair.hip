// pair.hip -- the gather of RobustMatcher::computeRelativePose (reference include/coloc/RobustMatcher.hpp:372-424, the loop at :393-398)
// on the device: from a pair's d_match and the two cameras' keypoints (or blocks of feature positions) to the undistorted
// correspondences x1 / x2 the a-contrario two-view solve starts from (pose_batch.hip: clc_pair_filter*_dev), without the pair going
// through the host.  track.hip's twin: the same ordered compaction, two 2-D sides instead of a 2-D and a 3-D one.
//
// One launch for a batch of pairs, blockIdx.y = pair, ONE workgroup per pair: nq <= maxkp is 5-10 k (the solve takes at most 16 384
// correspondences), a few KB in and a few tens of KB out -- the launch is latency-bound, and one workgroup keeps the ordered compaction
// a matter of one ballot per wave and one 16-entry LDS scan per 1 024 queries.  The points leave in PIXELS: the 'F' / 'H' conditioning
// is the staging launch's (acransac.hip: acr_stage_kernel), so the block and its pinned mirrors serve all three models.
#include "clc_ctx.h"
#include "ud_pixel.h"

#include <cmath>
#include <cstring>

namespace clc {

namespace {

constexpr int kPairThreads = 1024;

__global__ __launch_bounds__(kPairThreads) void pair_build_kernel(const PairJobs jobs)
{
    const PairJobDev& jb = jobs.j[blockIdx.y];
    __shared__ uint32_t s_wave[kPairThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t nq = jb.nq > 0 ? (uint32_t)jb.nq : 0u;
    if (jb.a.count) { const uint32_t c = jb.a.count[0]; nq = c < nq ? c : nq; }
    int32_t nt = jb.nt > 0 ? jb.nt : 0;
    if (jb.b.count) { const uint32_t c = jb.b.count[0]; nt = c < (uint32_t)nt ? (int32_t)c : nt; }
    uint32_t base = 0;                                   // pairs of the queries before this pass (the same in every thread)
    for (uint32_t q0 = 0; q0 < nq; q0 += kPairThreads) {
        const uint32_t q = q0 + tid;
        const int32_t m = q < nq ? jb.match[q] : -1;
        const bool ok = m >= 0 && m < nt;
        // ordered compaction: accepted lanes below this one in the wave (ballot + mbcnt), accepted queries of the waves before it (LDS)
        const uint64_t b = __ballot(ok);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t off = base, total = 0;
        for (uint32_t w = 0; w < kPairThreads / 64; ++w) {
            const uint32_t c = s_wave[w];
            off += w < wave ? c : 0u;
            total += c;
        }
        __syncthreads();                                 // (s_wave is written again in the next pass)
        const uint32_t i = off + before;
        if (ok && i < (uint32_t)jb.cap) {
            float fx, fy;
            double u1[2], u2[2];
            feature_position(jb.a.kps, jb.a.feat, jb.a.feat_stride, q, jobs.scale, &fx, &fy);
            ud_pixel(fx, fy, UdCamera{ jb.a.focal, jb.a.ppx, jb.a.ppy, jb.a.k1, jb.a.k2, jb.a.k3 }, u1);
            feature_position(jb.b.kps, jb.b.feat, jb.b.feat_stride, (uint32_t)m, jobs.scale, &fx, &fy);
            ud_pixel(fx, fy, UdCamera{ jb.b.focal, jb.b.ppx, jb.b.ppy, jb.b.k1, jb.b.k2, jb.b.k3 }, u2);
            jb.x1[2 * (size_t)i] = u1[0]; jb.x1[2 * (size_t)i + 1] = u1[1];
            jb.x2[2 * (size_t)i] = u2[0]; jb.x2[2 * (size_t)i + 1] = u2[1];
            if (jb.pair_q) jb.pair_q[i] = (int32_t)q;
            if (jb.pair_t) jb.pair_t[i] = m;
            if (jb.h_q) jb.h_q[i] = (int32_t)q;
            if (jb.h_t) jb.h_t[i] = m;
            if (jb.h_x1) { jb.h_x1[2 * (size_t)i] = u1[0]; jb.h_x1[2 * (size_t)i + 1] = u1[1]; }
            if (jb.h_x2) { jb.h_x2[2 * (size_t)i] = u2[0]; jb.h_x2[2 * (size_t)i + 1] = u2[1]; }
        }
        base += total;
    }
    // the count comes out last: every wave's stores (device blocks and pinned mirrors) are complete and visible system-wide before the
    // word the host polls changes
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        if (jb.n) *jb.n = (int32_t)base;
        if (jb.h_n) __hip_atomic_store(jb.h_n, base, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

int pair_side(clc_ctx* ctx, const uint32_t* count, const clc_keypoint* kps, const float* feat, const int stride, const clc_camera_k3& cam,
              PairSideDev& out)
{
    if ((kps != nullptr) == (feat != nullptr)) return fail(ctx, CLC_ERR_BAD_ARG, "pair: exactly one of d_kps / d_feat per camera");
    if (feat && stride < 2) return fail(ctx, CLC_ERR_BAD_ARG, "pair: feat_stride < 2");
    if (((uintptr_t)kps & 3u) || ((uintptr_t)feat & 3u) || ((uintptr_t)count & 3u)) return fail(ctx, CLC_ERR_BAD_ARG, "pair: misaligned device pointer");
    if (!(cam.focal > 0.0)) return fail(ctx, CLC_ERR_BAD_ARG, "pair: focal must be positive");
    out.count = count; out.kps = kps; out.feat = feat; out.feat_stride = stride;
    out.focal = cam.focal; out.ppx = cam.ppx; out.ppy = cam.ppy; out.k1 = cam.k1; out.k2 = cam.k2; out.k3 = cam.k3;
    return CLC_OK;
}

} // namespace

hipError_t launch_pair_build(PairJobs& jobs, const int n_jobs, hipStream_t stream)
{
    if (n_jobs < 1 || n_jobs > kMaxBatch) return hipErrorInvalidValue;
    // GPUDetector.hpp:173 through clc_keypoints_to_features: pow(float, integer) evaluated in double, rounded to float -- on the host
    for (int l = 0; l < CLC_MAX_LEVELS; ++l) jobs.scale[l] = (float)std::pow((double)1.2f, (double)l);
    hipLaunchKernelGGL(pair_build_kernel, dim3(1, n_jobs), dim3(kPairThreads), 0, stream, jobs);
    return hipGetLastError();
}

int pair_job_inputs(clc_ctx* ctx, const clc_pair_job& job, PairJobDev& out, const char* who)
{
    out = PairJobDev{};
    if (job.nq < 0 || job.nt < 0 || (job.nq > 0 && !job.d_match)) return fail(ctx, CLC_ERR_BAD_ARG, who);
    if ((uintptr_t)job.d_match & 3u) return fail(ctx, CLC_ERR_BAD_ARG, "pair: misaligned device pointer");
    int rc = pair_side(ctx, job.d_count_a, job.d_kps_a, job.d_feat_a, job.feat_stride_a, job.cam_a, out.a);
    if (rc == CLC_OK) rc = pair_side(ctx, job.d_count_b, job.d_kps_b, job.d_feat_b, job.feat_stride_b, job.cam_b, out.b);
    if (rc != CLC_OK) return rc;
    out.match = job.d_match; out.nq = job.nq; out.nt = job.nt;
    return CLC_OK;
}

int ensure_pair(clc_ctx* ctx, size_t cap)
{
    cap = (cap + 63) & ~(size_t)63;
    if (cap < 64) cap = 64;
    if (cap <= ctx->pair_cap && ctx->d_pair && ctx->h_pair) return CLC_OK;
    // (nothing of an earlier call is in flight: a pair filter returns after its staging launch has consumed the block)
    if (ctx->d_pair) { (void)hipFree(ctx->d_pair); ctx->d_pair = nullptr; }
    if (ctx->h_pair) { (void)hipHostFree(ctx->h_pair); ctx->h_pair = nullptr; }
    ctx->pair_cap = 0;
    const size_t body = cap * (4 * sizeof(double) + 2 * sizeof(int32_t));
    CLC_HIP(ctx, hipMalloc((void**)&ctx->d_pair, body + 64));
    CLC_HIP(ctx, hipHostMalloc((void**)&ctx->h_pair, 64 + body, hipHostMallocDefault));
    memset(ctx->h_pair, 0xFF, 64);
    ctx->pair_cap = cap;
    return CLC_OK;
}

} // namespace clc

using namespace clc;

extern "C" {

int clc_pair_build_dev(clc_ctx* ctx, const clc_pair_job* job, double* d_x1, double* d_x2, int32_t* d_pair_q, int32_t* d_pair_t, int32_t* d_n,
                       void* stream)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "pair_build: null context / job");
    PairJobs jobs{};
    const int rc = pair_job_inputs(ctx, *job, jobs.j[0], "pair_build: bad argument");
    if (rc != CLC_OK) return rc;
    if (job->nq > 0 && (!d_x1 || !d_x2)) return fail(ctx, CLC_ERR_BAD_ARG, "pair_build: null output");
    if (((uintptr_t)d_x1 & 7u) || ((uintptr_t)d_x2 & 7u) || ((uintptr_t)d_pair_q & 3u) || ((uintptr_t)d_pair_t & 3u) || ((uintptr_t)d_n & 3u))
        return fail(ctx, CLC_ERR_BAD_ARG, "pair_build: misaligned device pointer");
    if (job->nq == 0 && !d_n) return CLC_OK;
    jobs.j[0].x1 = d_x1; jobs.j[0].x2 = d_x2; jobs.j[0].pair_q = d_pair_q; jobs.j[0].pair_t = d_pair_t; jobs.j[0].n = d_n;
    jobs.j[0].cap = job->nq;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    CLC_HIP(ctx, launch_pair_build(jobs, 1, pick(ctx, stream)));
    return CLC_OK;
}

} // extern "C"

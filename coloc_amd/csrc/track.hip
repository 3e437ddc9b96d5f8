// track.hip -- Localizer::setupTracks (reference include/coloc/Localizer.hpp:59-75) on the device: from the map matcher's d_match, the
// detector's keypoints (or a block of feature positions) and the map's 3-D points to the correspondences the a-contrario pose solve
// starts from (pose_batch.hip: clc_track_localize*_dev), without the frame going through the host.
//
// One launch for a batch of cameras, blockIdx.y = camera, ONE workgroup per camera: nq <= maxkp is 5-10 k (the solve takes at most
// 16 384 tracks), a few KB in and a few tens of KB out -- the launch is latency-bound, and one workgroup keeps the ordered compaction a
// matter of one ballot per wave and one 16-entry LDS scan per 1 024 queries.  The undistortion's loops are data-dependent and diverge;
// at this size that does not matter.
#include "clc_ctx.h"
#include "ud_pixel.h"

#include <cmath>
#include <cstring>

namespace clc {

namespace {

constexpr int kTrackThreads = 1024;

__global__ __launch_bounds__(kTrackThreads) void track_build_kernel(const TrackJobs jobs)
{
    const TrackJobDev& jb = jobs.j[blockIdx.y];
    __shared__ uint32_t s_wave[kTrackThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t nq = jb.nq > 0 ? (uint32_t)jb.nq : 0u;
    if (jb.count) { const uint32_t c = jb.count[0]; nq = c < nq ? c : nq; }
    uint32_t base = 0;                                   // tracks of the queries before this pass (the same in every thread)
    for (uint32_t q0 = 0; q0 < nq; q0 += kTrackThreads) {
        const uint32_t q = q0 + tid;
        const int32_t m = q < nq ? jb.match[q] : -1;
        const bool ok = m >= 0 && m < jobs.map_n;
        // ordered compaction: accepted lanes below this one in the wave (ballot + mbcnt), accepted queries of the waves before it (LDS)
        const uint64_t b = __ballot(ok);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t off = base, total = 0;
        for (uint32_t w = 0; w < kTrackThreads / 64; ++w) {
            const uint32_t c = s_wave[w];
            off += w < wave ? c : 0u;
            total += c;
        }
        __syncthreads();                                 // (s_wave is written again in the next pass)
        const uint32_t i = off + before;
        if (ok && i < (uint32_t)jb.cap) {
            float fx, fy;
            feature_position(jb.kps, jb.feat, jb.feat_stride, q, jobs.scale, &fx, &fy);
            // get_ud_pixel: ima2cam, radius by bisection, cam2ima (ud_pixel.h, shared with pair.hip)
            ud_pixel(fx, fy, UdCamera{ jb.focal, jb.ppx, jb.ppy, jb.k1, jb.k2, jb.k3 }, jb.x + 2 * (size_t)i);
            const double* X = jobs.map_X + 3 * (size_t)m;
            jb.X[3 * (size_t)i] = X[0]; jb.X[3 * (size_t)i + 1] = X[1]; jb.X[3 * (size_t)i + 2] = X[2];
            if (jb.query) jb.query[i] = (int32_t)q;
            if (jb.map) jb.map[i] = m;
            if (jb.h_query) jb.h_query[i] = (int32_t)q;
            if (jb.h_map) jb.h_map[i] = m;
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

} // namespace

hipError_t launch_track_build(TrackJobs& jobs, const int n_jobs, hipStream_t stream)
{
    if (n_jobs < 1 || n_jobs > kMaxBatch) return hipErrorInvalidValue;
    // GPUDetector.hpp:173 through clc_keypoints_to_features: pow(float, integer) evaluated in double, rounded to float -- on the host
    for (int l = 0; l < CLC_MAX_LEVELS; ++l) jobs.scale[l] = (float)std::pow((double)1.2f, (double)l);
    hipLaunchKernelGGL(track_build_kernel, dim3(1, n_jobs), dim3(kTrackThreads), 0, stream, jobs);
    return hipGetLastError();
}

int track_job_inputs(clc_ctx* ctx_map, const clc_track_job& job, TrackJobDev& out, const char* who)
{
    out = TrackJobDev{};
    if (job.nq < 0 || (job.nq > 0 && !job.d_match)) return fail(ctx_map, CLC_ERR_BAD_ARG, who);
    if ((job.d_kps != nullptr) == (job.d_feat != nullptr)) return fail(ctx_map, CLC_ERR_BAD_ARG, "track: exactly one of d_kps / d_feat");
    if (job.d_feat && job.feat_stride < 2) return fail(ctx_map, CLC_ERR_BAD_ARG, "track: feat_stride < 2");
    if (((uintptr_t)job.d_match & 3u) || ((uintptr_t)job.d_kps & 3u) || ((uintptr_t)job.d_feat & 3u) || ((uintptr_t)job.d_count & 3u))
        return fail(ctx_map, CLC_ERR_BAD_ARG, "track: misaligned device pointer");
    if (!(job.cam.focal > 0.0)) return fail(ctx_map, CLC_ERR_BAD_ARG, "track: focal must be positive");
    if (ctx_map->map_X_n < 0) return fail(ctx_map, CLC_ERR_STATE, "track before set_map_points");
    if (ctx_map->map_n >= 0 && ctx_map->map_X_n < ctx_map->map_n)
        return fail(ctx_map, CLC_ERR_STATE, "track: fewer map points (set_map_points) than map descriptors (set_map)");
    out.match = job.d_match; out.count = job.d_count; out.kps = job.d_kps; out.feat = job.d_feat;
    out.nq = job.nq; out.feat_stride = job.feat_stride;
    out.focal = job.cam.focal; out.ppx = job.cam.ppx; out.ppy = job.cam.ppy; out.k1 = job.cam.k1; out.k2 = job.cam.k2; out.k3 = job.cam.k3;
    return CLC_OK;
}

int ensure_track(clc_ctx* ctx, size_t cap)
{
    cap = (cap + 63) & ~(size_t)63;
    if (cap < 64) cap = 64;
    if (cap <= ctx->trk_cap && ctx->d_trk && ctx->h_trk) return CLC_OK;
    // (nothing of an earlier call is in flight: a track solve returns after its staging launch has consumed the block)
    if (ctx->d_trk) { (void)hipFree(ctx->d_trk); ctx->d_trk = nullptr; }
    if (ctx->h_trk) { (void)hipHostFree(ctx->h_trk); ctx->h_trk = nullptr; }
    ctx->trk_cap = 0;
    CLC_HIP(ctx, hipMalloc((void**)&ctx->d_trk, cap * (5 * sizeof(double) + 2 * sizeof(int32_t)) + 64));
    CLC_HIP(ctx, hipHostMalloc((void**)&ctx->h_trk, 64 + cap * 2 * sizeof(int32_t), hipHostMallocDefault));
    memset(ctx->h_trk, 0xFF, 64);
    ctx->trk_cap = cap;
    return CLC_OK;
}

} // namespace clc

using namespace clc;

extern "C" {

int clc_set_map_points(clc_ctx* ctx, const double* h_X, int n)
{
    if (!ctx || n < 0 || (n > 0 && !h_X)) return fail(ctx, CLC_ERR_BAD_ARG, "set_map_points: bad argument");
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) { ctx->map_X_n = -1; return CLC_OK; }
    if (n > ctx->map_X_cap) {
        CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_map_X) { (void)hipFree(ctx->d_map_X); ctx->d_map_X = nullptr; }
        ctx->map_X_cap = 0; ctx->map_X_n = -1;
        CLC_HIP(ctx, hipMalloc((void**)&ctx->d_map_X, (size_t)n * 3 * sizeof(double)));
        ctx->map_X_cap = n;
    }
    ctx->map_X_n = -1;
    CLC_HIP(ctx, hipMemcpyAsync(ctx->d_map_X, h_X, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->map_X_n = n;
    return CLC_OK;
}

int clc_track_build_dev(clc_ctx* ctx, const clc_track_job* job, double* d_X, double* d_x, int32_t* d_query, int32_t* d_map, int32_t* d_n,
                        void* stream)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "track_build: null context / job");
    TrackJobs jobs{};
    const int rc = track_job_inputs(ctx, *job, jobs.j[0], "track_build: bad argument");
    if (rc != CLC_OK) return rc;
    if (job->nq > 0 && (!d_X || !d_x)) return fail(ctx, CLC_ERR_BAD_ARG, "track_build: null output");
    if (((uintptr_t)d_X & 7u) || ((uintptr_t)d_x & 7u) || ((uintptr_t)d_query & 3u) || ((uintptr_t)d_map & 3u) || ((uintptr_t)d_n & 3u))
        return fail(ctx, CLC_ERR_BAD_ARG, "track_build: misaligned device pointer");
    if (job->nq == 0 && !d_n) return CLC_OK;
    jobs.j[0].X = d_X; jobs.j[0].x = d_x; jobs.j[0].query = d_query; jobs.j[0].map = d_map; jobs.j[0].n = d_n;
    jobs.j[0].cap = job->nq;
    jobs.map_X = ctx->d_map_X; jobs.map_n = ctx->map_X_n;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    CLC_HIP(ctx, launch_track_build(jobs, 1, pick(ctx, stream)));
    return CLC_OK;
}

} // extern "C"

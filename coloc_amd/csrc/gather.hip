// gather.hip -- the two gathers that turn a matcher's d_match into the correspondences an a-contrario solve starts from, on the device,
// without the frame or the pair going through the host (pose_batch.hip: clc_track_localize*_dev, clc_pair_filter*_dev):
//   tracks  Localizer::setupTracks (reference include/coloc/Localizer.hpp:59-75): the detector's keypoints (or a block of feature
//           positions) and the map's 3-D points -> undistorted x | X
//   pairs   the gather of RobustMatcher::computeRelativePose (RobustMatcher.hpp:372-424, the loop at :393-398): the two cameras' keypoints
//           (or feature positions) -> undistorted x1 | x2.  The points leave in PIXELS: the 'F' / 'H' conditioning is the staging launch's
//           (acransac.hip: acr_stage_kernel), so the block and its pinned mirrors serve all three models.
// Both are ONE ordered compaction (gather below, over wg_compact.h) that differs only in what an accepted query writes.  gather_rows_kernel:
// rows of a descriptor block picked by an index list (the temporary map's descriptors of the inter-camera step, inter_pose.hip).
//   map pairs  the common features of two maps as 3-D / 3-D pairs X_new | X_old with their common lists, the bounding box of the X_old
//           and the count in one launch (map_update.hip: clc_map_align_sim_dev) -- a third emit, and the one gather that adds something
//           (gather_finish) between its last correspondence and its count.
//
// One launch for a batch of jobs, blockIdx.y = job, ONE workgroup per job: nq <= maxkp is 5-10 k (the solve takes at most 16 384
// correspondences), a few KB in and a few tens of KB out -- the launch is latency-bound, and one workgroup keeps the ordered compaction a
// matter of one ballot per wave and one 16-entry LDS scan per 1 024 queries.  The undistortion's loops are data-dependent and diverge;
// at this size that does not matter.
#include "clc_ctx.h"
#include "ud_pixel.h"
#include "wg_compact.h"

#include <cmath>
#include <cstring>

namespace clc {

namespace {

constexpr int kGatherThreads = 1024;

// get_ud_pixel of row `row` of one 2-D side: the feature position, then ima2cam, radius by bisection, cam2ima (ud_pixel.h)
__device__ __forceinline__ void side_pixel(const GatherSide& s, const uint32_t row, const float* scale, double* out)
{
    float fx, fy;
    feature_position(s.kps, s.feat, s.feat_stride, row, scale, &fx, &fy);
    ud_pixel(fx, fy, s.cam, out);
}

// What differs between the gathers: the train rows a match may name (the same in every thread) and what accepted query q -> train row m
// writes as correspondence i.
__device__ __forceinline__ int32_t train_rows(const TrackJobs& jobs, const TrackJobDev&) { return jobs.map_n; }
__device__ __forceinline__ void emit(const TrackJobs& jobs, const TrackJobDev& jb, const uint32_t q, const int32_t m, const size_t i)
{
    side_pixel(jb.a, q, jobs.scale, jb.x + 2 * i);
    const double* X = jobs.map_X + 3 * (size_t)m;
    jb.X[3 * i] = X[0]; jb.X[3 * i + 1] = X[1]; jb.X[3 * i + 2] = X[2];
    if (jb.query) jb.query[i] = (int32_t)q;
    if (jb.map) jb.map[i] = m;
    if (jb.h_query) jb.h_query[i] = (int32_t)q;
    if (jb.h_map) jb.h_map[i] = m;
}

__device__ __forceinline__ int32_t train_rows(const PairJobs&, const PairJobDev& jb)
{
    int32_t nt = jb.nt > 0 ? jb.nt : 0;
    if (jb.b.count) { const uint32_t c = jb.b.count[0]; nt = c < (uint32_t)nt ? (int32_t)c : nt; }
    return nt;
}
__device__ __forceinline__ void emit(const PairJobs& jobs, const PairJobDev& jb, const uint32_t q, const int32_t m, const size_t i)
{
    double u1[2], u2[2];
    side_pixel(jb.a, q, jobs.scale, u1);
    side_pixel(jb.b, (uint32_t)m, jobs.scale, u2);
    jb.x1[2 * i] = u1[0]; jb.x1[2 * i + 1] = u1[1];
    jb.x2[2 * i] = u2[0]; jb.x2[2 * i + 1] = u2[1];
    if (jb.pair_q) jb.pair_q[i] = (int32_t)q;
    if (jb.pair_t) jb.pair_t[i] = m;
    if (jb.h_q) jb.h_q[i] = (int32_t)q;
    if (jb.h_t) jb.h_t[i] = m;
    if (jb.h_x1) { jb.h_x1[2 * i] = u1[0]; jb.h_x1[2 * i + 1] = u1[1]; }
    if (jb.h_x2) { jb.h_x2[2 * i] = u2[0]; jb.h_x2[2 * i + 1] = u2[1]; }
}

// the common features of two maps: a match names a row of the new map; pair i = the landmark of new row m | the landmark of old row q
__device__ __forceinline__ int32_t train_rows(const MapPairJobs&, const MapPairJobDev& jb) { return jb.n_new > 0 ? jb.n_new : 0; }
__device__ __forceinline__ void emit(const MapPairJobs&, const MapPairJobDev& jb, const uint32_t q, const int32_t m, const size_t i)
{
    const double* xn = jb.new_X + 3 * (size_t)m;
    const double* xo = jb.old_X + 3 * (size_t)q;
    jb.xn[3 * i] = xn[0]; jb.xn[3 * i + 1] = xn[1]; jb.xn[3 * i + 2] = xn[2];
    jb.xo[3 * i] = xo[0]; jb.xo[3 * i + 1] = xo[1]; jb.xo[3 * i + 2] = xo[2];
    jb.cq[i] = (int32_t)q; jb.ct[i] = m;
}

// What a gather adds once its correspondences are written and before the count goes out: nothing for tracks and pairs; the map pairs'
// bounding box of the old points written (minima and maxima: exact whatever the order), into the pinned record
template <class Jobs, class Job> __device__ __forceinline__ void gather_finish(const Jobs&, const Job&, const uint32_t) {}
__device__ __forceinline__ void gather_finish(const MapPairJobs&, const MapPairJobDev& jb, const uint32_t count)
{
    __shared__ double s_box[kGatherThreads / 64][6];
    const uint32_t tid = threadIdx.x, n = count < (uint32_t)jb.cap ? count : (uint32_t)jb.cap;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    double bx[6] = { inf, inf, inf, -inf, -inf, -inf };
    __syncthreads();                                     // the pairs of this workgroup are read back (global memory, one workgroup)
    for (uint32_t i = tid; i < n; i += kGatherThreads)
        for (int c = 0; c < 3; ++c) {
            const double v = jb.xo[3 * (size_t)i + c];
            bx[c] = v < bx[c] ? v : bx[c];
            bx[3 + c] = v > bx[3 + c] ? v : bx[3 + c];
        }
    for (int c = 0; c < 6; ++c)
        for (int d = 32; d > 0; d >>= 1) {
            const double o = __shfl_xor(bx[c], d);
            bx[c] = c < 3 ? (o < bx[c] ? o : bx[c]) : (o > bx[c] ? o : bx[c]);
        }
    if ((tid & 63u) == 0) for (int c = 0; c < 6; ++c) s_box[tid >> 6][c] = bx[c];
    __syncthreads();
    if (tid == 0 && jb.h_box)
        for (int c = 0; c < 6; ++c) {
            double v = s_box[0][c];
            for (int w = 1; w < kGatherThreads / 64; ++w) { const double o = s_box[w][c]; v = c < 3 ? (o < v ? o : v) : (o > v ? o : v); }
            jb.h_box[c] = v;
        }
}

// The gather as an ordered compaction (wg_compact.h, which states the two rules it keeps): correspondence i is the i-th accepted query in
// ascending query order, and the count comes out last, behind a system-scope fence.
template <class Jobs> __device__ __forceinline__ void gather(const Jobs& jobs)
{
    const auto& jb = jobs.j[blockIdx.y];
    __shared__ uint32_t s_wave[kGatherThreads / 64];
    const uint32_t tid = threadIdx.x;
    uint32_t nq = jb.nq > 0 ? (uint32_t)jb.nq : 0u;
    if (jb.a.count) { const uint32_t c = jb.a.count[0]; nq = c < nq ? c : nq; }
    const int32_t nt = train_rows(jobs, jb);
    uint32_t base = 0;                                   // correspondences of the queries before this pass (the same in every thread)
    for (uint32_t q0 = 0; q0 < nq; q0 += kGatherThreads) {
        const uint32_t q = q0 + tid;
        const int32_t m = q < nq ? jb.match[q] : -1;
        const bool ok = m >= 0 && m < nt;
        uint32_t total;
        const uint32_t i = base + ordered_slot<kGatherThreads>(ok, s_wave, &total);
        if (ok && i < (uint32_t)jb.cap) emit(jobs, jb, q, m, (size_t)i);
        base += total;
    }
    gather_finish(jobs, jb, base);
    // the count comes out last: every wave's stores (device blocks and pinned mirrors) are complete and visible system-wide before the
    // word the host polls changes
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        if (jb.n) *jb.n = (int32_t)base;
        if (jb.h_n) __hip_atomic_store(jb.h_n, base, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// two instantiations, two kernels: each carries only its own emit
__global__ __launch_bounds__(kGatherThreads) void track_build_kernel(const TrackJobs jobs) { gather(jobs); }
__global__ __launch_bounds__(kGatherThreads) void pair_build_kernel(const PairJobs jobs) { gather(jobs); }
__global__ __launch_bounds__(kGatherThreads) void map_pair_build_kernel(const MapPairJobs jobs) { gather(jobs); }

// rows idx[0 .. n) of a descriptor block, 16 bytes per thread
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ src, const int32_t* __restrict__ idx, uint4* __restrict__ dst, const uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n * 4u) dst[i] = src[(size_t)(idx ? (uint32_t)idx[i >> 2] : i >> 2) * 4u + (i & 3u)];
}

// the same with a source block per row: row i = row idx[i] of block srcs.src[cam[i]] (the grown map's rows: map_grow.hip)
__global__ __launch_bounds__(256) void gather_rows_multi_kernel(const RowSources srcs, const int32_t* __restrict__ cam, const int32_t* __restrict__ idx,
                                                                uint4* __restrict__ dst, const uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n * 4u) return;
    const int32_t c = cam[i >> 2], r = idx[i >> 2];
    const uint4* src = nullptr;
    for (int k = 0; k < kMaxBatch; ++k) if (k == c) src = srcs.src[k];      // (a select per block: the table stays in registers)
    dst[i] = src && r >= 0 ? src[(size_t)r * 4u + (i & 3u)] : make_uint4(0u, 0u, 0u, 0u);
}

template <class Jobs> hipError_t launch(void (*kernel)(const Jobs), Jobs& jobs, const int n_jobs, hipStream_t stream)
{
    if (n_jobs < 1 || n_jobs > kMaxBatch) return hipErrorInvalidValue;
    level_scales(jobs.scale);
    hipLaunchKernelGGL(kernel, dim3(1, n_jobs), dim3(kGatherThreads), 0, stream, jobs);
    return hipGetLastError();
}

} // namespace

int gather_side(clc_ctx* ctx, const char* who, const uint32_t* count, const clc_keypoint* kps, const float* feat, const int stride,
                const clc_camera_k3& cam, GatherSide& out)
{
    const auto bad = [&](const char* what) { return fail(ctx, CLC_ERR_BAD_ARG, (std::string(who) + what).c_str()); };
    if ((kps != nullptr) == (feat != nullptr)) return bad(": exactly one of d_kps / d_feat per camera");
    if (feat && stride < 2) return bad(": feat_stride < 2");
    if (((uintptr_t)kps & 3u) || ((uintptr_t)feat & 3u) || ((uintptr_t)count & 3u)) return bad(": misaligned device pointer");
    if (!(cam.focal > 0.0)) return bad(": focal must be positive");
    out = GatherSide{ count, kps, feat, stride, UdCamera{ cam.focal, cam.ppx, cam.ppy, cam.k1, cam.k2, cam.k3 } };
    return CLC_OK;
}

hipError_t launch_gather(TrackJobs& jobs, const int n_jobs, hipStream_t stream) { return launch(track_build_kernel, jobs, n_jobs, stream); }
hipError_t launch_gather(PairJobs& jobs, const int n_jobs, hipStream_t stream) { return launch(pair_build_kernel, jobs, n_jobs, stream); }
hipError_t launch_gather(MapPairJobs& jobs, hipStream_t stream)
{
    hipLaunchKernelGGL(map_pair_build_kernel, dim3(1, 1), dim3(kGatherThreads), 0, stream, jobs);
    return hipGetLastError();
}

hipError_t launch_gather_rows(const uint4* src, const int32_t* d_idx, uint4* dst, const uint32_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(((size_t)n * 4 + 255) / 256)), dim3(256), 0, stream, src, d_idx, dst, n);
    return hipGetLastError();
}

hipError_t launch_gather_rows_multi(const RowSources& srcs, const int32_t* d_cam, const int32_t* d_idx, uint4* dst, const uint32_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_rows_multi_kernel, dim3((unsigned)(((size_t)n * 4 + 255) / 256)), dim3(256), 0, stream, srcs, d_cam, d_idx, dst, n);
    return hipGetLastError();
}

int gather_inputs(clc_ctx* ctx_map, const clc_track_job& job, TrackJobDev& out, const char* who)
{
    out = TrackJobDev{};
    if (job.nq < 0 || (job.nq > 0 && !job.d_match)) return fail(ctx_map, CLC_ERR_BAD_ARG, who);
    if ((uintptr_t)job.d_match & 3u) return fail(ctx_map, CLC_ERR_BAD_ARG, "track: misaligned device pointer");
    const int rc = gather_side(ctx_map, "track", job.d_count, job.d_kps, job.d_feat, job.feat_stride, job.cam, out.a);
    if (rc != CLC_OK) return rc;
    out.match = job.d_match; out.nq = job.nq;
    if (ctx_map->map_X_n < 0) return fail(ctx_map, CLC_ERR_STATE, "track before set_map_points");
    if (ctx_map->map_n >= 0 && ctx_map->map_X_n < ctx_map->map_n)
        return fail(ctx_map, CLC_ERR_STATE, "track: fewer map points (set_map_points) than map descriptors (set_map)");
    return CLC_OK;
}

int gather_inputs(clc_ctx* ctx, const clc_pair_job& job, PairJobDev& out, const char* who)
{
    out = PairJobDev{};
    if (job.nq < 0 || job.nt < 0 || (job.nq > 0 && !job.d_match)) return fail(ctx, CLC_ERR_BAD_ARG, who);
    if ((uintptr_t)job.d_match & 3u) return fail(ctx, CLC_ERR_BAD_ARG, "pair: misaligned device pointer");
    int rc = gather_side(ctx, "pair", job.d_count_a, job.d_kps_a, job.d_feat_a, job.feat_stride_a, job.cam_a, out.a);
    if (rc == CLC_OK) rc = gather_side(ctx, "pair", job.d_count_b, job.d_kps_b, job.d_feat_b, job.feat_stride_b, job.cam_b, out.b);
    out.match = job.d_match; out.nq = job.nq; out.nt = job.nt;
    return rc;
}

int ensure_gather(clc_ctx* ctx, GatherBlock& g, size_t cap, const GatherLayout& lay)
{
    cap = up64(cap < 64 ? 64 : cap);
    if (cap <= g.cap && g.d && g.h) return CLC_OK;
    // (no synchronisation: nothing of an earlier call is in flight, a solve returns after its staging launch has consumed the block)
    g.cap = 0;
    GatherView v;
    int rc = carve_block(ctx, g.d, 0, 1, false, "growing a gather block", [&](Carve& c) { v.dev(c, lay, cap); });
    if (rc == CLC_OK) rc = carve_block(ctx, g.h, 0, 1, false, "growing a pinned gather block", [&](Carve& c) { v.pin(c, lay, cap); });
    if (rc != CLC_OK) return rc;
    memset(g.h.ptr, 0xFF, 64);        // the count word: not out yet
    g.cap = cap;
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
    ctx->map_X_n = -1;
    const int rc = grow(ctx, ctx->d_map_X, (size_t)n * 3 * sizeof(double), 0, 1, true, "growing d_map_X");
    if (rc != CLC_OK) return rc;
    CLC_HIP(ctx, hipMemcpyAsync(ctx->d_map_X.ptr, h_X, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->map_X_n = n;
    return CLC_OK;
}

int clc_track_build_dev(clc_ctx* ctx, const clc_track_job* job, double* d_X, double* d_x, int32_t* d_query, int32_t* d_map, int32_t* d_n,
                        void* stream)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "track_build: null context / job");
    TrackJobs jobs{};
    TrackJobDev& jb = jobs.j[0];
    const int rc = gather_inputs(ctx, *job, jb, "track_build: bad argument");
    if (rc != CLC_OK) return rc;
    if (job->nq > 0 && (!d_X || !d_x)) return fail(ctx, CLC_ERR_BAD_ARG, "track_build: null output");
    if (((uintptr_t)d_X & 7u) || ((uintptr_t)d_x & 7u) || ((uintptr_t)d_query & 3u) || ((uintptr_t)d_map & 3u) || ((uintptr_t)d_n & 3u))
        return fail(ctx, CLC_ERR_BAD_ARG, "track_build: misaligned device pointer");
    if (job->nq == 0 && !d_n) return CLC_OK;
    jb.X = d_X; jb.x = d_x; jb.query = d_query; jb.map = d_map; jb.n = d_n;
    jb.cap = job->nq;
    jobs.map_X = ctx->d_map_X.as<double>(); jobs.map_n = ctx->map_X_n;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    CLC_HIP(ctx, launch_gather(jobs, 1, pick(ctx, stream)));
    return CLC_OK;
}

int clc_pair_build_dev(clc_ctx* ctx, const clc_pair_job* job, double* d_x1, double* d_x2, int32_t* d_pair_q, int32_t* d_pair_t, int32_t* d_n,
                       void* stream)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "pair_build: null context / job");
    PairJobs jobs{};
    PairJobDev& jb = jobs.j[0];
    const int rc = gather_inputs(ctx, *job, jb, "pair_build: bad argument");
    if (rc != CLC_OK) return rc;
    if (job->nq > 0 && (!d_x1 || !d_x2)) return fail(ctx, CLC_ERR_BAD_ARG, "pair_build: null output");
    if (((uintptr_t)d_x1 & 7u) || ((uintptr_t)d_x2 & 7u) || ((uintptr_t)d_pair_q & 3u) || ((uintptr_t)d_pair_t & 3u) || ((uintptr_t)d_n & 3u))
        return fail(ctx, CLC_ERR_BAD_ARG, "pair_build: misaligned device pointer");
    if (job->nq == 0 && !d_n) return CLC_OK;
    jb.x1 = d_x1; jb.x2 = d_x2; jb.pair_q = d_pair_q; jb.pair_t = d_pair_t; jb.n = d_n;
    jb.cap = job->nq;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    CLC_HIP(ctx, launch_gather(jobs, 1, pick(ctx, stream)));
    return CLC_OK;
}

} // extern "C"

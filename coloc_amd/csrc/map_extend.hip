// map_extend.hip -- the map extended in place (include/coloc_hip.h: clc_map_extend_dev, clc_map_extend_batch_dev, which state the rule;
// clc_fundamental_from_poses, clc_append_map_points): the untracked matches of two posed views become new rows behind the context's map.
// No counterpart in the reference.  A job is a chain on the context's stream, nothing in it waits for another workgroup:
//   clc_match_guided_dev      k2nn_guided.hip's prep and sweep as they are, under F from the two poses (extend_math.h, on the host), the
//                             list and its distances into the context's scratch
//   extend_mask_kernel        one thread per query: extend_keeps (extend_math.h) -> the masked list, a second array, so the guided list stands
//   unique_enqueue            k2nn_unique.hip's arm, claim and resolve on the masked list
//   extend_point_kernel       one thread per query, 256 a workgroup: an entry of -1 returns at once; otherwise both pixels through
//                             get_ud_pixel (ud_pixel.h), grow_point (map_math.h), X and a flag into the scratch
//   extend_append_kernel      ONE workgroup of 1 024: the ordered compaction (wg_compact.h) over the flags -> rows behind the running row
//                             count, which lives in a device word -- stored by a call's first job from the launch argument, advanced by
//                             every job --: X, A's descriptor row (four uint4 by the accepting thread), the lists, the d_track updates,
//                             the pinned mirrors; { n_added, n_dropped } in ONE pinned word last, behind the system-scope fence and
//                             release store of grow_compact_kernel
// Some thousand queries behind a sweep: short latency-bound launches, nothing here is tuned and nothing is claimed of its speed.
#include "clc_ctx.h"
#include "extend_math.h"
#include "ud_pixel.h"
#include "wg_compact.h"

#include <algorithm>
#include <chrono>
#include <vector>

namespace clc {

namespace {

constexpr int kAppendGroup = 1024;
constexpr int kWide = 256;
constexpr uint32_t kExtendMaxRows = 1u << 22;                        // rows of a view: the guided sweep's and the filter's limit
constexpr unsigned long long kNotYet = ~0ull;

// what the append launch leaves in pinned memory, one per job (64 bytes, ExtendJobPin::rec)
struct ExtendRec {
    unsigned long long word;          // (n_dropped << 32) | n_added, written LAST (system-scope release); kNotYet before
    int32_t n_guided, rows_after;
};
static_assert(sizeof(ExtendRec) <= 64, "ExtendJobPin carves 64 bytes for the record");

struct MaskArgs {
    const int32_t* guided; const uint16_t* best; const int32_t* track_a; const int32_t* track_b;
    int32_t* match;
    uint32_t nq; int32_t nt, max_distance;
};

struct PointArgs {
    const int32_t* match;
    GatherSide a, b;
    float scale[CLC_MAX_LEVELS];
    double cam_a[3], cam_b[3], P_a[12], P_b[12], Rt_a[12], Rt_b[12];
    uint32_t nq; int32_t nt;
    double* X; uint8_t* flag;
};

struct AppendArgs {
    const int32_t* guided; const int32_t* match; const uint8_t* flag; const double* X;      // the job's scratch, nq entries
    const uint4* desc_a;
    uint32_t nq; int32_t nt;
    int32_t arm;                                                     // >= 0: the call's first job stores it as the running row count
    int32_t cap;                                                     // MatcherOptions.maxkp
    int32_t* rows;                                                   // the running row count
    uint4* map_desc; double* map_X;
    int32_t* new_q; int32_t* new_t;                                  // nullable, device
    int32_t* track_a; int32_t* track_b;                              // nullable: update_tracks off, or the view has no list
    double* h_X; int32_t* h_q; int32_t* h_t;                         // pinned mirrors
    ExtendRec* rec;
};

__global__ __launch_bounds__(kWide) void extend_mask_kernel(const MaskArgs a)
{
    const uint32_t q = blockIdx.x * kWide + threadIdx.x;
    if (q >= a.nq) return;
    const int32_t t = a.guided[q];
    int32_t out = -1;
    if (t >= 0 && t < a.nt) {
        const int32_t ta = a.track_a ? a.track_a[q] : -1, tb = a.track_b ? a.track_b[t] : -1;
        if (extend_keeps(ta, tb, a.best[q], a.max_distance)) out = t;
    }
    a.match[q] = out;
}

__device__ __forceinline__ void view_pixel(const GatherSide& side, const uint32_t row, const float* scale, double* out)
{
    float fx, fy;
    feature_position(side.kps, side.feat, side.feat_stride, row, scale, &fx, &fy);
    ud_pixel(fx, fy, side.cam, out);
}

__global__ __launch_bounds__(kWide) void extend_point_kernel(const PointArgs a)
{
    const uint32_t q = blockIdx.x * kWide + threadIdx.x;
    if (q >= a.nq) return;
    const int32_t t = a.match[q];
    if (t < 0 || t >= a.nt) return;
    double xa[2], xb[2], X[3] = { 0.0, 0.0, 0.0 };
    view_pixel(a.a, q, a.scale, xa);
    view_pixel(a.b, (uint32_t)t, a.scale, xb);
    const bool ok = grow_point(a.cam_a, a.cam_b, a.P_a, a.P_b, a.Rt_a, a.Rt_b, xa, xb, X);
    a.X[3 * (size_t)q] = X[0]; a.X[3 * (size_t)q + 1] = X[1]; a.X[3 * (size_t)q + 2] = X[2];
    a.flag[q] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kAppendGroup) void extend_append_kernel(const AppendArgs a)
{
    __shared__ uint32_t s_wave[kAppendGroup / 64];
    __shared__ uint32_t s_guided;
    if (threadIdx.x == 0) s_guided = 0u;
    const int32_t before = a.arm >= 0 ? a.arm : a.rows[0];           // read by every thread ahead of the barriers below; stored behind them
    const uint32_t room = before < a.cap ? (uint32_t)(a.cap - before) : 0u;
    uint32_t base = 0, guided = 0;
    for (uint32_t q0 = 0; q0 < a.nq; q0 += kAppendGroup) {
        const uint32_t q = q0 + threadIdx.x;
        const int32_t t = q < a.nq ? a.match[q] : -1;
        const bool ok = t >= 0 && t < a.nt && a.flag[q] != 0;
        if (q < a.nq && a.guided[q] >= 0) ++guided;
        uint32_t total;
        const uint32_t k = base + ordered_slot<kAppendGroup>(ok, s_wave, &total);
        if (ok && k < room) {
            const size_t row = (size_t)before + k;
            const double X0 = a.X[3 * (size_t)q], X1 = a.X[3 * (size_t)q + 1], X2 = a.X[3 * (size_t)q + 2];
            a.map_X[3 * row] = X0; a.map_X[3 * row + 1] = X1; a.map_X[3 * row + 2] = X2;
            const uint4* src = a.desc_a + 4 * (size_t)q;
            uint4* dst = a.map_desc + 4 * row;
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
            if (a.new_q) a.new_q[k] = (int32_t)q;
            if (a.new_t) a.new_t[k] = t;
            if (a.track_a) a.track_a[q] = (int32_t)row;
            if (a.track_b) a.track_b[t] = (int32_t)row;
            a.h_X[3 * (size_t)k] = X0; a.h_X[3 * (size_t)k + 1] = X1; a.h_X[3 * (size_t)k + 2] = X2;
            a.h_q[k] = (int32_t)q; a.h_t[k] = t;
        }
        base += total;
    }
    if (guided) atomicAdd(&s_guided, guided);                        // (nq == 0 runs no pass: s_guided is read behind the barrier below)
    // the counts come out last: the rows, the lists and the mirrors are complete and visible system-wide before the word the host polls changes
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t added = base < room ? base : room;
        a.rows[0] = before + (int32_t)added;
        a.rec->n_guided = (int32_t)s_guided;
        a.rec->rows_after = before + (int32_t)added;
        __hip_atomic_store(&a.rec->word, ((unsigned long long)(base - added) << 32) | added, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

inline dim3 wide_grid(const uint32_t n) { return dim3((n + kWide - 1u) / kWide); }

// the context's map points with room for `rows` rows, the first `keep` kept: DevBuf::grow would not keep them
int points_room(clc_ctx* ctx, const size_t rows, const size_t keep, const char* what)
{
    const size_t need = rows * 3 * sizeof(double);
    if (need <= ctx->d_map_X.bytes) return CLC_OK;
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    DevBuf grown;
    const hipError_t e = grown.alloc(need);
    if (e != hipSuccess) return fail(ctx, CLC_ERR_HIP, what, e);
    if (keep > 0) {
        CLC_HIP(ctx, hipMemcpyAsync(grown.ptr, ctx->d_map_X.ptr, keep * 3 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    std::swap(ctx->d_map_X, grown);
    return CLC_OK;
}

// one view's arguments, checked; its 2-D side into `side`
int view_inputs(clc_ctx* ctx, const clc_extend_view& v, GatherSide& side)
{
    const auto bad = [&](const char* what) { return fail(ctx, CLC_ERR_BAD_ARG, what); };
    if (v.n < 0 || (v.n > 0 && !v.d_desc)) return bad("map_extend: negative count / null descriptor block");
    if ((uintptr_t)v.d_desc & 15u) return bad("map_extend: descriptor rows must be 16-byte aligned");
    if ((uintptr_t)v.d_track & 3u) return bad("map_extend: misaligned device pointer");
    for (int i = 0; i < 12; ++i) if (!std::isfinite(v.Rt[i])) return bad("map_extend: Rt is not finite");
    return gather_side(ctx, "map_extend", v.d_count, v.d_kps, v.d_feat, v.feat_stride, v.cam, side);
}

void outputs_none(clc_map_extend& job, const int map_n)
{
    for (int i = 0; i < 9; ++i) job.F[i] = 0.0;
    job.map_n_before = map_n; job.n_guided = 0; job.n_added = 0; job.n_dropped = 0; job.status = CLC_OK;
}

int extend_batch(clc_ctx* ctx, clc_map_extend* jobs, const int n_jobs)
{
    if (!ctx || n_jobs < 0 || n_jobs > CLC_MAX_TRACK_PAIRS || (n_jobs > 0 && !jobs))
        return fail(ctx, CLC_ERR_BAD_ARG, "map_extend: null context / jobs, or a job count outside 0 .. CLC_MAX_TRACK_PAIRS");
    for (int j = 0; j < n_jobs; ++j) outputs_none(jobs[j], ctx->map_n);
    const auto refuse = [&](const int j, const int rc) { if (j >= 0) jobs[j].status = rc; return rc; };
    if (!ctx->has_mat) return refuse(n_jobs - 1, fail(ctx, CLC_ERR_STATE, "map_extend: context created without matcher options"));
    // everything is checked before anything is enqueued
    std::vector<GatherSide> side_a((size_t)n_jobs), side_b((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const clc_map_extend& jb = jobs[j];
        int rc = view_inputs(ctx, jb.a, side_a[(size_t)j]);
        if (rc == CLC_OK) rc = view_inputs(ctx, jb.b, side_b[(size_t)j]);
        if (rc == CLC_OK && (!(jb.band > 0.f) || !std::isfinite(jb.band))) rc = fail(ctx, CLC_ERR_BAD_ARG, "map_extend: band must be finite and positive");
        if (rc == CLC_OK && (jb.max_distance < 0 || jb.max_distance > kExtendMaxDistance))
            rc = fail(ctx, CLC_ERR_BAD_ARG, "map_extend: max_distance outside 0 .. 512");
        if (rc == CLC_OK && (((uintptr_t)jb.d_new_q & 3u) || ((uintptr_t)jb.d_new_t & 3u))) rc = fail(ctx, CLC_ERR_BAD_ARG, "map_extend: misaligned device pointer");
        if (rc != CLC_OK) return refuse(j, rc);
    }
    // the partially-owned state clc_track_localize_dev refuses; a map of 0 rows with its points cleared is an empty map
    if (ctx->map_n < 0) return refuse(n_jobs - 1, fail(ctx, CLC_ERR_STATE, "map_extend before set_map"));
    if (ctx->map_n > 0 ? ctx->map_X_n != ctx->map_n : ctx->map_X_n > 0)
        return refuse(n_jobs - 1, fail(ctx, CLC_ERR_STATE, "map_extend: the map's points (set_map_points) are not its descriptor rows (set_map)"));
    for (int j = 0; j < n_jobs; ++j)
        if ((uint32_t)jobs[j].a.n > kExtendMaxRows || (uint32_t)jobs[j].b.n > kExtendMaxRows)
            return refuse(j, fail(ctx, CLC_ERR_CAPACITY, "map_extend: more than 2^22 rows in a view"));
    std::vector<int> live;                                                   // a job without query rows adds nothing
    for (int j = 0; j < n_jobs; ++j) {
        const clc_camera_k3 &ca = jobs[j].a.cam, &cb = jobs[j].b.cam;
        const double cam_a[3] = { ca.focal, ca.ppx, ca.ppy }, cam_b[3] = { cb.focal, cb.ppx, cb.ppy };
        fundamental_from_poses(cam_a, jobs[j].a.Rt, cam_b, jobs[j].b.Rt, jobs[j].F);
        if (jobs[j].a.n > 0) live.push_back(j);
    }
    if (live.empty()) return CLC_OK;
    const int n = (int)live.size();
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int cap = (int)ctx->mopts.maxkp;

    int rc = points_room(ctx, (size_t)cap, (size_t)ctx->map_n, "map_extend: growing d_map_X");
    ExtendDev head;
    std::vector<ExtendJobDev> dv((size_t)n);
    std::vector<ExtendJobPin> pv((size_t)n);
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->d_extend, 1, 4, true, "growing d_extend", [&](Carve& c) {
        head.carve(c);
        for (int k = 0; k < n; ++k) dv[(size_t)k].carve(c, (size_t)jobs[live[(size_t)k]].a.n);
    });
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->h_extend, 1, 4, true, "growing h_extend", [&](Carve& c) {
        for (int k = 0; k < n; ++k) pv[(size_t)k].carve(c, (size_t)jobs[live[(size_t)k]].a.n);
    });
    if (rc != CLC_OK) return refuse(live[0], rc);
    for (int k = 0; k < n; ++k) __atomic_store_n(&((ExtendRec*)pv[(size_t)k].rec)->word, kNotYet, __ATOMIC_RELAXED);

    // behind whatever produced the inputs: an event on the producer's stream, no host synchronisation
    for (int k = 0; k < n; ++k) {
        hipStream_t prod = (hipStream_t)jobs[live[(size_t)k]].after_stream;
        if (prod && prod != st) CLC_HIP(ctx, order_behind(ctx->ev_track, prod, &st, 1));
    }
    for (int k = 0; k < n; ++k) {
        clc_map_extend& jb = jobs[live[(size_t)k]];
        const GatherSide &sa = side_a[(size_t)live[(size_t)k]], &sb = side_b[(size_t)live[(size_t)k]];
        const ExtendJobDev& d = dv[(size_t)k];
        const ExtendJobPin& p = pv[(size_t)k];
        // 2: the guided match as it stands
        clc_guided_job gj{};
        gj.d_q = jb.a.d_desc; gj.nq = jb.a.n; gj.d_t = jb.b.d_desc; gj.nt = jb.b.n;
        gj.d_count_a = jb.a.d_count; gj.d_count_b = jb.b.d_count;
        gj.d_kps_a = jb.a.d_kps; gj.d_feat_a = jb.a.d_feat; gj.feat_stride_a = jb.a.feat_stride;
        gj.d_kps_b = jb.b.d_kps; gj.d_feat_b = jb.b.d_feat; gj.feat_stride_b = jb.b.feat_stride;
        gj.cam_a = jb.a.cam; gj.cam_b = jb.b.cam;
        memcpy(gj.F, jb.F, sizeof gj.F);
        gj.band = jb.band; gj.threshold = jb.threshold;
        gj.d_match = d.guided; gj.d_best = d.best;
        rc = clc_match_guided_dev(ctx, &gj, st);
        if (rc != CLC_OK) return refuse(live[(size_t)k], rc);
        // 3: the mask
        MaskArgs m{};
        m.guided = d.guided; m.best = d.best; m.track_a = jb.a.d_track; m.track_b = jb.b.d_track; m.match = d.match;
        m.nq = (uint32_t)jb.a.n; m.nt = jb.b.n; m.max_distance = jb.max_distance;
        hipLaunchKernelGGL(extend_mask_kernel, wide_grid(m.nq), dim3(kWide), 0, st, m);
        CLC_HIP(ctx, hipGetLastError());
        // 4: one-to-one
        clc_unique_job uj{};
        uj.d_match = d.match; uj.d_best = d.best; uj.nq = jb.a.n; uj.nt = jb.b.n;
        UniqueDev ud;
        rc = unique_scratch(ctx, uj.nq, uj.nt, false, false, ud);
        if (rc == CLC_OK) rc = unique_enqueue(ctx, &uj, &ud, 1, st);
        if (rc != CLC_OK) return refuse(live[(size_t)k], rc);
        // 5: the points
        PointArgs pa{};
        pa.match = d.match; pa.a = sa; pa.b = sb;
        level_scales(pa.scale);
        pa.cam_a[0] = sa.cam.focal; pa.cam_a[1] = sa.cam.ppx; pa.cam_a[2] = sa.cam.ppy;
        pa.cam_b[0] = sb.cam.focal; pa.cam_b[1] = sb.cam.ppx; pa.cam_b[2] = sb.cam.ppy;
        memcpy(pa.Rt_a, jb.a.Rt, sizeof pa.Rt_a); memcpy(pa.Rt_b, jb.b.Rt, sizeof pa.Rt_b);
        projective_equivalent(sa.cam.focal, sa.cam.ppx, sa.cam.ppy, pa.Rt_a, pa.P_a);
        projective_equivalent(sb.cam.focal, sb.cam.ppx, sb.cam.ppy, pa.Rt_b, pa.P_b);
        pa.nq = (uint32_t)jb.a.n; pa.nt = jb.b.n; pa.X = d.X; pa.flag = d.flag;
        hipLaunchKernelGGL(extend_point_kernel, wide_grid(pa.nq), dim3(kWide), 0, st, pa);
        CLC_HIP(ctx, hipGetLastError());
        // 6: the append
        AppendArgs ap{};
        ap.guided = d.guided; ap.match = d.match; ap.flag = d.flag; ap.X = d.X;
        ap.desc_a = (const uint4*)jb.a.d_desc;
        ap.nq = (uint32_t)jb.a.n; ap.nt = jb.b.n;
        ap.arm = k == 0 ? ctx->map_n : -1;
        ap.cap = cap; ap.rows = head.rows;
        ap.map_desc = ctx->d_m.as<uint4>(); ap.map_X = ctx->d_map_X.as<double>();
        ap.new_q = jb.d_new_q; ap.new_t = jb.d_new_t;
        ap.track_a = jb.update_tracks ? jb.a.d_track : nullptr; ap.track_b = jb.update_tracks ? jb.b.d_track : nullptr;
        ap.h_X = p.X; ap.h_q = p.q; ap.h_t = p.t; ap.rec = (ExtendRec*)p.rec;
        hipLaunchKernelGGL(extend_append_kernel, dim3(1), dim3(kAppendGroup), 0, st, ap);
        CLC_HIP(ctx, hipGetLastError());
    }
    // ONE wait: the last job's word.  The jobs ran in order on one stream, each behind its own system-scope fence.
    const ExtendRec* last = (const ExtendRec*)pv[(size_t)(n - 1)].rec;
    rc = wait_pinned(ctx, &last->word, kNotYet, st, std::chrono::steady_clock::now(), 2, "map_extend: the append launch left no count");
    if (rc != CLC_OK) return refuse(live[(size_t)(n - 1)], rc);
    int rows = ctx->map_n, at = 0;
    for (int j = 0; j < n_jobs; ++j) {
        clc_map_extend& jb = jobs[j];
        jb.map_n_before = rows;
        if (at >= n || live[(size_t)at] != j) continue;
        const ExtendJobPin& p = pv[(size_t)at++];
        const ExtendRec* rec = (const ExtendRec*)p.rec;
        const unsigned long long w = __atomic_load_n(&rec->word, __ATOMIC_ACQUIRE);
        if (w == kNotYet) return refuse(j, fail(ctx, CLC_ERR_HIP, "map_extend: a job of the batch left no count"));
        jb.n_added = (int)(uint32_t)w; jb.n_dropped = (int)(uint32_t)(w >> 32); jb.n_guided = rec->n_guided;
        const size_t na = (size_t)jb.n_added;
        if (jb.new_q && na) memcpy(jb.new_q, p.q, na * sizeof(int32_t));
        if (jb.new_t && na) memcpy(jb.new_t, p.t, na * sizeof(int32_t));
        if (jb.X && na) memcpy(jb.X, p.X, 3 * na * sizeof(double));
        rows += jb.n_added;
    }
    if (rows > ctx->map_n) { ctx->map_n = rows; ctx->map_X_n = rows; }
    return CLC_OK;
}

} // namespace

} // namespace clc

using namespace clc;

extern "C" {

int clc_map_extend_dev(clc_ctx* ctx, clc_map_extend* job)
{
    if (!job) return fail(ctx, CLC_ERR_BAD_ARG, "map_extend: null job");
    return extend_batch(ctx, job, 1);
}

int clc_map_extend_batch_dev(clc_ctx* ctx, clc_map_extend* jobs, int n_jobs) { return extend_batch(ctx, jobs, n_jobs); }

int clc_fundamental_from_poses(const clc_camera_k3* cam_a, const double* Rt_a, const clc_camera_k3* cam_b, const double* Rt_b, double* F)
{
    if (!cam_a || !Rt_a || !cam_b || !Rt_b || !F || !(cam_a->focal > 0.0) || !(cam_b->focal > 0.0)) return CLC_ERR_BAD_ARG;
    const double a[3] = { cam_a->focal, cam_a->ppx, cam_a->ppy }, b[3] = { cam_b->focal, cam_b->ppx, cam_b->ppy };
    fundamental_from_poses(a, Rt_a, b, Rt_b, F);
    return CLC_OK;
}

int clc_append_map_points(clc_ctx* ctx, const double* h_X, int n)
{
    if (!ctx || n < 0 || (n > 0 && !h_X)) return fail(ctx, CLC_ERR_BAD_ARG, "append_map_points: bad argument");
    if (ctx->map_n >= 0) return fail(ctx, CLC_ERR_STATE, "append_map_points: the context holds map rows (clc_map_extend_dev extends rows and points together)");
    if (n == 0) return CLC_OK;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t have = ctx->map_X_n > 0 ? (size_t)ctx->map_X_n : 0, rows = have + (size_t)n;
    if (rows > (size_t)0x7FFFFFFF) return fail(ctx, CLC_ERR_CAPACITY, "append_map_points: more than 2^31 - 1 points");
    // half as much again where the block has to move: a map that grows a few rows per frame must not be copied at every frame
    const int rc = points_room(ctx, rows * 3 * sizeof(double) <= ctx->d_map_X.bytes ? rows : rows + rows / 2, have, "append_map_points: growing d_map_X");
    if (rc != CLC_OK) return rc;
    CLC_HIP(ctx, hipMemcpyAsync(ctx->d_map_X.as<double>() + 3 * have, h_X, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->map_X_n = (int)rows;
    return CLC_OK;
}

} // extern "C"

// map_cull.hip -- the map's observation statistics and the cull (include/coloc_hip.h: clc_map_observe_dev, clc_map_observe_batch_dev,
// clc_map_cull_dev, which state the rule; clc_map_stats_get, clc_cull_map_points, clc_map_cull_rule_default).  No counterpart in the
// reference.  Everything runs on the context's stream and nothing in it waits for another workgroup:
//   cull_cover_kernel      rows [stat_rows, map_n) -- what clc_map_extend_dev appended -- get visible = found = 0, last_view = epoch
//   observe_hit_kernel     one thread per (keypoint, view): the keypoint through get_ud_pixel (ud_pixel.h), the row d_track names through
//                          proj_point (proj_math.h), proj_in_radius -> the call's serial into the row's stamp word of the view
//   observe_update_kernel  one thread per (map row, view): proj_point, cull_in_view (cull_math.h), the three counters -- 32-bit integer
//                          adds, which commute, so a batch is ONE pair of launches with the view in blockIdx.y
//   cull_scan_kernel       ONE workgroup of 1 024: cull_clause per row and the ordered compaction (wg_compact.h) -> the remap in the
//                          context's scratch, the caller's d_remap and the pinned mirror; the kept count and the clause counts in a device record
//   cull_move_kernel       four lanes per OLD row: one uint4 of the descriptor each, the point and the counters by lanes 0 - 2, into the
//                          context's OTHER buffers -- row remap[r] < r of one workgroup is row r' of another, so never in place
//   cull_lists_kernel      the caller's track lists through the remap, in place, the list in blockIdx.y
//   cull_publish_kernel    one thread: the clause counts, then { n_kept, n_dropped } in ONE pinned word last, behind the system-scope fence
//                          and release store of the other compaction kernels
// The host waits for that word once per cull and installs by buffer swaps, as map_update.hip installs.  An observe call waits for nothing.
// Some thousand rows and keypoints: short latency-bound launches, nothing here is tuned and nothing is claimed of its speed.
#include "clc_ctx.h"
#include "cull_math.h"
#include "ud_pixel.h"
#include "wg_compact.h"

#include <algorithm>
#include <chrono>
#include <vector>

namespace clc {

namespace {

constexpr int kCullGroup = 1024;
constexpr int kWide = 256;
constexpr unsigned long long kNotYet = ~0ull;

// what the publish launch leaves in pinned memory (64 bytes, CullPin::rec)
struct CullRec {
    unsigned long long word;          // (n_dropped << 32) | n_kept, written LAST (system-scope release); kNotYet before
    uint32_t n_flagged, n_ratio, n_idle;
};
static_assert(sizeof(CullRec) <= 64, "CullPin carves 64 bytes for the record");

struct ObserveView {
    GatherSide side;
    double Rt[12];
    const int32_t* track; int32_t* counts;                           // nullable both
    uint32_t n;
    float lo, hi_x, hi_y, r2;                                        // cull_bounds and gate * gate, formed once on the host
};
struct ObserveArgs {
    ObserveView v[kMaxBatch];
    float scale[CLC_MAX_LEVELS];
    const double* map_X; uint32_t nm;
    uint32_t serial, epoch;
    uint32_t* hit; size_t stride;                                    // the stamp words: view v, row r at hit[v * stride + r]
    CullStat stat;
};
static_assert(sizeof(ObserveArgs) <= 4096, "ObserveArgs is passed as a kernel argument: a batch of CLC_MAX_BATCH views is ONE pair of launches");

struct ScanArgs {
    CullStat stat; const uint8_t* flagged;
    uint32_t n, epoch, min_visible, num, den, max_idle;
    int32_t* remap; int32_t* d_remap; int32_t* h_remap;              // the scratch; the caller's (nullable); the pinned mirror
    uint32_t* rec;                                                   // { n_kept, flagged, ratio, idle }
};
struct MoveArgs {
    const int32_t* remap; uint32_t n;
    const uint4* desc; uint4* desc_out;                              // nullable pair: a context that holds only points
    const double* X; double* X_out;
    CullStat stat, stat_out;                                         // null arrays: no counters to move
};
struct ListArgs {
    int32_t* list[kMaxBatch]; uint32_t n[kMaxBatch];
    const int32_t* remap; int32_t n_before;
};

__global__ __launch_bounds__(kWide) void cull_cover_kernel(const CullStat s, const uint32_t from, const uint32_t to, const uint32_t epoch)
{
    const uint32_t r = from + blockIdx.x * kWide + threadIdx.x;
    if (r >= to) return;
    s.visible[r] = 0u; s.found[r] = 0u; s.last_view[r] = epoch;
}

__global__ __launch_bounds__(kWide) void observe_hit_kernel(const ObserveArgs a)
{
    const ObserveView& v = a.v[blockIdx.y];
    const uint32_t q = blockIdx.x * kWide + threadIdx.x;
    if (q == 0 && v.counts) { v.counts[0] = 0; v.counts[1] = 0; }     // (the update launch adds to them)
    if (!v.track) return;
    uint32_t n = v.n;
    if (v.side.count) { const uint32_t c = v.side.count[0]; n = c < n ? c : n; }
    if (q >= n) return;
    const int32_t r = v.track[q];
    if (r < 0 || (uint32_t)r >= a.nm) return;                        // names no row
    float fx, fy, p[2];
    double u[2];
    feature_position(v.side.kps, v.side.feat, v.side.feat_stride, q, a.scale, &fx, &fy);
    ud_pixel(fx, fy, v.side.cam, u);
    const ProjCamera cam{ v.side.cam.focal, v.side.cam.ppx, v.side.cam.ppy };
    proj_point(v.Rt, cam, a.map_X + 3u * (size_t)r, p);
    if (proj_in_radius((float)u[0], (float)u[1], p[0], p[1], v.r2)) a.hit[blockIdx.y * a.stride + (uint32_t)r] = a.serial;
}

__global__ __launch_bounds__(kWide) void observe_update_kernel(const ObserveArgs a)
{
    __shared__ uint32_t s_cnt[2];
    const ObserveView& v = a.v[blockIdx.y];
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t r = blockIdx.x * kWide + threadIdx.x;
    bool in = false, hit = false;
    if (r < a.nm) {
        float p[2];
        const ProjCamera cam{ v.side.cam.focal, v.side.cam.ppx, v.side.cam.ppy };
        proj_point(v.Rt, cam, a.map_X + 3u * (size_t)r, p);
        in = cull_in_view(p[0], p[1], v.lo, v.hi_x, v.hi_y);
        if (in) {
            hit = a.hit[blockIdx.y * a.stride + r] == a.serial;
            atomicAdd(&a.stat.visible[r], 1u);
            if (hit) atomicAdd(&a.stat.found[r], 1u);
            a.stat.last_view[r] = a.epoch;                           // (every view of the batch stores the same word)
        }
    }
    if (v.counts) {                                                  // (uniform over the workgroup)
        const uint32_t n_in = (uint32_t)__popcll(__ballot(in)), n_hit = (uint32_t)__popcll(__ballot(hit));
        if ((threadIdx.x & 63u) == 0) { atomicAdd(&s_cnt[0], n_in); atomicAdd(&s_cnt[1], n_hit); }
        __syncthreads();
        if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&v.counts[threadIdx.x], (int32_t)s_cnt[threadIdx.x]);
    }
}

__global__ __launch_bounds__(kCullGroup) void cull_scan_kernel(const ScanArgs a)
{
    __shared__ uint32_t s_wave[kCullGroup / 64];
    __shared__ uint32_t s_clause[4];
    if (threadIdx.x < 4) s_clause[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t base = 0, mine[4] = { 0u, 0u, 0u, 0u };
    for (uint32_t r0 = 0; r0 < a.n; r0 += kCullGroup) {
        const uint32_t r = r0 + threadIdx.x;
        int clause = -1;                                             // (no row)
        if (r < a.n)
            clause = cull_clause(a.stat.visible[r], a.stat.found[r], a.stat.last_view[r], a.epoch, a.flagged && a.flagged[r] != 0, a.min_visible,
                                 a.num, a.den, a.max_idle);
        const bool keep = clause == kCullKept;
        uint32_t total;
        const uint32_t k = base + ordered_slot<kCullGroup>(keep, s_wave, &total);
        if (r < a.n) {
            const int32_t m = keep ? (int32_t)k : -1;
            a.remap[r] = m; a.h_remap[r] = m;
            if (a.d_remap) a.d_remap[r] = m;
            ++mine[clause];
        }
        base += total;
    }
    for (int c = 1; c < 4; ++c) if (mine[c]) atomicAdd(&s_clause[c], mine[c]);
    __threadfence_system();                                          // (the pinned mirror)
    __syncthreads();
    if (threadIdx.x == 0) { a.rec[0] = base; a.rec[1] = s_clause[1]; a.rec[2] = s_clause[2]; a.rec[3] = s_clause[3]; }
}

__global__ __launch_bounds__(kWide) void cull_move_kernel(const MoveArgs a)
{
    const uint32_t i = blockIdx.x * kWide + threadIdx.x, r = i >> 2, k = i & 3u;
    if (r >= a.n) return;
    const int32_t m = a.remap[r];
    if (m < 0 || (uint32_t)m > r) return;                            // (a kept row never moves up)
    if (a.desc) a.desc_out[4u * (size_t)m + k] = a.desc[4u * (size_t)r + k];
    if (k < 3u) {
        a.X_out[3u * (size_t)m + k] = a.X[3u * (size_t)r + k];
        if (a.stat.visible) {
            const uint32_t* src = k == 0u ? a.stat.visible : k == 1u ? a.stat.found : a.stat.last_view;
            uint32_t* dst = k == 0u ? a.stat_out.visible : k == 1u ? a.stat_out.found : a.stat_out.last_view;
            dst[m] = src[r];
        }
    }
}

__global__ __launch_bounds__(kWide) void cull_lists_kernel(const ListArgs a)
{
    const uint32_t i = blockIdx.x * kWide + threadIdx.x;
    if (i >= a.n[blockIdx.y]) return;
    int32_t* e = a.list[blockIdx.y] + i;
    *e = cull_remap_entry(*e, a.n_before, a.remap);
}

__global__ void cull_publish_kernel(const uint32_t* rec, const uint32_t n_before, CullRec* out)
{
    const uint32_t kept = rec[0];
    out->n_flagged = rec[1]; out->n_ratio = rec[2]; out->n_idle = rec[3];
    // the counts come out last: the rows, the lists and the mirror are complete (the launches before this one) and visible system-wide
    __threadfence_system();
    __hip_atomic_store(&out->word, ((unsigned long long)(n_before - kept) << 32) | kept, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

inline dim3 wide_grid(const uint32_t n, const unsigned y = 1) { return dim3(std::max((n + kWide - 1u) / kWide, 1u), y); }

// the state every entry here asks of the context (CLC_ERR_STATE): matcher options, a map, its points exactly its rows
int cull_state(clc_ctx* ctx, const char* who)
{
    const auto no = [&](const char* what) { return fail(ctx, CLC_ERR_STATE, (std::string(who) + what).c_str()); };
    if (!ctx->has_mat) return no(": context created without matcher options");
    if (ctx->map_n < 0) return no(" before set_map");
    if (ctx->map_n > 0 ? ctx->map_X_n != ctx->map_n : ctx->map_X_n > 0) return no(": the map's points (set_map_points) are not its descriptor rows (set_map)");
    return CLC_OK;
}

// COVER: the counters' block is there (room for MatcherOptions.maxkp rows, made once) and covers the map's rows
int cover_rows(clc_ctx* ctx, CullStat& stat)
{
    const size_t cap = ctx->has_mat ? (size_t)ctx->mopts.maxkp : 0;
    const int n = ctx->map_n > 0 ? ctx->map_n : 0;
    if ((size_t)n > cap) return fail(ctx, CLC_ERR_CAPACITY, "map statistics: more map rows than MatcherOptions.maxkp");
    const int rc = carve_block(ctx, ctx->d_stat, 0, 1, true, "allocating the map statistics", [&](Carve& c) { stat.carve(c, cap); });
    if (rc != CLC_OK) return rc;
    if (ctx->stat_rows > n) ctx->stat_rows = n;
    if (ctx->stat_rows < n) {
        hipLaunchKernelGGL(cull_cover_kernel, wide_grid((uint32_t)(n - ctx->stat_rows)), dim3(kWide), 0, ctx->stream, stat, (uint32_t)ctx->stat_rows,
                           (uint32_t)n, ctx->epoch);
        CLC_HIP(ctx, hipGetLastError());
        ctx->stat_rows = n;
    }
    return CLC_OK;
}

// room for `bytes` in the next map's points, at least as much as the installed block has (an extension behind the swap must not copy)
int next_points(clc_ctx* ctx, const size_t rows)
{
    const size_t need = std::max(ctx->d_map_X.bytes, rows * 3 * sizeof(double) + 64);
    return grow(ctx, ctx->d_map_X_next, need, 0, 1, true, "growing the next map's points");
}

void observe_outputs_none(clc_ctx* ctx, clc_map_observe& job)
{
    job.epoch = ctx ? ctx->epoch : 0u; job.map_n = ctx ? ctx->map_n : -1; job.status = CLC_OK;
}

int observe_batch(clc_ctx* ctx, clc_map_observe* jobs, const int n_views)
{
    if (!ctx || n_views < 0 || n_views > kMaxBatch || (n_views > 0 && !jobs))
        return fail(ctx, CLC_ERR_BAD_ARG, "map_observe: null context / jobs, or a view count outside 0 .. CLC_MAX_BATCH");
    for (int j = 0; j < n_views; ++j) observe_outputs_none(ctx, jobs[j]);
    const auto refuse = [&](const int j, const int rc) { if (j >= 0) jobs[j].status = rc; return rc; };
    // everything is checked before anything is enqueued
    ObserveArgs a{};
    uint32_t max_n = 0;
    for (int j = 0; j < n_views; ++j) {
        const clc_map_observe& jb = jobs[j];
        const clc_observe_view& v = jb.view;
        const auto bad = [&](const char* what) { return refuse(j, fail(ctx, CLC_ERR_BAD_ARG, what)); };
        if (v.n < 0) return bad("map_observe: negative count");
        if (((uintptr_t)v.d_track & 3u) || ((uintptr_t)v.d_counts & 3u)) return bad("map_observe: misaligned device pointer");
        if (jb.width <= 0 || jb.height <= 0) return bad("map_observe: width and height must be positive");
        const float r2 = jb.gate * jb.gate;                                             // the gate's limit, formed once, in float
        if (!(jb.gate >= 0.f) || !std::isfinite(jb.gate) || !std::isfinite(r2)) return bad("map_observe: gate and its square must be finite and not negative");
        if (!(jb.margin >= 0.f) || !std::isfinite(jb.margin)) return bad("map_observe: margin must be finite and not negative");
        for (int i = 0; i < 12; ++i) if (!std::isfinite(v.Rt[i])) return bad("map_observe: Rt is not finite");
        ObserveView& o = a.v[j];
        const int rc = gather_side(ctx, "map_observe", v.d_count, v.d_kps, v.d_feat, v.feat_stride, v.cam, o.side);
        if (rc != CLC_OK) return refuse(j, rc);
        memcpy(o.Rt, v.Rt, sizeof o.Rt);
        o.track = v.d_track; o.counts = v.d_counts; o.n = (uint32_t)v.n; o.r2 = r2;
        cull_bounds(jb.width, jb.height, jb.margin, &o.lo, &o.hi_x, &o.hi_y);
        max_n = std::max(max_n, o.n);
    }
    int rc = cull_state(ctx, "map_observe");
    if (rc != CLC_OK) return refuse(n_views - 1, rc);
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    rc = cover_rows(ctx, a.stat);
    ObserveDev od{};
    const size_t had = ctx->d_obs.bytes;                                                 // (a block that grows is a new block)
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->d_obs, 0, 1, true, "growing d_obs", [&](Carve& c) { od.carve(c, (size_t)ctx->mopts.maxkp, (size_t)std::max(n_views, 1)); });
    if (rc != CLC_OK) return refuse(n_views - 1, rc);
    // a stamp word holds the serial of the last call that hit its row: a new block holds none, and a serial never comes twice
    const bool wrapped = ctx->obs_serial + 1u == 0u;
    if (ctx->d_obs.bytes != had || wrapped) {
        CLC_HIP(ctx, hipMemsetAsync(ctx->d_obs.ptr, 0, ctx->d_obs.bytes, st));
        if (wrapped) ctx->obs_serial = 0u;
    }
    ++ctx->obs_serial;
    ++ctx->epoch;                                                                       // ONE call is ONE epoch, incremented BEFORE stamping
    for (int j = 0; j < n_views; ++j) { jobs[j].epoch = ctx->epoch; jobs[j].map_n = ctx->map_n; }
    if (n_views == 0) return CLC_OK;
    // behind whatever produced the inputs: an event on the producer's stream, no host synchronisation
    for (int j = 0; j < n_views; ++j) {
        hipStream_t prod = (hipStream_t)jobs[j].after_stream;
        if (prod && prod != st) CLC_HIP(ctx, order_behind(ctx->ev_track, prod, &st, 1));
    }
    level_scales(a.scale);
    a.map_X = ctx->d_map_X.as<double>(); a.nm = (uint32_t)ctx->map_n;
    a.serial = ctx->obs_serial; a.epoch = ctx->epoch;
    a.hit = od.hit; a.stride = od.stride;
    hipLaunchKernelGGL(observe_hit_kernel, wide_grid(max_n, (unsigned)n_views), dim3(kWide), 0, st, a);
    CLC_HIP(ctx, hipGetLastError());
    if (a.nm > 0) {
        hipLaunchKernelGGL(observe_update_kernel, wide_grid(a.nm, (unsigned)n_views), dim3(kWide), 0, st, a);
        CLC_HIP(ctx, hipGetLastError());
    }
    return CLC_OK;
}

void cull_outputs_none(clc_ctx* ctx, clc_map_cull& job)
{
    job.map_n_before = ctx && ctx->map_n > 0 ? ctx->map_n : 0;
    job.n_kept = job.map_n_before; job.n_dropped = 0; job.n_flagged = 0; job.n_ratio = 0; job.n_idle = 0; job.status = CLC_OK;
}

int map_cull(clc_ctx* ctx, clc_map_cull& job)
{
    cull_outputs_none(ctx, job);
    const auto refuse = [&](const int rc) { return job.status = rc; };
    const auto bad = [&](const char* what) { return refuse(fail(ctx, CLC_ERR_BAD_ARG, what)); };
    // everything is checked before anything is enqueued
    if (job.den <= 0 || job.num < 0 || job.min_visible < 1) return bad("map_cull: den <= 0, num < 0 or min_visible < 1");
    if (job.n_lists < 0 || job.n_lists > kMaxBatch) return bad("map_cull: a list count outside 0 .. CLC_MAX_BATCH");
    for (int l = 0; l < job.n_lists; ++l) {
        if (job.track_n[l] < 0 || (job.track_n[l] > 0 && !job.d_track[l])) return bad("map_cull: negative count / null list");
        if ((uintptr_t)job.d_track[l] & 3u) return bad("map_cull: misaligned device pointer");
    }
    if ((uintptr_t)job.d_remap & 3u) return bad("map_cull: misaligned device pointer");
    int rc = cull_state(ctx, "map_cull");
    if (rc != CLC_OK) return refuse(rc);
    const int n = ctx->map_n;
    ListArgs la{};
    uint32_t max_list = 0;
    for (int l = 0; l < job.n_lists; ++l) { la.list[l] = job.d_track[l]; la.n[l] = (uint32_t)job.track_n[l]; max_list = std::max(max_list, la.n[l]); }
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hipStream_t prod = (hipStream_t)job.after_stream;
    if (n == 0) {
        // no rows: nothing to judge, nothing to move; a list entry names no row
        ctx->stat_rows = 0;
        if (max_list > 0) {
            if (prod && prod != st) CLC_HIP(ctx, order_behind(ctx->ev_track, prod, &st, 1));
            la.remap = nullptr; la.n_before = 0;
            hipLaunchKernelGGL(cull_lists_kernel, wide_grid(max_list, (unsigned)job.n_lists), dim3(kWide), 0, st, la);
            CLC_HIP(ctx, hipGetLastError());
            CLC_HIP(ctx, hipStreamSynchronize(st));
        }
        return CLC_OK;
    }
    CullStat stat{}, stat_next{};
    CullDev cd{};
    CullPin cp{};
    rc = cover_rows(ctx, stat);
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->d_stat_next, 0, 1, true, "allocating the next map's statistics", [&](Carve& c) { stat_next.carve(c, (size_t)ctx->mopts.maxkp); });
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->d_cull, 1, 4, true, "growing d_cull", [&](Carve& c) { cd.carve(c, (size_t)n); });
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->h_cull, 1, 4, true, "growing h_cull", [&](Carve& c) { cp.carve(c, (size_t)n); });
    if (rc == CLC_OK) rc = grow(ctx, ctx->d_m_next, ctx->d_m.bytes, 0, 1, true, "allocating the next map's descriptor rows");
    if (rc == CLC_OK) rc = next_points(ctx, (size_t)n);
    if (rc != CLC_OK) return refuse(rc);
    CullRec* rec = (CullRec*)cp.rec;
    __atomic_store_n(&rec->word, kNotYet, __ATOMIC_RELAXED);
    if (prod && prod != st) CLC_HIP(ctx, order_behind(ctx->ev_track, prod, &st, 1));

    ScanArgs sa{};
    sa.stat = stat; sa.flagged = job.d_flagged;
    sa.n = (uint32_t)n; sa.epoch = ctx->epoch; sa.min_visible = (uint32_t)job.min_visible; sa.num = (uint32_t)job.num; sa.den = (uint32_t)job.den;
    sa.max_idle = job.max_idle;
    sa.remap = cd.remap; sa.d_remap = job.d_remap; sa.h_remap = cp.remap; sa.rec = cd.rec;
    hipLaunchKernelGGL(cull_scan_kernel, dim3(1), dim3(kCullGroup), 0, st, sa);
    CLC_HIP(ctx, hipGetLastError());
    MoveArgs ma{};
    ma.remap = cd.remap; ma.n = (uint32_t)n;
    ma.desc = ctx->d_m.as<uint4>(); ma.desc_out = ctx->d_m_next.as<uint4>();
    ma.X = ctx->d_map_X.as<double>(); ma.X_out = ctx->d_map_X_next.as<double>();
    ma.stat = stat; ma.stat_out = stat_next;
    hipLaunchKernelGGL(cull_move_kernel, wide_grid(4u * (uint32_t)n), dim3(kWide), 0, st, ma);
    CLC_HIP(ctx, hipGetLastError());
    if (max_list > 0) {
        la.remap = cd.remap; la.n_before = n;
        hipLaunchKernelGGL(cull_lists_kernel, wide_grid(max_list, (unsigned)job.n_lists), dim3(kWide), 0, st, la);
        CLC_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(cull_publish_kernel, dim3(1), dim3(1), 0, st, cd.rec, (uint32_t)n, rec);
    CLC_HIP(ctx, hipGetLastError());
    // ONE wait: the word the publish launch stores behind everything else
    rc = wait_pinned(ctx, &rec->word, kNotYet, st, std::chrono::steady_clock::now(), 2, "map_cull: the publish launch left no count");
    if (rc != CLC_OK) return refuse(rc);
    const unsigned long long w = __atomic_load_n(&rec->word, __ATOMIC_ACQUIRE);
    job.n_kept = (int)(uint32_t)w; job.n_dropped = (int)(uint32_t)(w >> 32);
    job.n_flagged = (int)rec->n_flagged; job.n_ratio = (int)rec->n_ratio; job.n_idle = (int)rec->n_idle;
    if (job.h_remap) memcpy(job.h_remap, cp.remap, sizeof(int32_t) * (size_t)n);
    // the install: the buffers change places, as map_update.hip installs.  The row numbering is new, so what names rows by index inside
    // the context -- the per-track state of the last grown build -- ends.
    std::swap(ctx->d_m, ctx->d_m_next);
    std::swap(ctx->d_map_X, ctx->d_map_X_next);
    std::swap(ctx->d_stat, ctx->d_stat_next);
    ctx->map_n = job.n_kept; ctx->map_X_n = job.n_kept > 0 ? job.n_kept : -1;
    ctx->stat_rows = job.n_kept;
    ctx->grow_table = nullptr;
    return CLC_OK;
}

} // namespace

} // namespace clc

using namespace clc;

extern "C" {

int clc_map_observe_dev(clc_ctx* ctx, clc_map_observe* job)
{
    if (!job) return fail(ctx, CLC_ERR_BAD_ARG, "map_observe: null job");
    return observe_batch(ctx, job, 1);
}

int clc_map_observe_batch_dev(clc_ctx* ctx, clc_map_observe* jobs, int n_views) { return observe_batch(ctx, jobs, n_views); }

int clc_map_cull_dev(clc_ctx* ctx, clc_map_cull* job)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "map_cull: null context / job");
    return map_cull(ctx, *job);
}

int clc_map_cull_rule_default(clc_map_cull* job)
{
    if (!job) return CLC_ERR_BAD_ARG;
    job->min_visible = kCullMinVisible; job->num = kCullNum; job->den = kCullDen; job->max_idle = kCullMaxIdle;
    return CLC_OK;
}

int clc_map_stats_get(clc_ctx* ctx, uint32_t* h_visible, uint32_t* h_found, uint32_t* h_last_view, uint32_t* epoch, int* rows)
{
    if (!ctx) return fail(ctx, CLC_ERR_BAD_ARG, "map_stats_get: null context");
    if (epoch) *epoch = ctx->epoch;
    if (rows) *rows = 0;
    if (!ctx->has_mat || ctx->map_n <= 0) return CLC_OK;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    CullStat stat{};
    const int rc = cover_rows(ctx, stat);
    if (rc != CLC_OK) return rc;
    const size_t bytes = sizeof(uint32_t) * (size_t)ctx->map_n;
    if (h_visible) CLC_HIP(ctx, hipMemcpyAsync(h_visible, stat.visible, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (h_found) CLC_HIP(ctx, hipMemcpyAsync(h_found, stat.found, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (h_last_view) CLC_HIP(ctx, hipMemcpyAsync(h_last_view, stat.last_view, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (rows) *rows = ctx->map_n;
    return CLC_OK;
}

int clc_cull_map_points(clc_ctx* ctx, const int32_t* h_remap, int n)
{
    if (!ctx || n < 0 || (n > 0 && !h_remap)) return fail(ctx, CLC_ERR_BAD_ARG, "cull_map_points: bad argument");
    if (ctx->map_n >= 0) return fail(ctx, CLC_ERR_STATE, "cull_map_points: the context holds map rows (clc_map_cull_dev culls rows and points together)");
    const int have = ctx->map_X_n > 0 ? ctx->map_X_n : 0;
    int32_t kept = 0;
    if (n != have || !cull_remap_valid(h_remap, n, &kept))
        return fail(ctx, CLC_ERR_BAD_ARG, "cull_map_points: the remap is not one entry per point, the kept entries 0, 1, 2, ... in ascending order");
    if (n == 0) return CLC_OK;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    CullDev cd{};
    int rc = carve_block(ctx, ctx->d_cull, 1, 4, true, "growing d_cull", [&](Carve& c) { cd.carve(c, (size_t)n); });
    if (rc == CLC_OK) rc = next_points(ctx, (size_t)n);
    if (rc != CLC_OK) return rc;
    CLC_HIP(ctx, hipMemcpyAsync(cd.remap, h_remap, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    MoveArgs ma{};
    ma.remap = cd.remap; ma.n = (uint32_t)n;
    ma.X = ctx->d_map_X.as<double>(); ma.X_out = ctx->d_map_X_next.as<double>();
    hipLaunchKernelGGL(cull_move_kernel, wide_grid(4u * (uint32_t)n), dim3(kWide), 0, ctx->stream, ma);
    CLC_HIP(ctx, hipGetLastError());
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::swap(ctx->d_map_X, ctx->d_map_X_next);
    ctx->map_X_n = kept > 0 ? kept : -1;
    return CLC_OK;
}

} // extern "C"

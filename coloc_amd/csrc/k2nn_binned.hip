// k2nn_binned.hip -- the map match around a predicted pose through a cell grid (include/coloc_hip.h: clc_match_map_binned_dev,
// clc_match_map_binned_batch_dev, clc_map_bin_build_dev, clc_map_binned_plan): the rule, the outputs and the bits of
// clc_match_map_guided_dev, without the whole-map sweep.  The projections are binned into 66 x 66 cells (bin_math.h) and a query looks at
// the at most 3 x 3 cells its window covers -- a superset of its candidates -- with the unchanged gate (proj_in_radius)
// on every row it meets.  The top-2 is a fold of keys (distance << 22) + row by min / med3, so the order the rows are met in does not
// show in the result.
//
// Three launches, all enqueue-only on the caller's stream:
//   proj_prep_kernel    k2nn_guided.hip's, unchanged: query points and projections (k2nn_proj.h)
//   bin_build_kernel    one workgroup of 1 024 threads per job: the cells' histogram in LDS (integer LDS atomics), an exclusive scan (five
//                       counters a thread, a wave scan, the waves' totals through LDS), then the records { xt, yt, row } scattered into cell
//                       order through the scanned counters as cursors.  The cell of a row is computed once and kept in 2 bytes per row;
//                       four rows of a thread are in flight at once, the one workgroup having nothing else to hide a load behind.
//   k2nn_binned_kernel  16 lanes per query, 16 queries per workgroup of 256.  The window's rows (at most three contiguous runs of the
//                       table) are read 16 records at a time, one per lane, coalesced; a lane whose record passes the gate reads that map
//                       row's 64 bytes itself and folds its key into its own running pair; the 16 pairs merge by four xor-shuffles and
//                       emit_result (k2nn_sweep.h) writes the answer.  No splits, no atomics, no arrival counter: a query's dependent
//                       loads are cell_start -> records -> rows, whatever the number of its candidates, and the first 16 records of all
//                       three runs go out together at each of those levels.
// Jobs whose plan is SWEEP (bin_plan) go through proj_batch, the guided entry's own path.
#include "clc_ctx.h"
#include "bin_math.h"
#include "proj_math.h"
#include "k2nn_proj.h"
#include "k2nn_sweep.h"
#include "k2nn_top2.h"

#include <cmath>
#include <vector>

namespace clc {

namespace {

constexpr int kBinThreads = 1024;
constexpr int kBinPerThread = 5;                                   // counters a thread scans: 5 x 1 024 slots hold the 4 357 table entries
constexpr int kBinSlots = kBinThreads * kBinPerThread;
static_assert(kBinSlots > kBinCells, "the scan covers every cell and the total behind them");
constexpr uint32_t kLanesPerQuery = 16;
constexpr uint32_t kMatchThreads = 256;
constexpr uint32_t kQueriesPerBlock = kMatchThreads / kLanesPerQuery;
constexpr uint16_t kNoCell = 0xFFFFu;                              // a row without a projection
constexpr int kBinAhead = 4;                                       // rows a thread of the bin kernel has in flight
constexpr int kFirst = 3;                                          // runs of a window: their first steps are in flight together

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef const f32x2 __attribute__((address_space(1)))* global_cf2_ptr;

struct BinJobDev {
    const uint4* q;                                                   // the frame's descriptor rows
    int32_t* out; uint16_t* best_out; uint16_t* second_out;
    const uint32_t* cnt_q;                                            // nullable: the detector's count word
    const float* qpos; const float* proj;                             // what the prep launch wrote
    u32x4* rec; int32_t* cell_start; uint16_t* cell_of;               // the table (BinnedDev, clc_layout.h)
    int32_t* cell_start_out; int32_t* cell_row_out;                   // clc_map_bin_build_dev's copies, nullable
    double rw, c;                                                     // the window's half-width, the cell's side
    float r2;
    uint32_t nq, thr, pad_;
};
struct BinJobList {
    BinJobDev j[kMaxBatch];
    const uint4* map; uint32_t nm;                                    // the context's map rows
};
static_assert(sizeof(BinJobList) <= 4096, "BinJobList is passed as a kernel argument: it must stay within the 4 KB kernarg segment");

__global__ __launch_bounds__(kBinThreads) void bin_build_kernel(const BinJobList jobs)
{
    __shared__ uint32_t s_cnt[kBinSlots];
    __shared__ uint32_t s_wave[kBinThreads / 64];
    const BinJobDev& jb = jobs.j[blockIdx.x];
    const uint32_t tid = threadIdx.x, nm = jobs.nm;
    for (uint32_t i = tid; i < (uint32_t)kBinSlots; i += kBinThreads) s_cnt[i] = 0u;
    __syncthreads();
    // the histogram: a row is binned iff it has a projection.  kBinAhead rows of a thread are in flight at once: the one workgroup has
    // nothing else to hide a load behind
    const global_cf2_ptr proj = (global_cf2_ptr)(uintptr_t)jb.proj;
    for (uint32_t base = tid; base < nm; base += kBinThreads * kBinAhead) {
        f32x2 p[kBinAhead];
#pragma unroll
        for (int a = 0; a < kBinAhead; ++a) {
            const uint32_t row = base + (uint32_t)a * kBinThreads;
            p[a] = proj[row < nm ? row : base];
        }
#pragma unroll
        for (int a = 0; a < kBinAhead; ++a) {
            const uint32_t row = base + (uint32_t)a * kBinThreads;
            if (row >= nm) continue;
            uint16_t cell = kNoCell;
            if (p[a].x == p[a].x && p[a].y == p[a].y) {
                cell = (uint16_t)bin_cell((double)p[a].x, (double)p[a].y, jb.c);
                atomicAdd(&s_cnt[cell], 1u);
            }
            jb.cell_of[row] = cell;
        }
    }
    __syncthreads();
    // the exclusive scan: slots 5 tid .. 5 tid + 4 (a stride of 5 dwords: no bank is hit twice by a half wave)
    uint32_t v[kBinPerThread], sum = 0u;
#pragma unroll
    for (int k = 0; k < kBinPerThread; ++k) { v[k] = s_cnt[kBinPerThread * tid + k]; sum += v[k]; }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if ((tid & 63u) >= (uint32_t)d) incl += o;
    }
    if ((tid & 63u) == 63u) s_wave[tid >> 6] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (uint32_t w = 0; w < (tid >> 6); ++w) run += s_wave[w];
#pragma unroll
    for (int k = 0; k < kBinPerThread; ++k) {
        const uint32_t slot = kBinPerThread * tid + k;
        s_cnt[slot] = run;                                                // the cell's cursor
        if (slot <= (uint32_t)kBinCells) {                                // (slot kBinCells: the number of binned rows)
            jb.cell_start[slot] = (int32_t)run;
            if (jb.cell_start_out) jb.cell_start_out[slot] = (int32_t)run;
        }
        run += v[k];
    }
    __syncthreads();
    // the scatter: the order inside a cell is whatever the cursor gives, the fold does not depend on it
    for (uint32_t base = tid; base < nm; base += kBinThreads * kBinAhead) {
        f32x2 p[kBinAhead];
        uint16_t cell[kBinAhead];
#pragma unroll
        for (int a = 0; a < kBinAhead; ++a) {
            const uint32_t row = base + (uint32_t)a * kBinThreads;
            p[a] = proj[row < nm ? row : base];
            cell[a] = row < nm ? jb.cell_of[row] : kNoCell;                  // (this thread wrote it)
        }
#pragma unroll
        for (int a = 0; a < kBinAhead; ++a) {
            if (cell[a] == kNoCell) continue;
            const uint32_t row = base + (uint32_t)a * kBinThreads;
            const uint32_t at = atomicAdd(&s_cnt[cell[a]], 1u);              // < the binned rows <= nm
            jb.rec[at] = u32x4{ __float_as_uint(p[a].x), __float_as_uint(p[a].y), row, 0u };
            if (jb.cell_row_out) jb.cell_row_out[at] = (int32_t)row;
        }
    }
}

__global__ __launch_bounds__(kMatchThreads) void k2nn_binned_kernel(const BinJobList jobs)
{
    const BinJobDev& jb = jobs.j[blockIdx.y];
    const uint32_t sub = threadIdx.x & (kLanesPerQuery - 1u);
    const uint32_t qi = blockIdx.x * kQueriesPerBlock + threadIdx.x / kLanesPerQuery;
    if (qi >= jb.nq) return;                                                 // (the 16 lanes of a query leave together)
    uint32_t nq_eff = jb.nq;
    if (jb.cnt_q) nq_eff = min(jb.cnt_q[0], nq_eff);
    const float xq = jb.qpos[2u * (size_t)qi], yq = jb.qpos[2u * (size_t)qi + 1u];
    uint32_t best = kEmpty, second = kEmpty;
    if (qi < nq_eff && xq == xq && yq == yq) {                               // a query without a point has no window
        uint32_t q[16];
        const global_cu4_ptr qp = (global_cu4_ptr)(uintptr_t)jb.q + (size_t)qi * 4u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32x4 w = qp[k];
            q[4 * k + 0] = w.x; q[4 * k + 1] = w.y; q[4 * k + 2] = w.z; q[4 * k + 3] = w.w;
        }
        int kx0, kx1, ky0, ky1;
        bin_window((double)xq, jb.rw, jb.c, &kx0, &kx1);
        bin_window((double)yq, jb.rw, jb.c, &ky0, &ky1);
        const global_cu4_ptr rec = (global_cu4_ptr)(uintptr_t)jb.rec;
        const global_cu4_ptr map = (global_cu4_ptr)(uintptr_t)jobs.map;
        const auto fold = [&](const u32x4 (&w)[4], const uint32_t row) {
            uint32_t dist = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                dist += __popc(q[4 * k + 0] ^ w[k].x) + __popc(q[4 * k + 1] ^ w[k].y) + __popc(q[4 * k + 2] ^ w[k].z) + __popc(q[4 * k + 3] ^ w[k].w);
            const uint32_t key = (dist << kKeyShift) + row;                      // the ABSOLUTE map row
            second = top2_med3(best, second, key);
            best = top2_min(best, key);
        };
        // the window's runs: cells ky * 66 + kx0 .. ky * 66 + kx1 are one run of the table (index <= 65 * 66 + 66 = kBinCells).  A query's
        // loads depend on one another -- table, records, rows -- and little else is in flight, so the first step of all three runs goes
        // out together at each level; a run of more than 16 rows finishes in the loop behind.
        uint32_t s[kFirst], e[kFirst];
#pragma unroll
        for (int r = 0; r < kFirst; ++r) {
            const bool on = ky0 + r <= ky1;
            const int at = (on ? ky0 + r : ky0) * kBinAxis;
            s[r] = (uint32_t)jb.cell_start[at + kx0];
            e[r] = on ? (uint32_t)jb.cell_start[at + kx1 + 1] : s[r];
        }
        u32x4 rc[kFirst];
        bool pass[kFirst];
#pragma unroll
        for (int r = 0; r < kFirst; ++r) {
            pass[r] = s[r] + sub < e[r];
            if (pass[r]) rc[r] = rec[s[r] + sub];
        }
        u32x4 w[kFirst][4];
#pragma unroll
        for (int r = 0; r < kFirst; ++r) {
            pass[r] = pass[r] && proj_in_radius(xq, yq, __uint_as_float(rc[r].x), __uint_as_float(rc[r].y), jb.r2);
            if (pass[r]) {
                const global_cu4_ptr mp = map + (size_t)rc[r].z * 4u;             // rc.z < nm: the bin kernel wrote it
#pragma unroll
                for (int k = 0; k < 4; ++k) w[r][k] = mp[k];
            }
        }
#pragma unroll
        for (int r = 0; r < kFirst; ++r)
            if (pass[r]) fold(w[r], rc[r].z);
        const auto rest = [&](const uint32_t from, const uint32_t to) {
            for (uint32_t i = from; i < to; i += kLanesPerQuery) {
                const u32x4 rr = rec[i];
                if (!proj_in_radius(xq, yq, __uint_as_float(rr.x), __uint_as_float(rr.y), jb.r2)) continue;
                const global_cu4_ptr mp = map + (size_t)rr.z * 4u;
                u32x4 wr[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) wr[k] = mp[k];
                fold(wr, rr.z);
            }
        };
#pragma unroll
        for (int r = 0; r < kFirst; ++r) rest(s[r] + sub + kLanesPerQuery, e[r]);
        // (a window of more than three cell rows: none is known to exist -- c >= rw --, but the superset must not rest on the rounding
        // of two quotients)
        for (int ky = ky0 + kFirst; ky <= ky1; ++ky)
            rest((uint32_t)jb.cell_start[ky * kBinAxis + kx0] + sub, (uint32_t)jb.cell_start[ky * kBinAxis + kx1 + 1]);
    }
    // the 16 running pairs of the query hold disjoint rows: merge them
#pragma unroll
    for (int m = (int)kLanesPerQuery / 2; m > 0; m >>= 1) {
        const uint32_t ob = __shfl_xor(best, m, (int)kLanesPerQuery), os = __shfl_xor(second, m, (int)kLanesPerQuery);
        second = top2_min(top2_min(second, os), top2_max(best, ob));
        best = top2_min(best, ob);
    }
    if (sub != 0u) return;
    emit_result<false>(jb, qi, best, second);             // every PLANNED row gets an answer; rows past a device-side count hold no key -> -1
}

// The jobs `pick` of a checked batch through prep, bin and (match: not the table alone) the match launch.  cell_start_out / cell_row_out:
// clc_map_bin_build_dev's copies of the first job's table, nullable.
int binned_launch(clc_ctx* ctx, const clc_map_guided_job* jobs, const std::vector<GatherSide>& sides, const std::vector<int>& pick_jobs, const bool match,
                  int32_t* cell_start_out, int32_t* cell_row_out, void* stream)
{
    const int n = (int)pick_jobs.size();
    const uint32_t nm = (uint32_t)ctx->map_n;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);
    std::vector<BinnedDev> dv((size_t)n);
    const int rc = carve_block(ctx, ctx->d_binned, 1, 4, true, "growing d_binned", [&](Carve& c) {
        for (int k = 0; k < n; ++k) dv[(size_t)k].carve(c, (size_t)jobs[pick_jobs[(size_t)k]].nq, nm, (size_t)kBinCells);
    });
    if (rc != CLC_OK) return rc;

    BinJobList list{};
    list.map = ctx->d_m.as<uint4>(); list.nm = nm;
    ProjPrepList prep{};
    level_scales(prep.scale);
    prep.map_X = ctx->d_map_X.as<double>(); prep.nm = nm;
    uint32_t rows = 0, max_nq = 0;
    for (int k = 0; k < n; ++k) {
        const clc_map_guided_job& job = jobs[pick_jobs[(size_t)k]];
        const BinnedDev& d = dv[(size_t)k];
        BinJobDev& b = list.j[k];
        b.q = (const uint4*)job.d_q;
        b.out = job.d_match; b.best_out = job.d_best; b.second_out = job.d_second;
        b.cnt_q = sides[(size_t)pick_jobs[(size_t)k]].count;
        b.qpos = d.qpos; b.proj = d.proj; b.rec = (u32x4*)d.rec; b.cell_start = d.cell_start; b.cell_of = d.cell_of;
        b.cell_start_out = k == 0 ? cell_start_out : nullptr; b.cell_row_out = k == 0 ? cell_row_out : nullptr;
        b.rw = bin_half_width(job.radius);
        b.c = bin_cell_side(b.rw, bin_extent(job.cam.ppx, job.cam.ppy));
        b.r2 = job.radius * job.radius;                                                 // the gate's limit, formed once, in float
        b.nq = (uint32_t)job.nq;
        b.thr = (uint32_t)(uint8_t)job.threshold;                                       // CUDAK2NN.cu:46: the kernel parameter is uint8_t
        ProjPrepJob& pj = prep.j[k];
        pj.a = sides[(size_t)pick_jobs[(size_t)k]];
        for (int i = 0; i < 12; ++i) pj.Rt[i] = job.Rt[i];
        pj.nq = b.nq;
        pj.qpos = d.qpos; pj.proj = d.proj;
        pj.qpos_out = job.d_qpos; pj.proj_out = job.d_proj;
        rows = std::max(rows, b.nq + nm);
        max_nq = std::max(max_nq, b.nq);
    }
    hipError_t e = rows > 0 ? proj_prep_launch(prep, rows, n, st) : hipSuccess;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bin_build_kernel, dim3((unsigned)n), dim3(kBinThreads), 0, st, list);
        e = hipGetLastError();
    }
    if (e == hipSuccess && match && max_nq > 0) {
        hipLaunchKernelGGL(k2nn_binned_kernel, dim3((max_nq + kQueriesPerBlock - 1u) / kQueriesPerBlock, (unsigned)n), dim3(kMatchThreads), 0, st, list);
        e = hipGetLastError();
    }
    return e == hipSuccess ? CLC_OK : fail(ctx, CLC_ERR_HIP, "match_map_binned: launch", e);
}

int binned_batch(clc_ctx* ctx, const clc_map_guided_job* jobs, const int n_jobs, void* stream)
{
    std::vector<GatherSide> sides;
    const int checked = proj_checks(ctx, jobs, n_jobs, sides);       // everything is checked before anything is enqueued
    if (checked != CLC_OK) return checked;
    std::vector<int> binned;
    std::vector<clc_map_guided_job> sweep;                          // a job without query rows has nothing to answer
    for (int j = 0; j < n_jobs; ++j) {
        if (jobs[j].nq <= 0) continue;
        if (bin_plan(jobs[j].cam.ppx, jobs[j].cam.ppy, jobs[j].radius, ctx->map_n) == BIN_PLAN_BINNED) binned.push_back(j);
        else sweep.push_back(jobs[j]);
    }
    // the SWEEP jobs together through the guided entry's path, first: a refusal there leaves nothing enqueued
    if (!sweep.empty()) {
        const int rc = proj_batch(ctx, sweep.data(), (int)sweep.size(), stream);
        if (rc != CLC_OK) return rc;
    }
    return binned.empty() ? CLC_OK : binned_launch(ctx, jobs, sides, binned, true, nullptr, nullptr, stream);
}

} // namespace

} // namespace clc

using namespace clc;

extern "C" {

int clc_match_map_binned_dev(clc_ctx* ctx, const clc_map_guided_job* job, void* stream)
{
    if (!job) return fail(ctx, CLC_ERR_BAD_ARG, "match_map_binned: null job");
    return binned_batch(ctx, job, 1, stream);
}

int clc_match_map_binned_batch_dev(clc_ctx* ctx, const clc_map_guided_job* jobs, int n_jobs, void* stream)
{
    return binned_batch(ctx, jobs, n_jobs, stream);
}

int clc_map_bin_build_dev(clc_ctx* ctx, const clc_map_guided_job* job, int32_t* d_cell_start, int32_t* d_cell_row, void* stream)
{
    if (!job) return fail(ctx, CLC_ERR_BAD_ARG, "map_bin_build: null job");
    std::vector<GatherSide> sides;
    const int checked = proj_checks(ctx, job, 1, sides);
    if (checked != CLC_OK) return checked;
    if (!d_cell_start || (ctx->map_n > 0 && !d_cell_row) || ((uintptr_t)d_cell_start & 3u) || ((uintptr_t)d_cell_row & 3u))
        return fail(ctx, CLC_ERR_BAD_ARG, "map_bin_build: null or misaligned table");
    if (!(std::isfinite(job->cam.ppx) && std::isfinite(job->cam.ppy) && job->cam.ppx > 0.0 && job->cam.ppy > 0.0))
        return fail(ctx, CLC_ERR_BAD_ARG, "map_bin_build: the principal point must be finite and positive");
    if (ctx->map_n > kBinMaxRows) return fail(ctx, CLC_ERR_CAPACITY, "map_bin_build: more than 65 536 map rows");
    return binned_launch(ctx, job, sides, std::vector<int>{ 0 }, false, d_cell_start, d_cell_row, stream);
}

int clc_map_binned_plan(const clc_ctx* ctx, const clc_camera_k3* cam, float radius, int32_t* info, double* cell_side)
{
    if (!ctx || !cam || !info) return fail(const_cast<clc_ctx*>(ctx), CLC_ERR_BAD_ARG, "map_binned_plan: null context, camera or info");
    info[0] = bin_plan(cam->ppx, cam->ppy, radius, ctx->map_n);
    info[1] = kBinAxis;
    info[2] = (int32_t)kLanesPerQuery;
    info[3] = 0;
    if (cell_side) *cell_side = bin_cell_side(bin_half_width(radius), bin_extent(cam->ppx, cam->ppy));
    return CLC_OK;
}

} // extern "C"

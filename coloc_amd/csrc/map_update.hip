// map_update.hip -- the map replaced on the device (include/coloc_hip.h: clc_map_align_dev, clc_map_align_sim_dev and the staged forms
// the batch compositions of map_build.hip end in): the tail of ColoC::updateMap (reference include/coloc/coloc.hpp:435-459) between
// setupMapDatabase and data = updateData -- matchMapFeatures(old map, new map) (GPUMatcher.hpp:157-163), matchMaps (every match kept),
// then ONE of two rules for bringing the new map to the old one: computeScaleDifference (colocUtils.hpp:184-211) + rescaleMap (:213-223),
// or this project's a-contrario similarity (clc_sim3_acransac over the common features).
// THE STEP, stated once for both rules (StepView and the step_* functions below), all enqueue-only on the context's stream:
//   step_args, step_state   the argument checks; the context's state, the capacity, n_old, the empty new map
//   step_next               d_m_next, and (not staged) d_map_X_next
//   step_behind, step_rows  behind the producer; gather_rows_kernel + the K2NN sweep (map_sweep_enqueue, inter_pose.hip): the new map's
//                           rows straight into d_m_next, then Q = the installed map (d_m), T = d_m_next, threshold 60 -> match[q] = new
//                           row of old row q, or -1
//   step_finish             the pinned mirrors out to the caller; an install is two swaps (d_m <-> d_m_next, d_map_X <-> d_map_X_next), so
//                           the previous map is intact until the last launch has run and stays the context's on every failure
// THE SCALE RULE (map_align) adds, between step_rows and step_finish:
//   map_align_kernel     ONE workgroup: the ordered compaction of wg_compact.h over the old rows -> the common lists cq / ct; the terms
//                        of the scale rule (scale_term, inter_math.h) in parallel, a chunk of 1 024 at a time in LDS; their sum by ONE
//                        lane in list order (the host's sum is sequential: the bits depend on it); scale_from_sum; the rescale, all
//                        threads striding over 3 n_new doubles, into d_map_X_next; the pinned mirrors; the record last
//   The host waits for ONE word, the record's.  The chunked one-lane sum is a second copy of inter_scale_kernel's loop (inter_dev.hip),
//   not shared with it: that kernel's code is left as it was.
// THE SIMILARITY RULE (map_align_sim) adds its own argument checks behind step_args, the clearing of the transform's counter in front of
// step_rows, and behind it: the ordered gather's map-pair form (gather.hip) -> the common lists, X_new | X_old of every common feature, the
// box of those X_old and the count, for which the host waits; the solve (pose_batch.hip: sim3_solve_dev, the rounds and the refit on the
// points where the gather left them); sim_transform_kernel over all n_new points, the pinned mirrors and the record the host waits for last.
#include "clc_ctx.h"
#include "inter_math.h"
#include "map_math.h"
#include "sim3_math.h"
#include "wg_compact.h"

#include <chrono>
#include <cstring>
#include <utility>

namespace clc {

namespace {

constexpr int kAlignThreads = 1024;
constexpr int kSumChunk = 1024;              // terms of the scale rule staged in LDS per pass of the sequential sum: one per thread

struct AlignRec { double scale; int32_t n_common, n_terms, status, ready; };      // pinned: `ready` comes out last
struct AlignJob {
    const int32_t* match;                    // n_old entries (null with n_old == 0: no sweep ran)
    const double* old_X; const double* new_X;      // the installed map's points; the new map's (new_X may BE out_X: the staged map)
    int32_t n_old, n_new;
    int32_t* cq; int32_t* ct;                // scratch: the common lists, n_old entries each
    double* out_X;                           // 3 n_new: the rescaled points
    double* h_X; int32_t* h_match;           // pinned mirrors (nullable)
    AlignRec* rec;
};

__global__ __launch_bounds__(kAlignThreads) void map_align_kernel(const AlignJob a)
{
    __shared__ uint32_t s_wave[kAlignThreads / 64];
    __shared__ double s_term[kSumChunk];
    __shared__ double s_scale;
    __shared__ int s_status;
    __shared__ uint32_t s_good;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_old = a.n_old > 0 ? (uint32_t)a.n_old : 0u, n_new = a.n_new > 0 ? (uint32_t)a.n_new : 0u;
    // 1. the common features in ascending old row (commonFeatures of the sweep, GPUMatcher.hpp:217); an index outside the new map: none
    uint32_t n_com = 0;
    for (uint32_t q0 = 0; q0 < n_old; q0 += kAlignThreads) {
        const uint32_t q = q0 + tid;
        int32_t t = -1;
        if (q < n_old) {
            t = a.match[q];
            if (t < 0 || (uint32_t)t >= n_new) t = -1;
            if (a.h_match) a.h_match[q] = t;
        }
        const bool ok = t >= 0;
        uint32_t total;
        const uint32_t c = n_com + ordered_slot<kAlignThreads>(ok, s_wave, &total);
        if (ok) { a.cq[c] = (int32_t)q; a.ct[c] = t; }       // (c < n_old: the lists hold that many)
        n_com += total;
    }
    __syncthreads();                                     // the lists of this workgroup are read back below (global memory, one workgroup)
    // 2. colocUtils.hpp:201-204 over consecutive common features: a chunk of terms in parallel into LDS, their SUM by one lane in list
    //    order.  A term that the rule's guard drops is stored as -1 (scale_term).
    const uint32_t n_pairs = n_com >= 2u ? n_com - 1u : 0u;
    double sum = 0.0; uint32_t good = 0;                             // (thread 0's)
    for (uint32_t k0 = 0; k0 < n_pairs; k0 += kSumChunk) {
        const uint32_t m = n_pairs - k0 < (uint32_t)kSumChunk ? n_pairs - k0 : (uint32_t)kSumChunk;
        for (uint32_t k = tid; k < m; k += kAlignThreads) {
            const uint32_t e = k0 + k;
            s_term[k] = scale_term(a.old_X + 3 * (size_t)a.cq[e], a.old_X + 3 * (size_t)a.cq[e + 1], a.new_X + 3 * (size_t)a.ct[e], a.new_X + 3 * (size_t)a.ct[e + 1]);
        }
        __syncthreads();
        if (tid == 0)
            for (uint32_t k = 0; k < m; ++k) { const double v = s_term[k]; if (!(v < 0.0)) { sum += v; ++good; } }
        __syncthreads();
    }
    if (tid == 0) {
        double scale;
        const int st = scale_from_sum(sum, good, &scale);
        s_scale = st == CLC_INTER_OK ? scale : 1.0;
        s_status = st == CLC_INTER_OK ? CLC_MAP_ALIGN_OK : CLC_MAP_ALIGN_NO_SCALE;
        s_good = good;
    }
    __syncthreads();                                     // (also: every term above was read from new_X before out_X, which may be new_X, changes)
    // 3. rescaleMap: every component one multiply
    const double scale = s_scale;
    for (uint32_t i = tid; i < 3u * n_new; i += kAlignThreads) {
        const double v = a.new_X[i] * scale;
        a.out_X[i] = v;
        if (a.h_X) a.h_X[i] = v;
    }
    // the record comes out last: every wave's stores are complete and visible system-wide before the word the host polls changes
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
        a.rec->scale = scale; a.rec->n_common = (int32_t)n_com; a.rec->n_terms = (int32_t)s_good; a.rec->status = s_status;
        __hip_atomic_store(&a.rec->ready, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

struct SimRec { int32_t ready, pad_; };
struct SimApply {
    const double* new_X; double* out_X; double* h_X;       // (new_X may BE out_X: every thread reads its point before it writes it)
    const int32_t* match; int32_t* h_match;                // the sweep's matches -> the cleaned mirror (nullable)
    int32_t n_old, n_new, mode, found;
    double s, A[12];
    SimRec* rec;
};
constexpr int kSimThreads = 256;
__global__ __launch_bounds__(kSimThreads) void sim_transform_kernel(const SimApply a, unsigned int* done /* device: workgroups that have finished */)
{
    const uint32_t i = blockIdx.x * kSimThreads + threadIdx.x;
    if (i < (uint32_t)a.n_new) {
        const double X[3] = { a.new_X[3 * (size_t)i], a.new_X[3 * (size_t)i + 1], a.new_X[3 * (size_t)i + 2] };
        double o[3] = { X[0], X[1], X[2] };                    // no model: the bits as they are
        if (a.found) {
            if (a.mode == CLC_SIM_APPLY_FULL) sim3_apply_point(a.A, X, o);
            else { o[0] = X[0] * a.s; o[1] = X[1] * a.s; o[2] = X[2] * a.s; }
        }
        for (int c = 0; c < 3; ++c) {
            a.out_X[3 * (size_t)i + c] = o[c];
            if (a.h_X) a.h_X[3 * (size_t)i + c] = o[c];
        }
    }
    if (a.h_match && i < (uint32_t)a.n_old) {
        int32_t t = a.match[i];
        if (t < 0 || t >= a.n_new) t = -1;
        a.h_match[i] = t;
    }
    // the record comes out last: the workgroup that finishes last (a counter in device memory, cleared in front of the launch) publishes it
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int before = atomicAdd(done, 1u);
        if (before + 1u == gridDim.x) {
            __threadfence_system();
            __hip_atomic_store(&a.rec->ready, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---- the step, each piece once over one view of the two jobs -----------------------------------------------------------------------------
// What clc_map_align and clc_map_align_sim have in common, as values and pointers; each rule fills it from its own job (step_view).
// staged: d_X is the context's own d_map_X_next (the staged map), rewritten in place.  srcs + d_cam (both or neither): a grown stage, new
// row i = row d_rows[i] of block srcs->src[d_cam[i]]
struct StepView {
    const char* who;                         // "map_align" / "map_align_sim": the prefix of every message
    const void* d_desc; const int32_t* d_rows; const double* d_X;
    int n_new, threshold, install;
    void* after_stream;
    int32_t* match; double* X;               // host, nullable
    int* n_old;                              // out
    bool staged; const RowSources* srcs; const int32_t* d_cam;
};
template <class Job> StepView step_view(const char* who, Job& job, const bool staged, const RowSources* srcs, const int32_t* d_cam)
{
    return StepView{ who, job.d_desc, job.d_rows, job.d_X, job.n_new, job.threshold, job.install, job.after_stream, job.match, job.X, &job.n_old, staged, srcs, d_cam };
}
int step_fail(clc_ctx* ctx, const StepView& v, const int code, const char* what) { return fail(ctx, code, (std::string(v.who) + what).c_str()); }

int step_args(clc_ctx* ctx, const StepView& v)
{
    if (!ctx->has_mat) return step_fail(ctx, v, CLC_ERR_STATE, ": context created without matcher options");
    if (v.n_new < 0 || (v.n_new > 0 && (!v.d_desc || !v.d_X))) return step_fail(ctx, v, CLC_ERR_BAD_ARG, ": negative count / null block");
    if (((uintptr_t)v.d_desc & 15u) || ((uintptr_t)v.d_rows & 3u) || ((uintptr_t)v.d_X & 7u)) return step_fail(ctx, v, CLC_ERR_BAD_ARG, ": misaligned device pointer");
    return CLC_OK;
}

// the context's state, the capacity, n_old; *empty: the new map has no rows and the step is complete
int step_state(clc_ctx* ctx, const StepView& v, bool* empty)
{
    const int rc = map_align_state(ctx, v.who);
    if (rc != CLC_OK) return rc;
    if ((uint32_t)v.n_new > ctx->mopts.maxkp) return step_fail(ctx, v, CLC_ERR_CAPACITY, ": more map rows than MatcherOptions.maxkp (the previous map stays)");
    const int n_old = *v.n_old = ctx->map_n;
    *empty = v.n_new == 0;
    if (*empty) {
        // nothing to match, nothing to scale: the empty map, as clc_map_build_dev installs it
        if (v.match) for (int q = 0; q < n_old; ++q) v.match[q] = -1;
        if (v.install) { ctx->map_n = 0; ctx->map_X_n = -1; map_rows_replaced(ctx); }
    }
    return CLC_OK;
}

// the next map's descriptor rows and (not staged) its points
int step_next(clc_ctx* ctx, const StepView& v)
{
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    MapPointsDev next;
    int rc = grow(ctx, ctx->d_m_next, ctx->d_m.bytes, 0, 1, true, "allocating the next map's descriptor rows");
    if (rc == CLC_OK && !v.staged) rc = carve_block(ctx, ctx->d_map_X_next, 1, 4, true, "growing the next map's points", [&](Carve& c) { next.carve(c, (size_t)v.n_new); });
    return rc;
}

// behind whatever produced the new map: an event on the producer's stream, no host synchronisation
int step_behind(clc_ctx* ctx, const StepView& v)
{
    hipStream_t st = ctx->stream, prod = (hipStream_t)v.after_stream;
    if (prod && prod != st) CLC_HIP(ctx, order_behind(ctx->ev_track, prod, &st, 1));
    return CLC_OK;
}

// the new rows into the NEXT map's buffer (the installed map's rows are the sweep's queries: they stay where they are) and the sweep
// into lists.match; a failed enqueue of the sweep drains the stream
int step_rows(clc_ctx* ctx, const StepView& v, const AlignDev& lists)
{
    hipStream_t st = ctx->stream;
    const int n_old = *v.n_old;
    uint4* rows = ctx->d_m_next.as<uint4>();
    int rc = CLC_OK;
    if (v.srcs) {
        CLC_HIP(ctx, launch_gather_rows_multi(*v.srcs, v.d_cam, v.d_rows, rows, (uint32_t)v.n_new, st));
        if (n_old > 0) rc = map_sweep_rows_enqueue(ctx, v.n_new, ctx->d_m.ptr, n_old, rows, lists.match, v.threshold, st);
    } else if (n_old > 0) {
        rc = map_sweep_enqueue(ctx, v.d_desc, v.d_rows, v.n_new, ctx->d_m.ptr, n_old, rows, lists.match, v.threshold, st);
    } else if (v.install) {
        CLC_HIP(ctx, launch_gather_rows((const uint4*)v.d_desc, v.d_rows, rows, (uint32_t)v.n_new, st));
    }
    if (rc != CLC_OK) (void)hipStreamSynchronize(st);
    return rc;
}

// the pinned mirrors the rule's kernel filled (null: not asked for) out to the caller, and the install
void step_finish(clc_ctx* ctx, const StepView& v, const int32_t* h_match, const double* h_X)
{
    if (h_match) memcpy(v.match, h_match, sizeof(int32_t) * (size_t)*v.n_old);
    if (h_X) memcpy(v.X, h_X, sizeof(double) * 3 * (size_t)v.n_new);
    if (v.install) {
        std::swap(ctx->d_m, ctx->d_m_next);
        std::swap(ctx->d_map_X, ctx->d_map_X_next);
        ctx->map_n = v.n_new; ctx->map_X_n = v.n_new;
        map_rows_replaced(ctx);
    }
}

// ---- the scale rule (clc_map_align_dev) ---------------------------------------------------------------------------------------------------
int map_align(clc_ctx* ctx, clc_map_align& job, const bool staged, const RowSources* srcs = nullptr, const int32_t* d_cam = nullptr)
{
    align_outputs_none(job);
    const StepView v = step_view("map_align", job, staged, srcs, d_cam);
    bool empty = false;
    int rc = step_args(ctx, v);
    if (rc == CLC_OK) rc = step_state(ctx, v, &empty);
    if (rc != CLC_OK || empty) return rc;
    const int n_old = job.n_old, n_new = job.n_new;
    hipStream_t st = ctx->stream;
    // the match and the common lists, their pinned mirror (AlignDev, AlignPin)
    AlignDev dev; AlignPin pin;
    rc = step_next(ctx, v);
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->d_align, 1, 4, true, "growing the map alignment block", [&](Carve& c) { dev.carve(c, (size_t)n_old); });
    if (rc == CLC_OK)
        rc = carve_block(ctx, ctx->h_align, 1, 4, true, "growing the pinned map alignment block",
                         [&](Carve& c) { pin.carve(c, (size_t)n_old, (size_t)n_new, sizeof(AlignRec), alignof(AlignRec)); });
    if (rc != CLC_OK) return rc;
    AlignJob a{};
    a.match = n_old > 0 ? dev.match : nullptr;
    a.cq = dev.cq; a.ct = dev.ct;
    a.old_X = ctx->d_map_X.as<double>(); a.new_X = job.d_X; a.out_X = ctx->d_map_X_next.as<double>();
    a.n_old = n_old; a.n_new = n_new;
    a.rec = (AlignRec*)pin.rec;
    a.h_X = job.X ? pin.X : nullptr; a.h_match = job.match && n_old > 0 ? pin.match : nullptr;
    __atomic_store_n(&a.rec->ready, 0, __ATOMIC_RELAXED);
    rc = step_behind(ctx, v);
    if (rc == CLC_OK) rc = step_rows(ctx, v, dev);
    if (rc != CLC_OK) return rc;
    hipLaunchKernelGGL(map_align_kernel, dim3(1), dim3(kAlignThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(ctx, CLC_ERR_HIP, "map_align: the align launch", e); }
    // the one word the host needs; the kernel is the last launch, so the gather and the sweep have run when it is out
    rc = wait_pinned(ctx, &a.rec->ready, 0, st, std::chrono::steady_clock::now(), 5, "map_align: the align launch left no record");
    if (rc != CLC_OK) return rc;
    job.scale = a.rec->scale; job.n_common = a.rec->n_common; job.n_terms = a.rec->n_terms; job.status = a.rec->status;
    step_finish(ctx, v, a.h_match, a.h_X);
    return CLC_OK;
}

// ---- the similarity rule (clc_map_align_sim_dev) -------------------------------------------------------------------------------------------
int map_align_sim(clc_ctx* ctx, clc_map_align_sim& job, const bool staged, const RowSources* srcs = nullptr, const int32_t* d_cam = nullptr)
{
    sim_outputs_none(job);
    const StepView v = step_view("map_align_sim", job, staged, srcs, d_cam);
    bool empty = false;
    int rc = step_args(ctx, v);
    if (rc != CLC_OK) return rc;
    if (job.apply != CLC_SIM_APPLY_SCALE && job.apply != CLC_SIM_APPLY_FULL) return fail(ctx, CLC_ERR_BAD_ARG, "map_align_sim: apply must be CLC_SIM_APPLY_SCALE or CLC_SIM_APPLY_FULL");
    if (job.max_iteration < 0) return fail(ctx, CLC_ERR_BAD_ARG, "map_align_sim: negative max_iteration");
    rc = step_state(ctx, v, &empty);
    if (rc != CLC_OK || empty) return rc;
    const int n_old = job.n_old, n_new = job.n_new;
    hipStream_t st = ctx->stream;
    const size_t cap = (size_t)(n_old < kAcrMaxN ? n_old : kAcrMaxN);
    AlignSimDev dev; AlignSimPin pin;
    rc = step_next(ctx, v);
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->d_align, 1, 4, true, "growing the map alignment block", [&](Carve& c) { dev.carve(c, (size_t)n_old, cap); });
    if (rc == CLC_OK)
        rc = carve_block(ctx, ctx->h_align, 1, 4, true, "growing the pinned map alignment block",
                         [&](Carve& c) { pin.carve(c, (size_t)n_old, (size_t)n_new, sizeof(SimRec), alignof(SimRec)); });
    if (rc != CLC_OK) return rc;
    int32_t* d_match = dev.lists.match;
    SimRec* rec = (SimRec*)pin.rec;
    __atomic_store_n(pin.h_n, 0xFFFFFFFFu, __ATOMIC_RELAXED);
    __atomic_store_n(&rec->ready, 0, __ATOMIC_RELAXED);
    rc = step_behind(ctx, v);
    if (rc != CLC_OK) return rc;
    CLC_HIP(ctx, hipMemsetAsync(dev.done, 0, sizeof(unsigned int), st));
    rc = step_rows(ctx, v, dev.lists);
    if (rc != CLC_OK) return rc;
    // the common features as 3-D / 3-D pairs, their box and their count
    MapPairJobs pj{};
    MapPairJobDev& g = pj.j[0];
    g.match = d_match; g.nq = n_old; g.cap = (int)cap; g.n = nullptr; g.h_n = pin.h_n;
    g.old_X = ctx->d_map_X.as<double>(); g.new_X = job.d_X; g.n_new = n_new;
    g.xn = dev.xn; g.xo = dev.xo; g.cq = dev.lists.cq; g.ct = dev.lists.ct; g.h_box = pin.box;
    hipError_t e = launch_gather(pj, st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(ctx, CLC_ERR_HIP, "map_align_sim: the gather launch", e); }
    rc = wait_pinned(ctx, pin.h_n, 0xFFFFFFFFu, st, std::chrono::steady_clock::now(), 5, "map_align_sim: the gather launch left no count");
    if (rc != CLC_OK) return rc;
    const uint32_t n_common = __atomic_load_n(pin.h_n, __ATOMIC_ACQUIRE);
    job.n_common = (int)n_common;
    if (n_common > (uint32_t)kAcrMaxN) return fail(ctx, CLC_ERR_CAPACITY, "map_align_sim: more than 16384 common features (the previous map stays)");
    // the solve on the pairs where they lie
    Sim3Out o{};
    int n_inl = 0, its = 0;
    double emax = 0.0, nfa = INFINITY;
    double box[6];
    memcpy(box, pin.box, sizeof box);
    rc = sim3_solve_dev(ctx, dev.xn, dev.xo, (int)n_common, box, job.max_iteration > 0 ? job.max_iteration : 256, job.seed, job.precision, &o,
                        job.inlier, &n_inl, &emax, &nfa, &its);
    if (rc != CLC_OK) return rc;
    // every point of the new map
    SimApply a{};
    a.new_X = job.d_X; a.out_X = ctx->d_map_X_next.as<double>(); a.h_X = job.X ? pin.X : nullptr;
    a.match = d_match; a.h_match = job.match && n_old > 0 ? pin.match : nullptr;
    a.n_old = n_old; a.n_new = n_new; a.mode = job.apply; a.found = o.found; a.s = o.s;
    memcpy(a.A, o.A, sizeof a.A);
    a.rec = rec;
    const int most = n_new > n_old ? n_new : n_old;
    hipLaunchKernelGGL(sim_transform_kernel, dim3((unsigned)((most + kSimThreads - 1) / kSimThreads)), dim3(kSimThreads), 0, st, a, dev.done);
    e = hipGetLastError();
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(ctx, CLC_ERR_HIP, "map_align_sim: the transform launch", e); }
    rc = wait_pinned(ctx, &rec->ready, 0, st, std::chrono::steady_clock::now(), 5, "map_align_sim: the transform launch left no record");
    if (rc != CLC_OK) return rc;
    job.n_inliers = n_inl; job.iterations = its; job.refit = o.refit; job.status = o.found ? CLC_MAP_SIM_OK : CLC_MAP_SIM_NO_MODEL;
    job.s = o.s; memcpy(job.R, o.R, sizeof job.R); memcpy(job.t, o.t, sizeof job.t);
    job.error_max = emax; job.min_nfa = nfa;
    step_finish(ctx, v, a.h_match, a.h_X);
    return CLC_OK;
}

// ---- a rule on a staged map (the batch compositions, map_build.hip) ----------------------------------------------------------------------
// The in fields both rules read, from the stage half: the rows of the lower seed camera's block (a grown stage: of every camera's, srcs),
// the staged points in place, installing, the host points into job.X; threshold and match as the caller `asked`
template <class Step> void staged_inputs(clc_ctx* ctx, const clc_map_job& job, const MapStaged& staged, const Step& asked, Step& a, RowSources& srcs)
{
    for (int c = 0; c < job.tracks.n_cams && c < kMaxBatch; ++c) srcs.src[c] = (const uint4*)job.cams[c].d_desc;
    a.d_desc = job.cams[staged.cam_i].d_desc; a.d_rows = staged.d_row; a.d_X = ctx->d_map_X_next.as<double>(); a.n_new = staged.n;
    a.threshold = asked.threshold; a.install = 1; a.after_stream = nullptr;          // (the stage half ran on the context's stream)
    a.match = asked.match; a.X = job.X;
}

// what the rule did to the points, done to the poses: the two seed cameras' and (gr) every resected or seed camera's in the grow record
// (rescaleMap multiplies every pose's centre, colocUtils.hpp:213-223: the resected cameras' too)
template <class Op> void staged_poses(clc_map_job& job, const MapStaged& staged, clc_map_grow* gr, const Op& op)
{
    op(job.Rt_seed_a);
    op(job.Rt_seed_b);
    if (gr)
        for (int c = 0; c < job.tracks.n_cams; ++c)
            if (gr->resected[c] || c == staged.cam_i || c == staged.cam_j) op(gr->Rt[c]);
}

} // namespace

void align_outputs_none(clc_map_align& job)
{
    job.n_old = 0; job.n_common = 0; job.n_terms = 0; job.status = CLC_MAP_ALIGN_NO_SCALE; job.scale = 1.0;
}

void sim_outputs_none(clc_map_align_sim& job)
{
    job.n_old = 0; job.n_common = 0; job.n_inliers = 0; job.iterations = 0; job.refit = 0; job.status = CLC_MAP_SIM_NO_MODEL;
    job.s = 1.0; job.error_max = 0.0; job.min_nfa = INFINITY;
    for (int q = 0; q < 9; ++q) job.R[q] = q % 4 == 0 ? 1.0 : 0.0;
    for (int q = 0; q < 3; ++q) job.t[q] = 0.0;
}

int map_align_state(clc_ctx* ctx, const char* who)
{
    if (ctx->map_n < 0 || ctx->map_X_n < 0 || ctx->map_X_n < ctx->map_n)
        return fail(ctx, CLC_ERR_STATE, (std::string(who) + ": the context holds no map with points (clc_set_map + clc_set_map_points, or a build)").c_str());
    return CLC_OK;
}

int map_align_staged(clc_ctx* ctx, clc_map_job& job, const MapStaged& staged, clc_map_align& align, clc_map_grow* gr)
{
    RowSources srcs{};
    clc_map_align a{};
    staged_inputs(ctx, job, staged, align, a, srcs);
    const int rc = map_align(ctx, a, true, staged.d_cam ? &srcs : nullptr, staged.d_cam);
    align.n_old = a.n_old; align.n_common = a.n_common; align.n_terms = a.n_terms; align.status = a.status; align.scale = a.scale;
    if (rc != CLC_OK) return job.status = rc;
    staged_poses(job, staged, gr, [&](double* Rt) { rescale_pose(Rt, a.scale); });
    return CLC_OK;
}

int map_align_sim_staged(clc_ctx* ctx, clc_map_job& job, const MapStaged& staged, clc_map_align_sim& sim, clc_map_grow* gr)
{
    RowSources srcs{};
    clc_map_align_sim a{};
    staged_inputs(ctx, job, staged, sim, a, srcs);
    a.apply = sim.apply; a.max_iteration = sim.max_iteration; a.seed = sim.seed; a.precision = sim.precision; a.inlier = sim.inlier;
    const int rc = map_align_sim(ctx, a, true, staged.d_cam ? &srcs : nullptr, staged.d_cam);
    sim.n_old = a.n_old; sim.n_common = a.n_common; sim.n_inliers = a.n_inliers; sim.iterations = a.iterations; sim.refit = a.refit;
    sim.status = a.status; sim.s = a.s; sim.error_max = a.error_max; sim.min_nfa = a.min_nfa;
    memcpy(sim.R, a.R, sizeof sim.R); memcpy(sim.t, a.t, sizeof sim.t);
    if (rc != CLC_OK) return job.status = rc;
    if (a.status != CLC_MAP_SIM_OK) return CLC_OK;               // no model: the poses as they are
    staged_poses(job, staged, gr, [&](double* Rt) { if (a.apply == CLC_SIM_APPLY_FULL) sim3_apply_pose(a.s, a.R, a.t, Rt); else rescale_pose(Rt, a.s); });
    return CLC_OK;
}

} // namespace clc

using namespace clc;

extern "C" {

int clc_map_align_dev(clc_ctx* ctx, clc_map_align* job)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "map_align: null context / job");
    return map_align(ctx, *job, false);
}

int clc_map_align_sim_dev(clc_ctx* ctx, clc_map_align_sim* job)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "map_align_sim: null context / job");
    return map_align_sim(ctx, *job, false);
}

} // extern "C"

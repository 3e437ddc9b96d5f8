// k2nn_guided.hip -- the guided match: K2NN's top-2 and acceptance over the train rows within `band` pixels of the query's epipolar
// line under a known F (include/coloc_hip.h, clc_match_guided_dev / clc_match_guided_batch_dev, which state the rule).
//
// Two kernels, both enqueue-only on the caller's stream:
//   guided_prep_kernel        one thread per row of either camera: feature position, get_ud_pixel in fp64 (ud_pixel.h, the copy the pair
//                             kernel runs), then guided_line (guided_math.h) for a query row -> L, 3 floats; the pixel rounded to float for a
//                             train row -> (x, y), 2 floats.  Rows past a device-side count, and queries without a line, carry NaNs: they
//                             can never pass the gate.
//   k2nn_sweep_guided_kernel  the popcount sweep (k2nn_sweep.h: the ONE body behind this kernel and k2nn.hip's k2nn_sweep_kernel -- lane =
//                             query, the train row wave-uniform in SGPRs, the 2-D decomposition, the pipelined loop, the LDS fold, the
//                             atomic fold and the arrival-counter finalize) with a gate: the lane keeps the lines of its
//                             kR queries in six VGPRs, the train point arrives as the train row does -- one s_load_dwordx2 beside the
//                             s_load_dwordx16, a vector ahead --, and a non-candidate's key becomes kEmpty in front of the med3 / min pair
//                             (v_fma, v_fma, v_cmp, v_cndmask per pair: no branch).  Each v_fma reads ONE scalar operand (the train
//                             coordinate) next to two vector operands, the v_cmp one (the band): within the one-SGPR-per-instruction rule
//                             of the gfx9 vector ALU, so no v_mov copies a scalar into the loop.
// It runs whatever formulation the context is set to: a per-pair gate has no place in the matrix sweep, whose C operand is per tile.
// The jobs travel in records of their own (GuidedJobList), not in K2nnJobDev, whose layout the matrix sweep is compiled against.  This
// file owns the gates, the record, how its live counts are read (counted) and the kernel's entry; everything behind that is the body's.
//
// The same sweep serves the map match guided by a predicted pose (clc_match_map_guided_dev / clc_match_map_guided_batch_dev): the GATE is
// the body's template parameter (sweep_one, sweep_rows).
//   LineGate   3 floats per query (the line), limit = band:  v_fma, v_fma, v_cmp, v_cndmask per pair
//   PointGate  2 floats per query (the undistorted pixel), limit = r2 = radius^2; the train point is the landmark's projection under the
//              predicted [R|t]:  v_sub, v_sub, v_mul, v_fma, v_cmp, v_cndmask per pair (proj_in_radius, proj_math.h) -- each still reads at
//              most one scalar operand.  (A lane holds two queries, and the compiler pairs them in packed fp32: v_pk_add_f32 twice,
//              v_pk_mul_f32, v_pk_fma_f32 per train row, then v_cmp and v_cndmask per query -- IEEE fp32 per half, the same bits.)
//   proj_prep_kernel  one thread per row: a query row's undistorted pixel (what the track kernel computes for pt2D), a map row's
//              projection (proj_point from the context's d_map_X), each rounded once to float
#include "clc_ctx.h"
#include "guided_math.h"
#include "proj_math.h"
#include "k2nn_proj.h"
#include "k2nn_sweep.h"
#include "k2nn_top2.h"
#include "ud_pixel.h"

#include <cmath>
#include <vector>

namespace clc {

namespace {

constexpr int kGuidedMaxJobs = CLC_MAX_TRACK_PAIRS;
// One prep record is 272 bytes (two cameras and F in fp64), so a 4 KB kernel argument carries 14 of them: a batch of up to 14 jobs is
// ONE prep launch, a larger one (up to kGuidedMaxJobs = 28) two.  The sweep's records are smaller: always ONE sweep launch.
constexpr int kGuidedPrepJobs = 14;

struct GuidedPrepJob {
    GatherSide a, b;                  // the two cameras' rows, counts and intrinsics, as the pair kernel takes them
    double F[9];
    uint32_t nq, nt;                  // planned rows
    float* L; float* pos;             // the context's scratch: 3 nq / 2 nt floats
    float* line_out; float* tpos_out; // the caller's copies, nullable
};
struct GuidedPrepList {
    GuidedPrepJob j[kGuidedPrepJobs];
    float scale[CLC_MAX_LEVELS];      // as PairJobs::scale
};
static_assert(sizeof(GuidedPrepList) <= 4096, "GuidedPrepList is passed as a kernel argument: it must stay within the 4 KB kernarg segment");

struct GuidedJobDev {
    const uint4* q; const uint4* t;
    int32_t* out; uint16_t* best_out; uint16_t* second_out;
    const float* L; const float* pos;                                 // the gate's floats of every query row (Gate::kF each) / train points
    const uint32_t* cnt_q; const uint32_t* cnt_t;                     // nullable: the detectors' count words
    uint32_t nq, nt, thr;
    uint32_t qblocks, splits, t_per_split, partial_off, cnt_off;      // k2nn_plan's, popcount formulation, atomic fold
    float band;                                                       // the gate's limit: LineGate's band, PointGate's r2
    uint32_t pad_;
};
struct GuidedJobList { GuidedJobDev j[kGuidedMaxJobs]; };
static_assert(sizeof(GuidedJobList) <= 4096, "GuidedJobList is passed as a kernel argument: it must stay within the 4 KB kernarg segment");

// (the map match's prep records, ProjPrepJob / ProjPrepList: k2nn_proj.h, shared with k2nn_binned.hip)

// The two gates.  kF floats of a query stay in the lane's registers; pass() is the ONE statement of the gate (guided_math.h / proj_math.h).
struct LineGate {
    static constexpr int kF = 3;
    static __device__ __forceinline__ bool pass(const float (&g)[3], const float x, const float y, const float lim) { return guided_in_band(g[0], g[1], g[2], x, y, lim); }
};
struct PointGate {
    static constexpr int kF = 2;
    static __device__ __forceinline__ bool pass(const float (&g)[2], const float x, const float y, const float lim) { return proj_in_radius(g[0], g[1], x, y, lim); }
};

__device__ __forceinline__ uint32_t counted(const uint32_t planned, const uint32_t* count)
{
    if (!count) return planned;
    const uint32_t c = count[0];
    return c < planned ? c : planned;
}

__global__ __launch_bounds__(256) void guided_prep_kernel(const GuidedPrepList jobs)
{
    const GuidedPrepJob& jb = jobs.j[blockIdx.y];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= jb.nq + jb.nt) return;
    const bool is_q = i < jb.nq;
    const uint32_t row = is_q ? i : i - jb.nq;
    const GatherSide& s = is_q ? jb.a : jb.b;
    const bool there = row < counted(is_q ? jb.nq : jb.nt, s.count);
    double u[2] = { 0.0, 0.0 };
    if (there) {
        float fx, fy;
        feature_position(s.kps, s.feat, s.feat_stride, row, jobs.scale, &fx, &fy);
        ud_pixel(fx, fy, s.cam, u);
    }
    if (is_q) {
        float L[3] = { guided_none(), guided_none(), guided_none() };
        if (there) guided_line(jb.F, u[0], u[1], L);
        float* o = jb.L + 3u * (size_t)row;
        o[0] = L[0]; o[1] = L[1]; o[2] = L[2];
        if (jb.line_out) { float* c = jb.line_out + 3u * (size_t)row; c[0] = L[0]; c[1] = L[1]; c[2] = L[2]; }
    } else {
        const float x = there ? (float)u[0] : guided_none(), y = there ? (float)u[1] : guided_none();
        float* o = jb.pos + 2u * (size_t)row;
        o[0] = x; o[1] = y;
        if (jb.tpos_out) { float* c = jb.tpos_out + 2u * (size_t)row; c[0] = x; c[1] = y; }
    }
}

__global__ __launch_bounds__(256) void proj_prep_kernel(const ProjPrepList jobs)
{
    const ProjPrepJob& jb = jobs.j[blockIdx.y];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= jb.nq + jobs.nm) return;
    float xy[2] = { guided_none(), guided_none() };
    if (i < jb.nq) {
        if (i < counted(jb.nq, jb.a.count)) {
            float fx, fy;
            double u[2];
            feature_position(jb.a.kps, jb.a.feat, jb.a.feat_stride, i, jobs.scale, &fx, &fy);
            ud_pixel(fx, fy, jb.a.cam, u);
            xy[0] = (float)u[0]; xy[1] = (float)u[1];
        }
        float* o = jb.qpos + 2u * (size_t)i;
        o[0] = xy[0]; o[1] = xy[1];
        if (jb.qpos_out) { float* c = jb.qpos_out + 2u * (size_t)i; c[0] = xy[0]; c[1] = xy[1]; }
    } else {
        const uint32_t row = i - jb.nq;
        const ProjCamera cam{ jb.a.cam.focal, jb.a.cam.ppx, jb.a.cam.ppy };
        proj_point(jb.Rt, cam, jobs.map_X + 3u * (size_t)row, xy);
        float* o = jb.proj + 2u * (size_t)row;
        o[0] = xy[0]; o[1] = xy[1];
        if (jb.proj_out) { float* c = jb.proj_out + 2u * (size_t)row; c[0] = xy[0]; c[1] = xy[1]; }
    }
}

// The gated popcount sweep: the one body of k2nn_sweep.h with the gate.  The kernel's own: GuidedJobDev and its live counts (counted),
// the return when nothing is planned to sweep, the K2NN rule, always the atomic fold (guided_plan refuses every other plan).
template <int R, class Gate>
__global__ __launch_bounds__(64 * kWaves) void k2nn_sweep_guided_kernel(const GuidedJobList jobs, uint2* __restrict__ partial)
{
    const GuidedJobDev& job = jobs.j[blockIdx.y];
    if (job.nt == 0u) return;                                             // nothing planned to sweep: guided_nomatch_kernel answers
    const uint32_t job_nq = counted(job.nq, job.cnt_q), job_nt = counted(job.nt, job.cnt_t);
    SweepSplit<R> sp;
    if (sweep_split<R, Gate>(job, job_nq, job_nt, sp)) sweep_fold_finalize<R, false>(job, job_nq, partial, sp);
}

// jobs with an EMPTY planned train set (nomatch_rows, k2nn_sweep.h)
__global__ __launch_bounds__(256) void guided_nomatch_kernel(const GuidedJobList jobs) { nomatch_rows(jobs); }

// What the two gates share behind their argument checks.  kj: the live jobs' nq / nt.  The popcount formulation's plan, whatever the
// context's sweeps run; the scratch -- every job's query floats (qf per row), then its train points, each block starting on 16 bytes --
// through d_guided's one grow path; the top-2 workspace, cleared if need be; and the sweep's record of every job as far as the plan and
// the scratch decide it.
int guided_plan(clc_ctx* ctx, const char* over_capacity, std::vector<K2nnJobDev>& kj, const int qf, hipStream_t st, GuidedJobList& list)
{
    const int n = (int)kj.size();
    const int target = ctx->target_blocks > 0 && ctx->formulation == K2NN_POPCOUNT ? ctx->target_blocks : default_target_blocks(K2NN_POPCOUNT, ctx->k2dev);
    const K2nnPlan plan = k2nn_plan(kj.data(), n, target, ctx->xcd_map, K2NN_POPCOUNT, 0, 0, ctx->k2dev);
    if (!plan.atomic_merge) return fail(ctx, CLC_ERR_CAPACITY, over_capacity);

    std::vector<GuidedDev> dv((size_t)n);
    int rc = carve_block(ctx, ctx->d_guided, 1, 4, true, "growing d_guided", [&](Carve& c) {
        for (int k = 0; k < n; ++k) dv[(size_t)k].carve(c, (size_t)qf, kj[(size_t)k].nq, kj[(size_t)k].nt);
    });
    if (rc == CLC_OK) rc = ensure_partial(ctx, plan.partial_elems);
    if (rc != CLC_OK) return rc;
    if (ctx->partial_dirty) {
        CLC_HIP(ctx, hipMemsetAsync(ctx->d_partial.ptr, 0xFF, ctx->d_partial.bytes, st));
        ctx->partial_dirty = false;
    }
    for (int k = 0; k < n; ++k) {
        const K2nnJobDev& p = kj[(size_t)k];
        GuidedJobDev& g = list.j[k];
        g.L = dv[(size_t)k].L; g.pos = dv[(size_t)k].pos;
        g.nq = p.nq; g.nt = p.nt;
        g.qblocks = p.qblocks; g.splits = p.splits; g.t_per_split = p.t_per_split; g.partial_off = p.partial_off; g.cnt_off = p.cnt_off;
    }
    return CLC_OK;
}

// the sweep behind a prep launch (e: what that launch left) and, for the jobs with an empty train side, the answer without one
template <class Gate> int guided_sweep(clc_ctx* ctx, const char* who, hipError_t e, const GuidedJobList& list, const int n, hipStream_t st)
{
    uint32_t grid_x = 0, max_nq_empty = 0;
    for (int k = 0; k < n; ++k) {
        if (list.j[k].nt) grid_x = std::max(grid_x, list.j[k].qblocks * list.j[k].splits);
        else max_nq_empty = std::max(max_nq_empty, list.j[k].nq);
    }
    if (e == hipSuccess && grid_x > 0) {
        hipLaunchKernelGGL((k2nn_sweep_guided_kernel<kR, Gate>), dim3(grid_x, (unsigned)n), dim3(64 * kWaves), 0, st, list, ctx->d_partial.as<uint2>());
        e = hipGetLastError();
    }
    if (e == hipSuccess && max_nq_empty > 0) {
        hipLaunchKernelGGL(guided_nomatch_kernel, dim3((max_nq_empty + 255u) / 256u, (unsigned)n), dim3(256), 0, st, list);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { ctx->partial_dirty = true; return fail(ctx, CLC_ERR_HIP, who, e); }
    return CLC_OK;
}

// the arguments of one job, checked; its two sides into `pd`
int guided_inputs(clc_ctx* ctx, const clc_guided_job& job, PairJobDev& pd)
{
    const auto bad = [&](const char* what) { return fail(ctx, CLC_ERR_BAD_ARG, what); };
    if (job.nq < 0 || job.nt < 0 || (job.nq > 0 && (!job.d_q || !job.d_match)) || (job.nt > 0 && !job.d_t)) return bad("match_guided: negative count / null block");
    if (((uintptr_t)job.d_q & 15u) || ((uintptr_t)job.d_t & 15u)) return bad("match_guided: descriptor rows must be 16-byte aligned");
    if (((uintptr_t)job.d_match & 3u) || ((uintptr_t)job.d_best & 1u) || ((uintptr_t)job.d_second & 1u) || ((uintptr_t)job.d_line & 3u) ||
        ((uintptr_t)job.d_tpos & 3u))
        return bad("match_guided: misaligned device pointer");
    if (!(job.band > 0.f) || !std::isfinite(job.band)) return bad("match_guided: band must be finite and positive");
    pd = PairJobDev{};                                                                  // the sides' rules are the pair kernel's
    int rc = gather_side(ctx, "match_guided", job.d_count_a, job.d_kps_a, job.d_feat_a, job.feat_stride_a, job.cam_a, pd.a);
    if (rc == CLC_OK) rc = gather_side(ctx, "match_guided", job.d_count_b, job.d_kps_b, job.d_feat_b, job.feat_stride_b, job.cam_b, pd.b);
    if (rc != CLC_OK) return rc;
    if ((uint32_t)job.nt > kIdxMask + 1u) return fail(ctx, CLC_ERR_CAPACITY, "match_guided: more than 2^22 train rows");
    return CLC_OK;
}

int guided_batch(clc_ctx* ctx, const clc_guided_job* jobs, const int n_jobs, void* stream)
{
    if (!ctx || n_jobs < 0 || n_jobs > kGuidedMaxJobs || (n_jobs > 0 && !jobs)) return fail(ctx, CLC_ERR_BAD_ARG, "match_guided: null context / jobs, or a job count outside 0 .. CLC_MAX_TRACK_PAIRS");
    if (!ctx->has_mat) return fail(ctx, CLC_ERR_STATE, "match_guided: context created without matcher options");
    // everything is checked before anything is enqueued
    std::vector<PairJobDev> sides((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int rc = guided_inputs(ctx, jobs[j], sides[(size_t)j]);
        if (rc != CLC_OK) return rc;
    }
    std::vector<int> live;                                                   // a job without query rows has nothing to answer
    for (int j = 0; j < n_jobs; ++j) if (jobs[j].nq > 0) live.push_back(j);
    if (live.empty()) return CLC_OK;
    const int n = (int)live.size();
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);

    std::vector<K2nnJobDev> kj((size_t)n);
    for (int k = 0; k < n; ++k) { kj[(size_t)k] = K2nnJobDev{}; kj[(size_t)k].nq = (uint32_t)jobs[live[(size_t)k]].nq; kj[(size_t)k].nt = (uint32_t)jobs[live[(size_t)k]].nt; }
    GuidedJobList list{};
    const int rc = guided_plan(ctx, "match_guided: more than 2^22 train rows", kj, LineGate::kF, st, list);
    if (rc != CLC_OK) return rc;
    for (int k = 0; k < n; ++k) {
        const clc_guided_job& job = jobs[live[(size_t)k]];
        const PairJobDev& pd = sides[(size_t)live[(size_t)k]];
        GuidedJobDev& g = list.j[k];
        g.q = (const uint4*)job.d_q; g.t = (const uint4*)job.d_t;
        g.out = job.d_match; g.best_out = job.d_best; g.second_out = job.d_second;
        g.cnt_q = pd.a.count; g.cnt_t = pd.b.count;
        g.thr = (uint32_t)(uint8_t)job.threshold;                                       // CUDAK2NN.cu:46: the kernel parameter is uint8_t
        g.band = job.band;
    }

    for (int base = 0; base < n; base += kGuidedPrepJobs) {
        const int cnt = std::min(kGuidedPrepJobs, n - base);
        GuidedPrepList prep{};
        level_scales(prep.scale);
        uint32_t rows = 0;
        for (int k = 0; k < cnt; ++k) {
            const clc_guided_job& job = jobs[live[(size_t)(base + k)]];
            const PairJobDev& pd = sides[(size_t)live[(size_t)(base + k)]];
            GuidedPrepJob& pj = prep.j[k];
            pj.a = pd.a; pj.b = pd.b;
            for (int i = 0; i < 9; ++i) pj.F[i] = job.F[i];
            pj.nq = (uint32_t)job.nq; pj.nt = (uint32_t)job.nt;
            pj.L = const_cast<float*>(list.j[base + k].L); pj.pos = const_cast<float*>(list.j[base + k].pos);
            pj.line_out = job.d_line; pj.tpos_out = job.d_tpos;
            rows = std::max(rows, pj.nq + pj.nt);
        }
        hipLaunchKernelGGL(guided_prep_kernel, dim3((rows + 255u) / 256u, (unsigned)cnt), dim3(256), 0, st, prep);
    }
    return guided_sweep<LineGate>(ctx, "match_guided: launch", hipGetLastError(), list, n, st);
}

} // namespace

// ---- the map match guided by a predicted pose (declared in k2nn_proj.h: k2nn_binned.hip runs the same checks and the same prep) ----------
// the arguments of one job, checked; its 2-D side into `side`
static int proj_inputs(clc_ctx* ctx, const clc_map_guided_job& job, GatherSide& side)
{
    const auto bad = [&](const char* what) { return fail(ctx, CLC_ERR_BAD_ARG, what); };
    if (job.nq < 0 || (job.nq > 0 && (!job.d_q || !job.d_match))) return bad("match_map_guided: negative count / null block");
    if ((uintptr_t)job.d_q & 15u) return bad("match_map_guided: descriptor rows must be 16-byte aligned");
    if (((uintptr_t)job.d_match & 3u) || ((uintptr_t)job.d_best & 1u) || ((uintptr_t)job.d_second & 1u) || ((uintptr_t)job.d_qpos & 3u) ||
        ((uintptr_t)job.d_proj & 3u))
        return bad("match_map_guided: misaligned device pointer");
    const float r2 = job.radius * job.radius;                                          // the gate's limit, formed once, in float
    if (!(job.radius > 0.f) || !std::isfinite(job.radius) || !(r2 > 0.f) || !std::isfinite(r2))
        return bad("match_map_guided: radius and its square must be finite and positive");
    for (int i = 0; i < 12; ++i) if (!std::isfinite(job.Rt[i])) return bad("match_map_guided: Rt is not finite");
    return gather_side(ctx, "match_map_guided", job.d_count, job.d_kps, job.d_feat, job.feat_stride, job.cam, side);      // the gathers' rules
}

int proj_checks(clc_ctx* ctx, const clc_map_guided_job* jobs, const int n_jobs, std::vector<GatherSide>& sides)
{
    if (!ctx || n_jobs < 0 || n_jobs > kMaxBatch || (n_jobs > 0 && !jobs)) return fail(ctx, CLC_ERR_BAD_ARG, "match_map_guided: null context / jobs, or a job count outside 0 .. CLC_MAX_BATCH");
    if (!ctx->has_mat) return fail(ctx, CLC_ERR_STATE, "match_map_guided: context created without matcher options");
    if (ctx->map_n < 0) return fail(ctx, CLC_ERR_STATE, "match_map_guided before set_map");
    if (ctx->map_n > 0 && ctx->map_X_n < ctx->map_n)
        return fail(ctx, CLC_ERR_STATE, "match_map_guided: fewer map points (set_map_points) than map descriptors (set_map)");
    // everything is checked before anything is enqueued
    sides.assign((size_t)n_jobs, GatherSide{});
    for (int j = 0; j < n_jobs; ++j) {
        const int rc = proj_inputs(ctx, jobs[j], sides[(size_t)j]);
        if (rc != CLC_OK) return rc;
    }
    if ((uint32_t)ctx->map_n > kIdxMask + 1u) return fail(ctx, CLC_ERR_CAPACITY, "match_map_guided: more than 2^22 map rows");
    return CLC_OK;
}

hipError_t proj_prep_launch(const ProjPrepList& prep, const uint32_t rows, const int n, hipStream_t st)
{
    hipLaunchKernelGGL(proj_prep_kernel, dim3((rows + 255u) / 256u, (unsigned)n), dim3(256), 0, st, prep);
    return hipGetLastError();
}

int proj_batch(clc_ctx* ctx, const clc_map_guided_job* jobs, const int n_jobs, void* stream)
{
    std::vector<GatherSide> sides;
    const int checked = proj_checks(ctx, jobs, n_jobs, sides);
    if (checked != CLC_OK) return checked;
    std::vector<int> live;                                                  // a job without query rows has nothing to answer
    for (int j = 0; j < n_jobs; ++j) if (jobs[j].nq > 0) live.push_back(j);
    if (live.empty()) return CLC_OK;
    const int n = (int)live.size();
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = pick(ctx, stream);

    const uint32_t nm = (uint32_t)ctx->map_n;
    std::vector<K2nnJobDev> kj((size_t)n);
    for (int k = 0; k < n; ++k) { kj[(size_t)k] = K2nnJobDev{}; kj[(size_t)k].nq = (uint32_t)jobs[live[(size_t)k]].nq; kj[(size_t)k].nt = nm; }
    GuidedJobList list{};
    const int rc = guided_plan(ctx, "match_map_guided: more than 2^22 map rows", kj, PointGate::kF, st, list);
    if (rc != CLC_OK) return rc;

    ProjPrepList prep{};
    level_scales(prep.scale);
    prep.map_X = ctx->d_map_X.as<double>(); prep.nm = nm;
    uint32_t rows = 0;
    for (int k = 0; k < n; ++k) {
        const clc_map_guided_job& job = jobs[live[(size_t)k]];
        GuidedJobDev& g = list.j[k];
        g.q = (const uint4*)job.d_q; g.t = ctx->d_m.as<uint4>();
        g.out = job.d_match; g.best_out = job.d_best; g.second_out = job.d_second;
        g.cnt_q = sides[(size_t)live[(size_t)k]].count; g.cnt_t = nullptr;
        g.thr = (uint32_t)(uint8_t)job.threshold;                                       // CUDAK2NN.cu:46: the kernel parameter is uint8_t
        g.band = job.radius * job.radius;
        ProjPrepJob& pj = prep.j[k];
        pj.a = sides[(size_t)live[(size_t)k]];
        for (int i = 0; i < 12; ++i) pj.Rt[i] = job.Rt[i];
        pj.nq = g.nq;
        pj.qpos = const_cast<float*>(g.L); pj.proj = const_cast<float*>(g.pos);
        pj.qpos_out = job.d_qpos; pj.proj_out = job.d_proj;
        rows = std::max(rows, pj.nq + nm);
    }
    return guided_sweep<PointGate>(ctx, "match_map_guided: launch", proj_prep_launch(prep, rows, n, st), list, n, st);
}

} // namespace clc

using namespace clc;

extern "C" {

int clc_match_guided_dev(clc_ctx* ctx, const clc_guided_job* job, void* stream)
{
    if (!job) return fail(ctx, CLC_ERR_BAD_ARG, "match_guided: null job");
    return guided_batch(ctx, job, 1, stream);
}

int clc_match_guided_batch_dev(clc_ctx* ctx, const clc_guided_job* jobs, int n_jobs, void* stream)
{
    return guided_batch(ctx, jobs, n_jobs, stream);
}

int clc_match_map_guided_dev(clc_ctx* ctx, const clc_map_guided_job* job, void* stream)
{
    if (!job) return fail(ctx, CLC_ERR_BAD_ARG, "match_map_guided: null job");
    return proj_batch(ctx, job, 1, stream);
}

int clc_match_map_guided_batch_dev(clc_ctx* ctx, const clc_map_guided_job* jobs, int n_jobs, void* stream)
{
    return proj_batch(ctx, jobs, n_jobs, stream);
}

} // extern "C"

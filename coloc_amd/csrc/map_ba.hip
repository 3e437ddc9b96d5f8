// map_ba.hip -- the grown map bundle-adjusted on the device (include/coloc_hip.h: clc_ba_dev, clc_map_build_grow_ba_dev, and
// through map_build.hip's map_init_batch the _grow_ba_ and _sim_ batch entries): `refiner.refinePose(*scene, ba_refine_options, rmse, cov)` at the end of
// Reconstructor::reconstructScene (reference include/coloc/Reconstructor.hpp:160-161, Refiner.hpp:47-239) -- every valid camera's pose
// and every landmark under a Huber loss, by Levenberg-Marquardt through the Schur complement on the landmarks.  The arithmetic of a point
// and of an entry of the reduced system is ba_math.h's, host + device; here are the launches.  All enqueue-only on one stream; no kernel
// holds a lock or waits for another workgroup; a kernel that finds the run ended returns at once.
//   ba_pixels_kernel   (a composition only) one thread per (track, camera): the undistorted pixel of the track's row -> x[t][c]
//   ba_init_kernel     ONE workgroup: the cameras' [angle-axis | t], R, dR/dw; the ordered compaction (wg_compact.h) of the points with
//                      an observation that counts -> idx / bits; the Levenberg-Marquardt state
//   one iteration:
//   ba_build_kernel    one thread per listed point: residuals, Jacobians, weights -> the observations' records; (V + lambda diag V)^-1
//                      and that times g_t -> the point's record
//   ba_reduce_kernel   grid (entries, chunks of kBaChunk points): one thread per entry of the reduced system adds the chunk's points in
//                      order -> part[chunk][entry]
//   ba_solve_kernel    ONE workgroup: the chunks' sums in ascending order, the gradient test, the damped 48 x 48 Cholesky in LDS (the
//                      rows of a column side by side, each entry ba_chol_sum's), the cameras' step and trial poses
//   ba_try_kernel      one thread per listed point: d_X by back-substitution, the trial point, its cost; per chunk, summed in order, the
//                      cost, |d_X|^2 and |X|^2
//   ba_accept_kernel   ONE workgroup: the chunks' sums in order, accept or reject (ba_lm_trial), the committed points and cameras, lambda;
//                      the last of a round writes the pinned record and releases its word behind a system-scope fence
// The start is evaluated by init, try, accept with `initial` set.  Every sum over points runs over the compacted list, so its order is
// a function of the points' indices alone and a point without an observation changes nothing.  fp64 and latency-bound: a few thousand
// points, at most 8 cameras; nothing here is tuned and nothing is claimed of its speed.
#include "clc_ctx.h"
#include "ba_math.h"
#include "ud_pixel.h"
#include "wg_compact.h"

#include <algorithm>
#include <cmath>

namespace clc {

namespace {

constexpr int kOneGroup = 1024;
constexpr int kWide = 256;
constexpr int kSolveThreads = 256;
constexpr int kBaEntriesMax = ba_entries(kBaDim);      // a chunk's stride in `part`
constexpr int kRoundIterations = 4;                    // iterations the host enqueues between two looks at the record

// the pinned record: everything the host needs of a run, `ready` released last
struct BaRecord {
    double cost_initial, cost, lambda;
    double Rt[kBaCams][12];
    int32_t status, iterations, n_obs, n_points, n_accepted, n_slots;
    uint32_t ready;
};

struct BaState {
    BaCams cur, trial;
    BaLm lm;
    double dc[kBaDim];               // the cameras' step, slot-major
    double dn_c, pn_c;               // its squared norm, the camera parameters'
    int32_t n_pts, n_obs;            // listed points, observations that count
    int32_t initial, skip;           // the start is being evaluated / this iteration's factorisation failed: nothing to try
    int32_t cam_of_slot[kBaCams];
};

struct BaInit { double K[kBaCams][3], Rt[kBaCams][12]; uint32_t mask; int32_t max_it; double ftol; };

// what every launch works on
struct BaJob {
    BaState* st;
    double* X; const uint32_t* obs; const double* x;
    int32_t n_points, n_cams;
    int32_t* idx; uint32_t* bits;                      // the list: point index, observation bits that count
    double* rec; double* pt; double* flag;             // per listed point: n_cams x kBaRec | kBaPoint | { failed, largest |g_t| }
    double* X_try; double* part; double* tpart;        // 3 per listed point | [chunk][kBaEntriesMax] | [chunk][4]
    double a;
    BaRecord* h_rec;
};

struct Scales { float v[CLC_MAX_LEVELS]; };

__device__ __forceinline__ bool running(const BaState* st) { return st->lm.status == BA_RUNNING; }

__global__ __launch_bounds__(kWide) void ba_pixels_kernel(const GrowCams cams, const int32_t* __restrict__ table, const int32_t n_points, const int32_t n_cams,
                                                         double* __restrict__ x)
{
    const int32_t i = (int32_t)(blockIdx.x * kWide + threadIdx.x);
    if (i >= n_points * n_cams) return;
    const int32_t c = i % n_cams, r = table[i];
    double px[2] = { 0.0, 0.0 };
    if (r >= 0) {
        float fx, fy;
        feature_position(cams.side[c].kps, cams.side[c].feat, cams.side[c].feat_stride, (uint32_t)r, cams.scale, &fx, &fy);
        ud_pixel(fx, fy, cams.side[c].cam, px);
    }
    x[2 * (size_t)i] = px[0]; x[2 * (size_t)i + 1] = px[1];
}

__global__ __launch_bounds__(kOneGroup) void ba_init_kernel(const BaJob job, const BaInit in)
{
    __shared__ uint32_t s_wave[kOneGroup / 64];
    __shared__ int s_obs;
    BaState* st = job.st;
    if (threadIdx.x == 0) {
        s_obs = 0;
        BaCams& cams = st->cur;
        cams.n_cams = job.n_cams; cams.n_slots = 0;
        for (int c = 0; c < kBaCams; ++c) {
            cams.slot[c] = -1;
            for (int i = 0; i < 3; ++i) cams.K[c][i] = c < job.n_cams ? in.K[c][i] : 0.0;
            if (c >= job.n_cams || !((in.mask >> c) & 1u)) continue;
            st->cam_of_slot[cams.n_slots] = c;
            cams.slot[c] = cams.n_slots++;
            ba_camera_from_Rt(in.Rt[c], cams.par[c]);
            ba_camera_update(cams, c);
        }
    }
    __syncthreads();
    uint32_t base = 0;
    int n_obs = 0;
    for (int32_t t0 = 0; t0 < job.n_points; t0 += kOneGroup) {
        const int32_t t = t0 + (int32_t)threadIdx.x;
        const uint32_t bits = t < job.n_points ? ba_obs_bits(st->cur, job.obs[t]) : 0u;
        uint32_t total;
        const uint32_t k = base + ordered_slot<kOneGroup>(bits != 0u, s_wave, &total);
        if (bits != 0u) { job.idx[k] = t; job.bits[k] = bits; n_obs += __popc(bits); }      // (k < n_points: at most one entry per point)
        base += total;
    }
    if (n_obs) atomicAdd(&s_obs, n_obs);                 // (an integer count: the order does not matter)
    __syncthreads();
    if (threadIdx.x == 0) {
        st->n_pts = (int32_t)base; st->n_obs = s_obs;
        st->lm.lambda = kBaLambda0; st->lm.cost = 0.0; st->lm.cost_initial = 0.0; st->lm.it = 0; st->lm.max_it = in.max_it;
        st->lm.status = BA_RUNNING; st->lm.n_accepted = 0; st->lm.ftol = in.ftol;
        st->initial = 1; st->skip = 0; st->dn_c = 0.0; st->pn_c = 0.0;
        st->trial = st->cur;
    }
}

__global__ __launch_bounds__(kBaChunk) void ba_build_kernel(const BaJob job)
{
    const BaState* st = job.st;
    if (!running(st)) return;
    const int32_t k = (int32_t)(blockIdx.x * kBaChunk + threadIdx.x);
    if (k >= st->n_pts) return;
    const int32_t t = job.idx[k];
    double g = 0.0;
    const bool ok = ba_point_build(st->cur, job.bits[k], job.X + 3 * (size_t)t, job.x + 2 * (size_t)job.n_cams * t, job.a, st->lm.lambda,
                                   job.rec + (size_t)k * job.n_cams * kBaRec, job.pt + (size_t)k * kBaPoint, &g);
    job.flag[2 * (size_t)k] = ok ? 0.0 : 1.0;
    job.flag[2 * (size_t)k + 1] = g;
}

__global__ __launch_bounds__(kWide) void ba_reduce_kernel(const BaJob job)
{
    const BaState* st = job.st;
    if (!running(st)) return;
    const int32_t k0 = (int32_t)blockIdx.y * kBaChunk;
    if (k0 >= st->n_pts) return;
    const int32_t k1 = min(st->n_pts, k0 + kBaChunk);
    const int n = 6 * st->cur.n_slots, E = ba_entries(n), e = (int)(blockIdx.x * kWide + threadIdx.x);
    if (e >= E) return;
    double acc = 0.0;
    if (e < E - 2) {
        const BaEntry en = ba_entry(n, e, st->cam_of_slot);
        for (int32_t k = k0; k < k1; ++k) acc += ba_entry_term(en, job.bits[k], job.rec + (size_t)k * job.n_cams * kBaRec, job.pt + (size_t)k * kBaPoint);
    } else if (e == E - 2) {
        for (int32_t k = k0; k < k1; ++k) acc += job.flag[2 * (size_t)k];
    } else {
        for (int32_t k = k0; k < k1; ++k) acc = fmax(acc, job.flag[2 * (size_t)k + 1]);
    }
    job.part[(size_t)blockIdx.y * kBaEntriesMax + e] = acc;
}

__global__ __launch_bounds__(kSolveThreads) void ba_solve_kernel(const BaJob job)
{
    __shared__ double s_sys[kBaEntriesMax];
    __shared__ double s_S[kBaDim * kBaDim];
    __shared__ int s_go;
    BaState* st = job.st;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_go = ba_lm_may_step(st->lm) ? 1 : 0;
    __syncthreads();
    if (!s_go) return;
    const int n = 6 * st->cur.n_slots, E = ba_entries(n), tri = ba_tri(n);
    const int chunks = (st->n_pts + kBaChunk - 1) / kBaChunk;
    for (int e = tid; e < E; e += kSolveThreads) {
        double v = 0.0;
        if (e == E - 1) for (int c = 0; c < chunks; ++c) v = fmax(v, job.part[(size_t)c * kBaEntriesMax + e]);
        else for (int c = 0; c < chunks; ++c) v += job.part[(size_t)c * kBaEntriesMax + e];
        s_sys[e] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double gmax = s_sys[E - 1];
        for (int a = 0; a < n; ++a) gmax = fmax(gmax, fabs(s_sys[tri + 2 * n + a]));
        st->skip = 0;
        if (ba_lm_gradient_small(st->lm, gmax)) { st->lm.status = BA_OK; s_go = 0; }
        else if (s_sys[E - 2] > 0.0) { ba_lm_failed(st->lm); st->skip = 1; s_go = 0; }
    }
    __syncthreads();
    if (!s_go) return;
    const double lambda = st->lm.lambda;
    for (int i = tid; i < n * n; i += kSolveThreads) {
        const int b = i / n, a = i - b * n;
        if (a > b) continue;
        double v = s_sys[ba_tri_index(n, a, b)];
        if (a == b) { const double u = s_sys[tri + n + a]; v += lambda * (u > 1e-12 ? u : 1e-12); }
        s_S[b * kBaDim + a] = v;
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        if (tid == 0) {
            const double p = ba_chol_pivot(ba_chol_sum(s_S, j, j), s_S[j * kBaDim + j]);
            s_S[j * kBaDim + j] = p;
            if (p == 0.0) s_go = 0;
        }
        __syncthreads();
        if (!s_go) break;
        const int i = j + 1 + tid;
        if (i < n) s_S[i * kBaDim + j] = ba_chol_sum(s_S, i, j) / s_S[j * kBaDim + j];
        __syncthreads();
    }
    if (tid != 0) return;
    if (!s_go) { ba_lm_failed(st->lm); st->skip = 1; return; }
    ba_chol_substitute(s_S, n, s_sys + tri, st->dc);
    double dn = 0.0, pn = 0.0;
    for (int c = 0; c < st->cur.n_cams; ++c) {
        const int s = st->cur.slot[c];
        if (s < 0) continue;
        for (int i = 0; i < 6; ++i) {
            const double d = st->dc[6 * s + i], p = st->cur.par[c][i];
            dn += d * d; pn += p * p;
            st->trial.par[c][i] = p + d;
        }
        ba_camera_update(st->trial, c);
    }
    st->dn_c = dn; st->pn_c = pn;
}

__global__ __launch_bounds__(kBaChunk) void ba_try_kernel(const BaJob job)
{
    __shared__ double s_v[3][kBaChunk];
    const BaState* st = job.st;
    if (!running(st) || st->skip) return;
    const int32_t k0 = (int32_t)blockIdx.x * kBaChunk, k = k0 + (int32_t)threadIdx.x;
    if (k0 >= st->n_pts) return;
    double cost = 0.0, dd = 0.0, pp = 0.0;
    if (k < st->n_pts) {
        const int32_t t = job.idx[k];
        const double* X = job.X + 3 * (size_t)t;
        double Xt[3] = { X[0], X[1], X[2] };
        if (!st->initial) {
            double d[3];
            ba_point_delta(st->cur, job.bits[k], job.rec + (size_t)k * job.n_cams * kBaRec, job.pt + (size_t)k * kBaPoint, st->dc, d);
            for (int i = 0; i < 3; ++i) Xt[i] = X[i] + d[i];
            dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            pp = (X[0] * X[0] + X[1] * X[1]) + X[2] * X[2];
        }
        double* o = job.X_try + 3 * (size_t)k;
        o[0] = Xt[0]; o[1] = Xt[1]; o[2] = Xt[2];
        cost = ba_point_cost(st->trial, job.bits[k], Xt, job.x + 2 * (size_t)job.n_cams * t, job.a);
    }
    s_v[0][threadIdx.x] = cost; s_v[1][threadIdx.x] = dd; s_v[2][threadIdx.x] = pp;
    __syncthreads();
    if (threadIdx.x < 3) {
        const int32_t m = min(st->n_pts - k0, kBaChunk);
        double v = 0.0;
        for (int32_t i = 0; i < m; ++i) v += s_v[threadIdx.x][i];                // in the list's order
        job.tpart[4 * (size_t)blockIdx.x + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(kOneGroup) void ba_accept_kernel(const BaJob job, const int32_t publish)
{
    __shared__ double s_tot[3];
    __shared__ int s_mode;           // 0: nothing to do, 1: a trial (or the start) to judge, 2: commit
    BaState* st = job.st;
    const int tid = (int)threadIdx.x;
    if (tid == 0) {
        s_mode = running(st) && !st->skip ? 1 : 0;
        if (running(st) && st->skip) st->skip = 0;
    }
    __syncthreads();
    if (s_mode == 1) {
        const int chunks = (st->n_pts + kBaChunk - 1) / kBaChunk;
        if (tid < 3) {
            double v = 0.0;
            for (int c = 0; c < chunks; ++c) v += job.tpart[4 * (size_t)c + tid];
            s_tot[tid] = v;
        }
        __syncthreads();
        if (tid == 0) {
            if (st->initial) {
                st->initial = 0;
                st->lm.cost = s_tot[0]; st->lm.cost_initial = s_tot[0];
                if (st->n_obs == 0) st->lm.status = BA_EMPTY;
                else if (!isfinite(s_tot[0])) st->lm.status = BA_BAD_START;
            } else if (ba_lm_trial(st->lm, s_tot[0], st->dn_c + s_tot[1], st->pn_c + s_tot[2])) s_mode = 2;
        }
        __syncthreads();
        if (s_mode == 2) {
            for (int32_t i = tid; i < 3 * st->n_pts; i += kOneGroup) job.X[3 * (size_t)job.idx[i / 3] + i % 3] = job.X_try[i];
            if (tid < st->cur.n_cams && st->cur.slot[tid] >= 0) {
                for (int i = 0; i < 6; ++i) st->cur.par[tid][i] = st->trial.par[tid][i];
                for (int i = 0; i < 9; ++i) st->cur.R[tid][i] = st->trial.R[tid][i];
                for (int i = 0; i < 27; ++i) st->cur.dR[tid][i / 9][i % 9] = st->trial.dR[tid][i / 9][i % 9];
            }
        }
    }
    if (!publish) return;
    __syncthreads();
    BaRecord* r = job.h_rec;
    if (tid < st->cur.n_cams && st->cur.slot[tid] >= 0) ba_camera_to_Rt(st->cur.R[tid], st->cur.par[tid], r->Rt[tid]);
    if (tid == 0) {
        r->cost_initial = st->lm.cost_initial; r->cost = st->lm.cost; r->lambda = st->lm.lambda;
        r->status = st->lm.status; r->iterations = st->lm.it; r->n_obs = st->n_obs; r->n_points = st->n_pts; r->n_accepted = st->lm.n_accepted;
        r->n_slots = st->cur.n_slots;
    }
    // the word comes out last: the record is complete and visible system-wide before the word the host polls changes
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(&r->ready, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

} // namespace

int ba_check(clc_ctx* ctx, clc_map_ba* ba, const char* who)
{
    if (!ba) return fail(ctx, CLC_ERR_BAD_ARG, (std::string(who) + ": null ba").c_str());
    ba->status = CLC_BA_EMPTY; ba->iterations = 0; ba->n_cams = 0; ba->n_points = 0; ba->n_obs = 0;
    ba->cost_initial = 0.0; ba->cost_final = 0.0; ba->rmse = 0.0;
    if (ba->max_iterations < 0 || !(ba->function_tolerance >= 0.0))
        return fail(ctx, CLC_ERR_BAD_ARG, (std::string(who) + ": negative max_iterations / function_tolerance").c_str());
    return CLC_OK;
}

int ba_drive(clc_ctx* ctx, BaProblem& pb, clc_map_ba& ba)
{
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t P = (size_t)std::max(pb.n_points, 1), C = (size_t)pb.n_cams, chunks = (P + kBaChunk - 1) / kBaChunk;
    const BaDims dims{ sizeof(BaState), P, C, chunks, (size_t)kBaRec, (size_t)kBaPoint, (size_t)kBaEntriesMax, pb.x == nullptr };
    BaDev dv; BaPin pin;
    int rc = carve_block(ctx, ctx->d_bab, 1, 4, true, "growing the bundle adjustment block", [&](Carve& c) { dv.carve(c, dims); });
    if (rc == CLC_OK) rc = carve_block(ctx, ctx->h_bab, 0, 1, true, "allocating the bundle adjustment record", [&](Carve& c) { pin.carve(c, sizeof(BaRecord)); });
    if (rc != CLC_OK) return rc;
    BaJob job{};
    job.st = (BaState*)dv.state;
    job.X = pb.X; job.obs = pb.obs; job.x = pb.x ? pb.x : dv.x;
    job.n_points = pb.n_points; job.n_cams = pb.n_cams;
    job.idx = dv.idx; job.bits = dv.bits;
    job.rec = dv.rec; job.pt = dv.pt; job.flag = dv.flag;
    job.X_try = dv.X_try; job.part = dv.part; job.tpart = dv.tpart;
    job.a = ba.huber_a > 0.0 ? ba.huber_a : 16.0;
    job.h_rec = (BaRecord*)pin.rec;
    BaInit in{};
    memcpy(in.K, pb.K, sizeof in.K); memcpy(in.Rt, pb.Rt, sizeof in.Rt);
    in.mask = pb.mask; in.max_it = ba.max_iterations > 0 ? ba.max_iterations : 500; in.ftol = ba.function_tolerance > 0.0 ? ba.function_tolerance : 1e-8;
    const dim3 per_point((unsigned)chunks), one(1);
    const dim3 reduce_grid((unsigned)((kBaEntriesMax + kWide - 1) / kWide), (unsigned)chunks);
    const auto failed = [&](const char* what, hipError_t e) { (void)hipStreamSynchronize(st); return fail(ctx, CLC_ERR_HIP, what, e); };
    if (!pb.x && pb.n_points > 0) {
        const unsigned cells = (unsigned)(P * C);
        hipLaunchKernelGGL(ba_pixels_kernel, dim3((cells + kWide - 1) / kWide), dim3(kWide), 0, st, *pb.cams, pb.table, (int32_t)pb.n_points, (int32_t)pb.n_cams,
                           dv.x);
    }
    // the start: init, try, accept -- and the first look at the record
    __atomic_store_n(&job.h_rec->ready, 0u, __ATOMIC_RELAXED);
    hipLaunchKernelGGL(ba_init_kernel, one, dim3(kOneGroup), 0, st, job, in);
    hipLaunchKernelGGL(ba_try_kernel, per_point, dim3(kBaChunk), 0, st, job);
    hipLaunchKernelGGL(ba_accept_kernel, one, dim3(kOneGroup), 0, st, job, (int32_t)1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return failed("map_ba: the start's launches", e);
    rc = wait_pinned(ctx, &job.h_rec->ready, 0u, st, std::chrono::steady_clock::now(), 5, "map_ba: the start left no record");
    if (rc != CLC_OK) return rc;
    // rounds of kRoundIterations iterations; every iteration either counts or ends the run, so max_it + 1 of them always suffice
    const int rounds = in.max_it / kRoundIterations + 2;
    for (int r = 0; r < rounds && job.h_rec->status == BA_RUNNING; ++r) {
        __atomic_store_n(&job.h_rec->ready, 0u, __ATOMIC_RELAXED);
        for (int i = 0; i < kRoundIterations; ++i) {
            hipLaunchKernelGGL(ba_build_kernel, per_point, dim3(kBaChunk), 0, st, job);
            hipLaunchKernelGGL(ba_reduce_kernel, reduce_grid, dim3(kWide), 0, st, job);
            hipLaunchKernelGGL(ba_solve_kernel, one, dim3(kSolveThreads), 0, st, job);
            hipLaunchKernelGGL(ba_try_kernel, per_point, dim3(kBaChunk), 0, st, job);
            hipLaunchKernelGGL(ba_accept_kernel, one, dim3(kOneGroup), 0, st, job, (int32_t)(i == kRoundIterations - 1));
        }
        e = hipGetLastError();
        if (e != hipSuccess) return failed("map_ba: a round's launches", e);
        rc = wait_pinned(ctx, &job.h_rec->ready, 0u, st, std::chrono::steady_clock::now(), 5, "map_ba: a round left no record");
        if (rc != CLC_OK) return rc;
    }
    const BaRecord& rec = *job.h_rec;
    if (rec.status == BA_RUNNING) return fail(ctx, CLC_ERR_HIP, "map_ba: the run did not end within its rounds");
    ba.status = rec.status; ba.iterations = rec.iterations; ba.n_cams = rec.n_slots; ba.n_points = rec.n_points; ba.n_obs = rec.n_obs;
    if (rec.status == CLC_BA_EMPTY || rec.status == CLC_BA_BAD_START) {
        ba.cost_initial = rec.status == CLC_BA_EMPTY ? 0.0 : rec.cost_initial; ba.cost_final = ba.cost_initial; ba.rmse = 0.0;
        return CLC_OK;
    }
    ba.cost_initial = rec.cost_initial; ba.cost_final = rec.cost;
    ba.rmse = rec.n_obs > 0 ? std::sqrt(rec.cost / (2.0 * rec.n_obs)) : 0.0;
    if (rec.n_accepted > 0)
        for (int c = 0; c < pb.n_cams; ++c)
            if ((pb.mask >> c) & 1u) memcpy(pb.Rt[c], rec.Rt[c], sizeof pb.Rt[c]);
    return CLC_OK;
}

} // namespace clc

using namespace clc;

extern "C" {

int clc_ba_dev(clc_ctx* ctx, clc_ba_job* job)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "ba: null context / job");
    int rc = ba_check(ctx, &job->ba, "ba");
    if (rc != CLC_OK) return rc;
    if (job->n_cams < 1 || job->n_cams > kMaxBatch) return fail(ctx, CLC_ERR_BAD_ARG, "ba: n_cams outside [1, CLC_MAX_BATCH]");
    if (job->n_points < 0) return fail(ctx, CLC_ERR_BAD_ARG, "ba: negative n_points");
    if (job->n_points > 0 && (!job->d_X || !job->d_obs || !job->d_x)) return fail(ctx, CLC_ERR_BAD_ARG, "ba: null array");
    if (((uintptr_t)job->d_X & 7u) || ((uintptr_t)job->d_obs & 3u) || ((uintptr_t)job->d_x & 7u)) return fail(ctx, CLC_ERR_BAD_ARG, "ba: misaligned device pointer");
    BaProblem pb{};
    pb.n_cams = job->n_cams; pb.n_points = job->n_points; pb.mask = job->cam_mask & ((1u << job->n_cams) - 1u);
    for (int c = 0; c < job->n_cams; ++c) {
        if (((pb.mask >> c) & 1u) && !(job->cam[c].focal > 0.0)) return fail(ctx, CLC_ERR_BAD_ARG, "ba: focal must be positive");
        pb.K[c][0] = job->cam[c].focal; pb.K[c][1] = job->cam[c].ppx; pb.K[c][2] = job->cam[c].ppy;
        memcpy(pb.Rt[c], job->Rt[c], sizeof pb.Rt[c]);
    }
    pb.X = job->d_X; pb.obs = job->d_obs; pb.x = job->d_x;
    static const double none[1] = { 0.0 };
    if (job->n_points == 0) pb.x = none;                 // (never read: no point is listed)
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hipStream_t prod = (hipStream_t)job->after_stream;
    if (prod && prod != st) CLC_HIP(ctx, order_behind(ctx->ev_track, prod, &st, 1));
    rc = ba_drive(ctx, pb, job->ba);
    if (rc != CLC_OK) return rc;
    for (int c = 0; c < job->n_cams; ++c) memcpy(job->Rt[c], pb.Rt[c], sizeof pb.Rt[c]);
    return CLC_OK;
}

int clc_map_build_grow_ba_dev(clc_ctx* ctx, clc_map_job* job, clc_map_grow* grow, clc_map_ba* ba)
{
    if (!ctx || !job || !grow || !ba) return fail(ctx, CLC_ERR_BAD_ARG, "map_build_grow_ba: null context / job / grow / ba");
    const int rc = ba_check(ctx, ba, "map_build_grow_ba");
    return rc == CLC_OK ? map_build_grow(ctx, *job, *grow, ba) : rc;
}

} // extern "C"

// pose_batch.hip -- the a-contrario robust solvers behind the C ABI (include/coloc_hip.h): what Localizer::localizeImage
// (reference include/coloc/Localizer.hpp:82-93, SfM_Localizer::Localize with error_max = +inf) and RobustMatcher::filterEssential
// (RobustMatcher.hpp:153-171, robust::ACRANSAC) run -- and, since round 6, filterFundamental / filterHomography (:128-151, :188-239) --,
// single solves and batches of them driven from one host thread.
#include "clc_ctx.h"
#include "clc_acr.h"
#include "twoview_min.h"
#include "sim3_math.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace clc;

// a switch over AcrKindId that lacks a kind does not compile (set_problem, after_rounds, model_out)
#pragma clang diagnostic error "-Wswitch"

namespace {

// log10 C(n, k) and log10 C(k, m), k = 0..n, as OpenMVG tabulates them: a FLOAT log10 table, float accumulation
// (logcombi<float>); the O(n^2) re-summation of the prefix is replaced by the running prefix -- same additions, same order.
// `lg` = the context's table of (float) log10(k), grown on demand and kept: it does not depend on n, and n + 1 calls of the
// portable log10 per solve were 40 us of a 220 us solve at n = 1000 (200 us at n = 5000).
void acr_tables(int n, int m, float* logc_n, float* logc_k, std::vector<float>& lg)
{
    if (lg.size() < (size_t)n + 2) {
        const size_t have = lg.size() < 1 ? 1 : lg.size();
        lg.resize((size_t)n + 2, 0.0f);
        lg[0] = 0.0f;
        for (size_t k = have; k < lg.size(); ++k) lg[k] = (float)clc_acr_log10((double)k);
    }
    std::vector<float> prefix((size_t)n + 1, 0.0f);
    for (int i = 1; i <= n; ++i) prefix[i] = prefix[i - 1] + (lg[n - i + 1] - lg[i]);
    for (int k = 0; k <= n; ++k) {
        uint32_t kk = (uint32_t)k;
        if (kk >= (uint32_t)n || kk == 0) { logc_n[k] = 0.0f; continue; }
        if ((uint32_t)n - kk < kk) kk = (uint32_t)n - kk;
        logc_n[k] = prefix[kk];
    }
    for (int nn = 0; nn <= n; ++nn) {
        uint32_t kk = (uint32_t)m;
        float r = 0.0f;
        if (!(kk >= (uint32_t)nn || kk == 0)) {
            if ((uint32_t)nn - kk < kk) kk = (uint32_t)nn - kk;
            for (uint32_t i = 1; i <= kk; ++i) r += lg[nn - i + 1] - lg[i];
        }
        logc_k[nn] = r;
    }
}

// The identity a similarity solve reports where it finds no model: s = 1, R = I, t = 0, A = [I | 0]
Sim3Out sim3_identity()
{
    Sim3Out o{};
    o.s = 1.0; o.R[0] = o.R[4] = o.R[8] = 1.0; o.A[0] = o.A[5] = o.A[10] = 1.0;
    return o;
}

// The Huber constant of the refinement behind a pose: the caller's, 16 where it names none; -1: no refinement
double refine_huber_of(const bool refine, const double huber_a) { return refine ? (huber_a > 0.0 ? huber_a : 16.0) : -1.0; }

// One a-contrario solve as a small state machine: begin() validates and prepares the inputs and the problem, poll() looks at the pinned
// progress word ONCE and reports whether the run needs another round -- or moves on to what runs behind the rounds, whose record it then
// polls the same way --, finish() copies the result out.  What goes into the stream of the solve's rounds is acr_drive's.
// kind: an AcrKindId.  What a | b hold and what the solve needs is its row of acr_kind() (acr_kind.h); begin / poll / finish hold what is
// the same for every kind, and what differs is ONE switch each, a case per kind and no default: set_problem() (alpha, norm, what the
// problem carries by value), after_rounds() (nothing, the pose refinement, the similarity's refit), model_out() (how the model leaves).
// h_model: 12 doubles [R|t] (resection), [sR|t] (similarity); 18 for the two-view kinds, the model matrix and then the fundamental matrix
// that goes with it: { E, F }, { F, F }, { H, zeros }, in pixels.
struct AcrRun {
    // arguments
    clc_ctx* ctx = nullptr;
    int kind = kAcrResection, N = 0, img_w = 0, img_h = 0, max_iteration = 0;
    const double *h_a = nullptr, *h_b = nullptr, *h_K1 = nullptr, *h_K2 = nullptr;
    // a | b from device memory: X | x of the track block (resection) or x1 | x2 in pixels of the pair block (two-view kinds) of gather.hip;
    // they are staged from these blocks -- conditioned by the staging launch where the kind is --, h_a / h_b unused
    const double *dev_a = nullptr, *dev_b = nullptr;
    uint64_t seed = 0;
    double precision = 0.0, refine_huber = -1.0;
    double* h_model = nullptr; uint8_t* h_mask = nullptr; int32_t* h_inliers = nullptr;
    int *n_inliers = nullptr, *iterations = nullptr, *rounds = nullptr;
    double *error_max = nullptr, *min_nfa = nullptr, *h_cov = nullptr, *rmse = nullptr;
    Sim3Out* sim = nullptr;           // similarity: the reported one (out); box: { min, max } of b where the points are the device's
    const double* box = nullptr;      // (dev_a / dev_b: read in place by the rounds and the refit, not staged)
    int* valid = nullptr;
    // state
    enum Phase { IDLE, ROUNDS, REFINE, DONE } phase = IDLE;
    int status = CLC_OK;
    bool refine = false;
    AcrProblem pb{};
    tv::Normalizer norm_t{};          // the conditioned kinds: the conditioning of both point sets
    hipStream_t st = nullptr;         // the stream of the solve's rounds (its group's: acr_drive)
    hipStream_t after_st = nullptr;   // the stream of what runs behind the rounds (after_rounds)
    int bound = 0, first_bound = 0, reserve0 = 0;
    uint32_t round = 0, spins = 0;
    std::chrono::steady_clock::time_point wait_start;
    bool reported = false;            // the round waited for has come out and the run needs another one (bound: its batch bound)
    const double* stage_src = nullptr; double* stage_dst = nullptr; size_t stage_n = 0;   // the inputs' way to the device (a launch, not a copy)
    int batch_cap = kAcrMaxBatch;      // most iterations a round evaluates (acr_drive)
    unsigned long long* h_word = nullptr;
    AcrResult* h_res = nullptr;
    int32_t* p_inl = nullptr;
    RefineOut* p_ref = nullptr;
    Sim3Out* p_sim = nullptr; Sim3Out* d_sim = nullptr;
    int32_t* ready = nullptr;         // what the REFINE phase polls: the flag of the record of what runs behind the rounds
    double *d_a = nullptr, *d_b = nullptr, *d_K1 = nullptr, *d_K2 = nullptr, *d_models = nullptr, *d_ref = nullptr;
    AcrState* d_state = nullptr; AcrHyp* d_hyp = nullptr;
    uint32_t *d_sorted = nullptr, *d_best = nullptr, *d_index = nullptr;
    AcrResult* d_res = nullptr; uint8_t* d_mask = nullptr;

    // Every failure after the first launch drains the stream first (ignoring what the drain reports): launches of the failed solve may
    // still be in flight and would otherwise write the progress word / result record of the NEXT solve, which reuses the same pinned block.
    int drained(const int code) { (void)hipStreamSynchronize(st); phase = DONE; status = code; return code; }
    int stop(const int code) { phase = DONE; status = code; return code; }

    // validates, lays out the workspace and the pinned block, prepares the inputs; enqueues nothing.  cap: most iterations a round
    // evaluates.  Returns a status; phase == DONE afterwards means there is nothing to wait for.
    int begin(const int cap)
    {
        if (!acr_is_kind(kind)) return stop(fail(ctx, CLC_ERR_BAD_ARG, "acransac: unknown model"));
        const AcrKindInfo k = acr_kind(kind);
        if (!ctx || N < 0 || max_iteration < 0 || (k.needs_K1 && !h_K1) || (k.needs_K2 && !h_K2) || (N > 0 && !(dev_a && dev_b) && (!h_a || !h_b)) ||
            ((dev_a || dev_b) && (!dev_a || !dev_b)) || (k.in_place && dev_a && !box))
            return stop(fail(ctx, CLC_ERR_BAD_ARG, "acransac: bad argument"));
        if (kind == kAcrResection && !pose_K_ok(h_K1)) return stop(fail(ctx, CLC_ERR_BAD_ARG, "acransac: K must be { fx, skew, cx; 0, fy, cy; 0, 0, 1 }"));
        if (n_inliers) *n_inliers = 0;
        if (error_max) *error_max = 0.0;
        if (min_nfa) *min_nfa = INFINITY;
        if (iterations) *iterations = 0;
        if (rounds) *rounds = 0;
        if (valid) *valid = -1;
        if (sim) *sim = sim3_identity();
        if (h_mask && N > 0) memset(h_mask, 0, (size_t)N);
        if (N <= k.m || max_iteration == 0) return stop(CLC_OK);                 // ACRANSAC: nData <= sizeSample -> (0, 0), no model
        if (N > kAcrMaxN) return stop(fail(ctx, CLC_ERR_CAPACITY, "acransac: more than 16384 correspondences per solve"));
        if (max_iteration > 500000) return stop(fail(ctx, CLC_ERR_CAPACITY, "acransac: more than 500000 iterations"));
        if (k.needs_image && (img_w <= 0 || img_h <= 0)) return stop(fail(ctx, CLC_ERR_BAD_ARG, "acransac: image size needed for the two-view models"));
        phase = DONE; status = CLC_ERR_HIP;                                     // (what an early CLC_HIP return leaves behind)
        batch_cap = cap;
        const int rc0 = begin_body(k);
        if (rc0 != CLC_OK) { phase = DONE; status = rc0; }
        return rc0;
    }

    // The part of the problem that differs by kind: logalpha0 and norm (mult is the table's), what the problem carries by value, the
    // conditioning.  From the image size, K1 and the box.  False: the kind admits no alpha here, hence no model.
    bool set_problem()
    {
        const double D = sqrt((double)img_w * (double)img_w + (double)img_h * (double)img_h), A = (double)img_w * (double)img_h;
        pb.mult = acr_kind(kind).mult;
        pb.norm = 1.0;
        switch ((AcrKindId)kind) {
        case kAcrResection:
            // ACKernelAdaptorResection_Intrinsics: residuals on the normalised camera plane (x 1 / focal), logalpha0 = log10(pi)
            pb.logalpha0 = clc_acr_log10(M_PI);
            pb.norm = 1.0 / h_K1[0];
            for (int e = 0; e < 9; ++e) pb.K1v[e] = h_K1[e];
            return true;
        case kAcrEssential:
            // ACKernelAdaptorEssential: point-to-line, logalpha0 = log10(2 D / A * 0.5) of image 2, error^(1/2)
            pb.logalpha0 = clc_acr_log10(2.0 * D / A * .5);
            return true;
        case kAcrFundamental:
            // ACKernelAdaptor on conditioned points (NormalizePoints(x, &x_, &N_, w, h), x_n = d x + t, for both point sets): point-to-line,
            // log10(2 D / A / N2(0,0)), error^(1/2); thresholds and the reported precision scale with N2(0,0) = d
            norm_t = tv::normalizer(img_w, img_h);
            pb.norm = norm_t.d;
            pb.logalpha0 = clc_acr_log10(2.0 * D / A / pb.norm);
            return true;
        case kAcrHomography:
            // as the fundamental, point-to-point: log10(pi / A / N2(0,0)^2)
            norm_t = tv::normalizer(img_w, img_h);
            pb.norm = norm_t.d;
            pb.logalpha0 = clc_acr_log10(M_PI / A / (pb.norm * pb.norm));
            return true;
        case kAcrSimilarity: {
            // a squared distance in old-map units against the box of the old points: log10(((4 / 3) pi) / V), error^(3/2); a flat or
            // unbounded box admits no alpha
            double bx[6];
            if (dev_a) memcpy(bx, box, sizeof bx);
            for (int q = 0; q < 3 && !dev_a; ++q) {
                bx[q] = bx[3 + q] = h_b[q];
                for (int i = 1; i < N; ++i) { const double v = h_b[3 * i + q]; bx[q] = v < bx[q] ? v : bx[q]; bx[3 + q] = v > bx[3 + q] ? v : bx[3 + q]; }
            }
            const double V = sim3_box_volume(bx);
            if (!sim3_volume_ok(V)) return false;
            pb.logalpha0 = clc_acr_log10(sim3_alpha0(V));
            return true;
        }
        case kAcrKindCount: break;
        }
        return false;
    }

    int begin_body(const AcrKindInfo& k)
    {
        CLC_HIP(ctx, hipSetDevice(ctx->device));
        refine = kind == kAcrResection && refine_huber > 0.0;
        pb = AcrProblem{};
        if (!set_problem()) return stop(CLC_OK);
        // the device workspace and the pinned block (AcrDev, AcrPin: the inputs, staged by one launch, lie alike in both).  A round's
        // launches read what the round before them wrote: two copies of state, models, slots and sorted lists, indexed by launch parity
        // (acransac.hip: acr_round_kernel, acr_solve5_kernel).  ref: the record of what after_rounds() launches
        const AcrDims dims{ kind, (size_t)N, sizeof(AcrState), sizeof(AcrHyp), sizeof(AcrResult),
                            kind == kAcrSimilarity ? sizeof(Sim3Out) : (refine ? sizeof(RefineOut) : 0), (size_t)kAcrMaxBatch, k.in_place && dev_a != nullptr };
        AcrDev dv; AcrPin pin;
        int rc = ensure_pnp(ctx, [&](Carve& c) { dv.carve(c, dims); });
        if (rc == CLC_OK) rc = ensure_pinned(ctx, [&](Carve& c) { pin.carve(c, dims); });
        if (rc != CLC_OK) return rc;
        d_a = dv.in.a; d_b = dv.in.b; d_K1 = dv.in.K1; d_K2 = dv.in.K2;
        if (dims.points_elsewhere) { d_a = const_cast<double*>(dev_a); d_b = const_cast<double*>(dev_b); }
        float* d_cn = dv.in.logc_n; float* d_ck = dv.in.logc_k;
        d_state = (AcrState*)dv.in.state; d_models = dv.models; d_hyp = (AcrHyp*)dv.hyp; d_sorted = dv.sorted; d_best = dv.best; d_index = dv.index;
        d_res = (AcrResult*)dv.result; d_mask = dv.mask; d_ref = dv.ref;
        double* hp = pin.in.a;
        if (!dev_a && k.conditioned) {
            // (points from device memory: the staging launch applies the same two operations, launch_acr_stage's cond)
            tv::condition(norm_t, h_a, N, pin.in.a);
            tv::condition(norm_t, h_b, N, pin.in.b);
        } else if (!dev_a) {
            memcpy(pin.in.a, h_a, sizeof(double) * k.a_width * N);
            memcpy(pin.in.b, h_b, sizeof(double) * k.b_width * N);
        }
        memset(pin.in.K1, 0, sizeof(double) * 32);                     // (K1 | K2)
        if (h_K1) memcpy(pin.in.K1, h_K1, sizeof(double) * 9);
        if (h_K2) memcpy(pin.in.K2, h_K2, sizeof(double) * 9);
        acr_tables(N, k.m, pin.in.logc_n, pin.in.logc_k, ctx->acr_lg);
        // the state ACRANSAC starts from is part of the upload (every round draws its own samples on the device)
        AcrState* h_states = (AcrState*)pin.in.state;
        memset(h_states, 0, 2 * sizeof(AcrState));
        // launch 0 (parity 0) reads copy 1
        AcrState* h_init = h_states + 1;
        h_init->min_nfa = INFINITY; h_init->error_max = INFINITY;
        h_init->best_iter = -1;
        h_init->reserve = max_iteration / 10;
        h_init->n_iter = max_iteration - h_init->reserve;
        h_init->n_index = N; h_init->index_all = 1;
        h_init->ac_mode = std::isinf(precision) ? 1 : 0;
        h_init->grow = batch_cap < 32 ? batch_cap : 32;
        h_init->cur_batch = h_init->n_iter < h_init->grow ? h_init->n_iter : h_init->grow;
        h_word = pin.word; h_res = (AcrResult*)pin.result; p_inl = pin.inliers; p_ref = pin.ref;
        p_sim = (Sim3Out*)pin.ref; d_sim = (Sim3Out*)dv.ref;
        __atomic_store_n(h_word, 0ull, __ATOMIC_RELAXED);

        pb.kind = kind; pb.n = N; pb.m = k.m; pb.max_models = k.M; pb.model_doubles = k.md; pb.batch_cap = batch_cap;
        pb.a = d_a; pb.b = d_b; pb.K1 = d_K1; pb.K2 = d_K2; pb.logc_n = d_cn; pb.logc_k = d_ck;
        pb.loge0 = clc_acr_log10((double)k.M * (double)(N - k.m));
        pb.max_threshold = std::isinf(precision) ? INFINITY : precision * (pb.norm * pb.norm);
        pb.seed = seed;

        stage_src = hp; stage_dst = dv.in.a; stage_n = (pin.in.bytes / sizeof(double) + 1) & ~(size_t)1;      // (both blocks go on past the inputs)
        // Upper bound of the batch a round can ask for, from what the host knows when it enqueues it (one or two rounds behind the
        // device): while the index set has not switched the batch doubles up to kAcrMaxBatch; afterwards it is what is left of the
        // reserve, remaining = n_iter - iter (+ a margin for the "no inliers: n_iter++" rule, once per round).
        reserve0 = h_init->reserve;
        bound = h_init->n_iter < batch_cap ? h_init->n_iter : batch_cap;
        first_bound = h_init->cur_batch;                               // (a replaying launch takes its first batch as it stands)
        round = 1;
        spins = 0;
        reported = false;
        wait_start = std::chrono::steady_clock::now();
        phase = ROUNDS;
        status = CLC_OK;
        return CLC_OK;
    }

    // this solve's part of a round's launch
    void chain(AcrChain& c) const
    {
        c.pb = pb;
        c.states = d_state; c.hyps = d_hyp; c.sorted = d_sorted; c.models = d_models; c.best_inliers = d_best; c.index_set = d_index;
        c.h_word = h_word;
        c.fin = AcrFinish{ d_mask, d_res, nullptr, p_inl, h_res };
    }
    // the next round is in the stream: wait for that round's word
    void advance()
    {
        ++round; spins = 0; reported = false;
        wait_start = std::chrono::steady_clock::now();
    }

    // What runs behind the rounds, behind the word that said "done": nothing (the solve has ended), or ONE launch whose pinned record sets
    // `ready` last -- the host polls that instead of synchronising after_st (~5 us), with the synchronisation as the fallback after 5 ms.
    int after_rounds()
    {
        hipError_t e = hipSuccess;
        const char* what = "";
        switch ((AcrKindId)kind) {
        case kAcrResection:
            if (!refine) { phase = DONE; return CLC_OK; }
            // The pose refinement, on the run's own context's stream: behind the launch that completed the run when the rounds ran there
            // (nothing is queued behind that launch any more: the word of the last round comes out of the last launch); a shared group's
            // stream still carries the other solves' rounds, and what the refinement reads was written before the word the host has just
            // seen -- system-scope release / acquire --, so the launch needs no ordering against it.
            ready = &p_ref->ready; after_st = ctx->stream; what = "launch_pnp_refine";
            __atomic_store_n(ready, 0, __ATOMIC_RELAXED);
            e = launch_pnp_refine((const double*)d_res /* AcrResult.model = [R|t] */, d_a, d_b, d_mask, N, d_K1, refine_huber, 50, d_ref, after_st,
                                  &ctx->prof, &d_res->valid, p_ref);
            break;
        case kAcrEssential:
        case kAcrFundamental:
        case kAcrHomography:
        case kAcrKindCount:             // (no kind: begin() has refused it)
            phase = DONE;
            return CLC_OK;
        case kAcrSimilarity:
            // the acceptance rule and the refit: one single-workgroup launch on the rounds' stream, behind the round enqueued ahead (it
            // reads the result record and the mask of the completing round, and uses the index set as its list)
            ready = &p_sim->ready; after_st = st; what = "launch_sim3_refit";
            __atomic_store_n(ready, 0, __ATOMIC_RELAXED);
            e = launch_sim3_refit(d_res, d_mask, d_a, d_b, N, (int32_t*)d_index, d_sim, p_sim, after_st);
            break;
        }
        if (e != hipSuccess) return drained(fail(ctx, CLC_ERR_HIP, what, e));
        spins = 0;
        wait_start = std::chrono::steady_clock::now();
        phase = REFINE;
        return CLC_OK;
    }

    // One look at the progress word / the ready flag of what runs behind the rounds; enqueues no round.  prof: where the end of the rounds
    // is marked (null: nowhere).  Returns the status; phase == DONE when the solve has ended.
    int poll(Profiler* prof)
    {
        if (phase == ROUNDS) {
            // the select kernel publishes one packed word (round number, iterations consumed, iter, n_iter) in pinned memory: poll it
            // (a stream synchronisation costs ~10 us per round); after 2 ms without progress fall back to the synchronisation, which
            // also surfaces errors
            unsigned long long w = __atomic_load_n(h_word, __ATOMIC_ACQUIRE);
            if ((w >> 49) < (round & 0x7FFFu)) {
                if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - wait_start > std::chrono::milliseconds(2)) {
                    const hipError_t e = hipStreamSynchronize(st);
                    if (e != hipSuccess) return drained(fail(ctx, CLC_ERR_HIP, "hipStreamSynchronize(st)", e));
                    w = __atomic_load_n(h_word, __ATOMIC_ACQUIRE);
                    if ((w >> 49) < (round & 0x7FFFu)) return drained(fail(ctx, CLC_ERR_HIP, "acransac: round did not complete"));
                } else return CLC_OK;
            }
            const int iter_k = (int)(w & 0xFFFFFu), n_iter_k = (int)((w >> 20) & 0xFFFFFu);
            if (iter_k < n_iter_k) {
                const bool switched = ((w >> 48) & 1u) != 0;
                const long left = (long)n_iter_k - iter_k + 4 + (switched ? 0 : reserve0);
                bound = left > batch_cap ? batch_cap : (int)left;
                if (round > 0x7000u) return drained(fail(ctx, CLC_ERR_STATE, "acransac: too many rounds"));
                reported = true;
                return CLC_OK;
            }
            // done: the completing round has left the result in pinned memory
            prof_mark(prof, CLC_KERNEL_PNP_SCORE, false, st);
            // The result record, mask and inlier list were written by the round that completed the run BEFORE its word (system-scope
            // release / acquire): no finish launch, and without refinement no stream synchronisation either -- the round enqueued ahead is
            // still in the stream, evaluates nothing and touches no host memory; anything enqueued later on this stream is ordered behind it.
            return after_rounds();
        }
        if (phase == REFINE) {
            if (__atomic_load_n(ready, __ATOMIC_ACQUIRE) == 0) {
                if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - wait_start > std::chrono::milliseconds(5)) {
                    const hipError_t e = hipStreamSynchronize(after_st);
                    if (e != hipSuccess) return drained(fail(ctx, CLC_ERR_HIP, "hipStreamSynchronize(refine stream)", e));
                    if (__atomic_load_n(ready, __ATOMIC_ACQUIRE) == 0) return drained(fail(ctx, CLC_ERR_HIP, "acransac: refinement did not complete"));
                } else return CLC_OK;
            }
            phase = DONE;
        }
        return status;
    }

    // The model as the run leaves it, into h_model (nullable; AcrRun's head says what each kind leaves); r: the run's record, which a
    // kind may still amend
    void model_out(AcrResult& r)
    {
        const size_t m9 = sizeof(double) * 9;
        switch ((AcrKindId)kind) {
        case kAcrResection:
            if (h_model) memcpy(h_model, r.model, sizeof(double) * 12);
            return;
        case kAcrEssential:
            if (h_model) { memcpy(h_model, r.model + 9, m9); memcpy(h_model + 9, r.model, m9); }      // the slots hold { F, E }
            return;
        case kAcrFundamental:
            // Unnormalize(&model): F = N2^T Fn N1 (no model: zeros); it is its own fundamental matrix
            if (!h_model) return;
            if (r.n_inliers > 0) tv::unnormalize(false, norm_t, r.model, h_model);
            else memset(h_model, 0, m9);
            memcpy(h_model + 9, h_model, m9);
            return;
        case kAcrHomography:
            // Unnormalize(&model): H = N2^-1 Hn N1 (no model: zeros); no fundamental matrix goes with it
            if (!h_model) return;
            if (r.n_inliers > 0) tv::unnormalize(true, norm_t, r.model, h_model);
            else memset(h_model, 0, m9);
            memset(h_model + 9, 0, m9);
            return;
        case kAcrSimilarity: {
            // what the refit launch decided: not accepted = no model, no inliers (min_nfa and the iterations stay the run's)
            const Sim3Out o = *p_sim;
            if (!o.found) { r.n_inliers = 0; r.error_max = 0.0; r.valid = -1; }
            if (sim) { *sim = o; sim->ready = 0; }
            if (h_model) memcpy(h_model, o.A, sizeof o.A);
            return;
        }
        case kAcrKindCount: return;
        }
    }

    // after phase == DONE with status CLC_OK and a run that was started: the result into the caller's buffers
    void finish()
    {
        if (status != CLC_OK || !h_res) return;
        AcrResult r = *h_res;
        model_out(r);
        if (valid) *valid = r.valid;
        // the mask is rebuilt from the inlier list here (h_mask was cleared above): the device does not push N bytes + one scattered byte
        // per inlier over PCIe for it
        if (h_mask) for (int i = 0; i < r.n_inliers; ++i) h_mask[p_inl[i]] = 1;
        if (h_inliers && r.n_inliers > 0) memcpy(h_inliers, p_inl, sizeof(int32_t) * (size_t)r.n_inliers);
        if (n_inliers) *n_inliers = r.n_inliers;
        if (error_max) *error_max = r.error_max;
        if (min_nfa) *min_nfa = r.min_nfa;
        if (iterations) *iterations = r.iterations;
        if (rounds) *rounds = r.rounds;
        if (refine && r.n_inliers > 0) {
            if (h_model) memcpy(h_model, p_ref->Rt, sizeof p_ref->Rt);
            if (h_cov) memcpy(h_cov, p_ref->cov, sizeof p_ref->cov);
            if (rmse) *rmse = p_ref->rmse;
        }
    }
};

// A group: runs that share one stream and one sequence of launches -- round r of every run of the group still in its rounds is ONE
// launch (resection) or two (two-view) with blockIdx.y = run (launch_acr_round).  The group owns everything that goes into its stream:
// the ordering behind the other contexts' streams, the staging, the rounds, and the ordering of the other contexts' streams behind it.
struct AcrGroup {
    bool shared = false;              // a lockstep batch (acr_lockstep): every run of the batch, on the first context's stream
    bool running = false;
    std::vector<AcrRun*> live;        // the runs that entered their rounds
    hipStream_t st = nullptr;
    int launches = 0;

    // CLC_KERNEL_PNP_SCORE brackets the rounds of a run that has the stream to itself
    Profiler* prof(AcrRun* r) const { return shared ? nullptr : &r->ctx->prof; }
    void fail_all(const int code)
    {
        for (AcrRun* r : live) if (r->phase != AcrRun::DONE) (void)r->drained(code);
        running = false;
    }

    // first: the context of the group's first run, whose stream the group runs on
    void start(clc_ctx* first)
    {
        if (live.empty()) return;
        st = first->stream;
        running = true;
        clc_ctx* ctx0 = live[0]->ctx;
        // A solve's workspace (its context's d_pnp: inputs, both state copies, slots) may still be written by launches that an EARLIER solve
        // left on that context's OWN stream -- a solve returns when its word says "done", the round enqueued ahead of it is still queued
        // and its keeper carries the state forward.  This group's staging and rounds have to come behind those.
        for (AcrRun* r : live) {
            r->st = st;
            clc_ctx* c = r->ctx;
            if (c->stream != st) (void)order_behind(c->ev_group, c->stream, &st, 1);
        }
        // the inputs of all runs: one staging launch per kMaxBatch of them
        for (size_t k = 0; k < live.size(); k += kMaxBatch) {
            const int n = (int)std::min<size_t>(kMaxBatch, live.size() - k);
            const double* src[kMaxBatch]; double* dst[kMaxBatch]; size_t cnt[kMaxBatch];
            const double* da[kMaxBatch]; const double* db[kMaxBatch]; int nc[kMaxBatch];      // (runs that start from device tracks / pairs)
            int aw[kMaxBatch]; double cond[kMaxBatch][3];
            for (int i = 0; i < n; ++i) {
                const AcrRun* r = live[k + i];
                src[i] = r->stage_src; dst[i] = r->stage_dst; cnt[i] = r->stage_n;
                const AcrKindInfo kd = acr_kind(r->kind);
                da[i] = kd.in_place ? nullptr : r->dev_a; db[i] = kd.in_place ? nullptr : r->dev_b; nc[i] = r->N;      // (in place: not staged)
                aw[i] = kd.a_width;
                const bool cnd = kd.conditioned && r->dev_a;
                cond[i][0] = cnd ? r->norm_t.d : 0.0; cond[i][1] = cnd ? r->norm_t.tx : 0.0; cond[i][2] = cnd ? r->norm_t.ty : 0.0;
            }
            const hipError_t e = launch_acr_stage(src, dst, cnt, n, st, da, db, nc, aw, cond);
            if (e != hipSuccess) {
                fail_all(fail(ctx0, CLC_ERR_HIP, shared ? "acransac: shared staging launch" : "launch_acr_stage(&stage_src, &stage_dst, &stage_n, 1, st)", e));
                return;
            }
        }
        for (AcrRun* r : live) prof_mark(prof(r), CLC_KERNEL_PNP_SCORE, true, st);
        int b0 = 1, b1 = 1;
        for (AcrRun* r : live) { b0 = std::max(b0, r->first_bound); b1 = std::max(b1, r->bound); }
        if (enqueue(b0)) (void)enqueue(b1);                            // the second: speculative, the round after the one being waited for
    }

    // The next round of the runs that are still in their rounds (what the host knows when it enqueues: a run that finishes in the round
    // being waited for rides along once more and finds nothing to replay), kMaxBatch per launch.  Rounds are enqueued ONE AHEAD of what the
    // host knows: the solve / nfa / select kernels take the round's batch from the device state (a round enqueued after the run has
    // finished finds nothing to do), so the GPU goes from one round's select straight into the next round's solve while the host is still
    // polling (a 10 us bubble per round otherwise).  False: the group has failed.
    bool enqueue(const int bound)
    {
        AcrChains pack;
        int n = 0;
        auto flush = [&]() -> bool {
            if (n == 0) return true;
            const hipError_t e = launch_acr_round(pack, n, launches & 1, bound, st);
            n = 0;
            if (e == hipSuccess) return true;
            fail_all(fail(live[0]->ctx, CLC_ERR_HIP, shared ? "acransac: shared round launch" : "launch_acr_round(one, 1, launches & 1, bnd, st)", e));
            return false;
        };
        for (AcrRun* r : live) {
            if (r->phase != AcrRun::ROUNDS) continue;
            r->chain(pack.c[n++]);
            if (n == kMaxBatch && !flush()) return false;
        }
        if (!flush()) return false;
        ++launches;
        return true;
    }

    // One look at every run that is not waiting for the group's next launch (ROUNDS: its word; REFINE: its record); once every run still
    // in its rounds has reported, the next launch (refinements of finished runs may still be out on their own streams; they do not hold
    // the rounds up).
    void step()
    {
        bool any_live = false, rounds_waiting = false, any_more = false;
        int bnd = 1;
        for (AcrRun* r : live) {
            if (r->phase == AcrRun::DONE) continue;
            any_live = true;
            if (!(r->phase == AcrRun::ROUNDS && r->reported)) (void)r->poll(prof(r));
            if (r->phase != AcrRun::ROUNDS) continue;
            if (!r->reported) rounds_waiting = true;
            else { any_more = true; bnd = std::max(bnd, r->bound); }
        }
        if (!any_live) end();
        else if (any_more && !rounds_waiting && enqueue(bnd))
            for (AcrRun* r : live) if (r->phase == AcrRun::ROUNDS) r->advance();
    }

    // The launch enqueued ahead of the last round is still in the group's stream (it finds nothing to replay, but its keepers carry every
    // chain's state forward inside that chain's workspace): whatever the other contexts enqueue next on THEIR streams -- the staging of
    // their next solve, a refinement -- has to come behind it.
    void end()
    {
        running = false;
        if (std::all_of(live.begin(), live.end(), [&](const AcrRun* r) { return r->ctx->stream == st; })) return;
        std::vector<hipStream_t> own;
        for (const AcrRun* r : live) own.push_back(r->ctx->stream);
        (void)order_behind(live[0]->ctx->ev_group, st, own.data(), own.size());
    }
};

// The batch's solves -- one kind, contexts on one device -- share their launches (lockstep, round 5) or run chains of their own.  Why:
// eight interleaved poses were ~80 launches from one thread (4-5 us each inside the runtime, and the runtime serialises launching threads),
// eight two-view filters ~100; in lockstep they are ~10 and ~16.  Same bits per solve: a chain's kernels take its batch from its own device
// state, the grid and the sort width (the largest chain's) only bound them.
// Measured (MI355X, N = 1 000, 30 % outliers, tools/time_two_view.py; interleaved -> lockstep, one staging launch
// for the batch, a round's launches carrying only the solves still in their rounds):
//     two-view filters   2: 0.417 -> 0.439 ms   4: 0.570 -> 0.574   8: 1.08-1.21 -> 0.75-0.80      (rounds of <= 12 / 16 iterations)
//     resection poses    2: 0.190 -> 0.189      4: 0.251 -> 0.271   8: 0.514 -> 0.508; with rounds of <= 8 iterations 0.429 (4: 0.295)
// The interleaved batch is bound by the host's launch calls (eight poses = ~70 launches of 5-7 us from one thread, two of them in flight on
// the device at a time); in lockstep eight poses are ~12 launches, but each carries every solve's speculative slots -- 8 x 32 iterations x 4
// models of 1 024 threads do not fit the chip at once (33 us per round against 17.5) -- hence the cap on a round's iterations, which costs
// rounds.  The two-view round is a 44 us chain of dependent fp64 steps in ONE wave per iteration: eight chains' solves in one launch cost
// what one costs.  Default (acr_kind()'s lockstep_from / lockstep_cap): lockstep for essential batches of four or more (rounds of <= 12
// iterations) and batches of eight or more of the one-launch kinds (<= 8); CLC_ACR_LOCKSTEP=1 / =0 forces it on (any batch of two or
// more) / off for every kind, CLC_ACR_BATCH_CAP the iterations.
bool acr_lockstep(const int kind, const int n_jobs)
{
    static const int mode = [] { const char* e = getenv("CLC_ACR_LOCKSTEP"); return !e ? -1 : (e[0] == '0' ? 0 : 1); }();
    if (n_jobs < 2 || mode == 0) return false;
    if (mode == 1) return true;
    return n_jobs >= acr_kind(kind).lockstep_from;     // (the one-launch rounds share the resection's break-even)
}

// Every run to its end from ONE host thread.  shared: the runs are ONE group on the first run's context's stream (a lockstep batch);
// otherwise every run is a group of its own on its context's stream (a single solve, an interleaved batch), started -- staged, its first
// two rounds enqueued -- as soon as it is begun, so that the host prepares the next run's inputs while the device runs this one's rounds.
// A run is a chain of short launches with the host in the loop and leaves the GPU idle most of the time, so the groups' chains interleave
// on the device (BASELINE config[2]: "batched PnP/RANSAC pose").  Round 5 measured two and three driving threads (the runs dealt out,
// each thread on its runs' own contexts and streams): eight two-view filters 0.134 -> 0.136 ms per pair, eight poses 0.049 -> 0.052 ms per
// pose -- the chains' own latency, not the host's launch calls, is what a batch waits for; one thread stays.
void acr_drive(AcrRun* runs, const int n, const bool shared)
{
    std::vector<AcrGroup> groups(shared ? 1 : (size_t)n);
    for (int i = 0; i < n; ++i) {
        AcrRun& r = runs[i];
        AcrGroup& g = groups[shared ? 0 : (size_t)i];
        g.shared = shared;
        int cap = shared ? acr_kind(r.kind).lockstep_cap : kAcrMaxBatch;      // (a shared launch carries every chain's speculative slots: shorter rounds)
        if (const char* e = getenv("CLC_ACR_BATCH_CAP")) { const int v = atoi(e); if (v >= 1 && v <= kAcrMaxBatch) cap = v; }
        (void)r.begin(cap);
        if (r.phase == AcrRun::ROUNDS) g.live.push_back(&r);
        if (!shared) g.start(r.ctx);
        else if (i == n - 1) g.start(runs[0].ctx);
    }
    for (bool any = true; any;) {
        any = false;
        for (AcrGroup& g : groups) if (g.running) { g.step(); any = true; }
    }
}

// a single solve whose arguments are in `run`
int solve_one(AcrRun& run)
{
    acr_drive(&run, 1, false);
    run.finish();
    return run.status;
}

// The end of a batch: every run's result into its caller's buffers, then per_job(i, status of run i) for what the entry point adds (the
// job's status, its copies); returns the first failure.
template <class F> int finish_all(std::vector<AcrRun>& runs, F&& per_job)
{
    int first = CLC_OK;
    for (size_t i = 0; i < runs.size(); ++i) {
        runs[i].finish();
        per_job(i, runs[i].status);
        if (runs[i].status != CLC_OK && first == CLC_OK) first = runs[i].status;
    }
    return first;
}

} // namespace

extern "C" {

int clc_pnp_acransac(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, int max_iteration, uint64_t seed,
                     double precision, double* h_Rt, uint8_t* h_inlier_mask, int32_t* h_inliers, int* n_inliers, double* error_max,
                     double* min_nfa, int* iterations)
{
    if (h_Rt) memset(h_Rt, 0, sizeof(double) * 12);
    AcrRun run;
    run.ctx = ctx; run.kind = kAcrResection; run.h_a = h_X; run.h_b = h_x; run.N = N; run.h_K1 = h_K;
    run.max_iteration = max_iteration; run.seed = seed; run.precision = precision;
    run.h_model = h_Rt; run.h_mask = h_inlier_mask; run.h_inliers = h_inliers; run.n_inliers = n_inliers; run.error_max = error_max;
    run.min_nfa = min_nfa; run.iterations = iterations;
    return solve_one(run);
}

int clc_pnp_localize_ac(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, int max_iteration, uint64_t seed,
                        double precision, double huber_a, double* h_Rt, double* h_cov, uint8_t* h_inlier_mask, int32_t* h_inliers,
                        int* n_inliers, double* error_max, double* rmse)
{
    if (h_Rt) memset(h_Rt, 0, sizeof(double) * 12);
    if (h_cov) memset(h_cov, 0, sizeof(double) * 36);
    if (rmse) *rmse = 0.0;
    AcrRun run;
    run.ctx = ctx; run.kind = kAcrResection; run.h_a = h_X; run.h_b = h_x; run.N = N; run.h_K1 = h_K;
    run.max_iteration = max_iteration; run.seed = seed; run.precision = precision; run.refine_huber = refine_huber_of(true, huber_a);
    run.h_model = h_Rt; run.h_mask = h_inlier_mask; run.h_inliers = h_inliers; run.n_inliers = n_inliers; run.error_max = error_max;
    run.h_cov = h_cov; run.rmse = rmse;
    return solve_one(run);
}

int clc_pnp_localize_ac_batch(clc_ctx* const* ctxs, clc_pose_job* jobs, int n_jobs)
{
    if (n_jobs < 0 || (n_jobs > 0 && (!ctxs || !jobs))) return CLC_ERR_BAD_ARG;
    if (n_jobs == 0) return CLC_OK;
    const int rc0 = check_batch_contexts(ctxs, n_jobs, "pnp_localize_ac_batch: every job needs a context of its own");
    if (rc0 != CLC_OK) return rc0;
    std::vector<AcrRun> runs((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        clc_pose_job& jb = jobs[i];
        AcrRun& r = runs[(size_t)i];
        if (jb.Rt) memset(jb.Rt, 0, sizeof(double) * 12);
        if (jb.cov) memset(jb.cov, 0, sizeof(double) * 36);
        jb.n_inliers = 0; jb.error_max = 0.0; jb.rmse = 0.0; jb.iterations = 0;
        r.ctx = ctxs[i]; r.kind = kAcrResection; r.h_a = jb.X; r.h_b = jb.x; r.N = jb.n; r.h_K1 = jb.K;
        r.max_iteration = jb.max_iteration; r.seed = jb.seed; r.precision = jb.precision;
        r.refine_huber = refine_huber_of(jb.refine, jb.huber_a);
        r.h_model = jb.Rt; r.h_mask = jb.inlier_mask; r.h_inliers = jb.inliers; r.n_inliers = &jb.n_inliers; r.error_max = &jb.error_max;
        r.iterations = &jb.iterations; r.h_cov = jb.cov; r.rmse = &jb.rmse;
    }
    acr_drive(runs.data(), n_jobs, acr_lockstep(kAcrResection, n_jobs));
    return finish_all(runs, [&](const size_t i, const int status) { jobs[i].status = status; });
}

int clc_essential_acransac(clc_ctx* ctx, const double* h_x1, const double* h_x2, int N, const double* h_K1, const double* h_K2,
                           int img_w, int img_h, int max_iteration, uint64_t seed, double precision, double* h_E, double* h_F,
                           uint8_t* h_inlier_mask, int32_t* h_inliers, int* n_inliers, double* error_max, double* min_nfa, int* iterations)
{
    return clc_two_view_acransac(ctx, CLC_MODEL_ESSENTIAL, h_x1, h_x2, N, h_K1, h_K2, img_w, img_h, max_iteration, seed, precision, h_E, h_F,
                                 h_inlier_mask, h_inliers, n_inliers, error_max, min_nfa, iterations);
}

int clc_two_view_acransac(clc_ctx* ctx, int model, const double* h_x1, const double* h_x2, int N, const double* h_K1, const double* h_K2,
                          int img_w, int img_h, int max_iteration, uint64_t seed, double precision, double* h_M, double* h_F,
                          uint8_t* h_inlier_mask, int32_t* h_inliers, int* n_inliers, double* error_max, double* min_nfa, int* iterations)
{
    const int kind = acr_kind_of_model(model);
    if (!acr_is_kind(kind)) return fail(ctx, CLC_ERR_BAD_ARG, "two_view_acransac: model must be 'E', 'F' or 'H'");
    // the model as the solve leaves it (AcrRun::model_out): the model matrix, then the fundamental matrix that goes with it
    double EF[18] = {};
    AcrRun run;
    run.ctx = ctx; run.kind = kind; run.h_a = h_x1; run.h_b = h_x2; run.N = N; run.img_w = img_w; run.img_h = img_h;
    if (acr_kind(kind).needs_K1) run.h_K1 = h_K1;
    if (acr_kind(kind).needs_K2) run.h_K2 = h_K2;
    run.max_iteration = max_iteration; run.seed = seed; run.precision = precision;
    run.h_model = EF; run.h_mask = h_inlier_mask; run.h_inliers = h_inliers; run.n_inliers = n_inliers; run.error_max = error_max;
    run.min_nfa = min_nfa; run.iterations = iterations;
    const int rc = solve_one(run);
    if (h_M) memcpy(h_M, EF, sizeof(double) * 9);
    if (h_F) memcpy(h_F, EF + 9, sizeof(double) * 9);
    return rc;
}

int clc_two_view_minimal(clc_ctx* ctx, int model, const double* h_x1, const double* h_x2, int N, int img_w, int img_h, const int32_t* h_samples,
                         int S, double* h_models)
{
    const int kind = acr_kind_of_model(model);
    if (!ctx || (kind != kAcrFundamental && kind != kAcrHomography) || N <= 0 || S < 0 || !h_x1 || !h_x2 || img_w <= 0 || img_h <= 0 || (S > 0 && (!h_samples || !h_models)))
        return fail(ctx, CLC_ERR_BAD_ARG, "two_view_minimal: bad argument (models 'F' and 'H')");
    if (S == 0) return CLC_OK;
    const int m = acr_kind(kind).m, M = acr_kind(kind).M;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pts = (size_t)4 * N, out = (size_t)S * M * 9;
    TwoViewMinDev dv;
    int rc = ensure_pnp(ctx, [&](Carve& c) { dv.carve(c, (size_t)N, (size_t)S * m, out); });
    if (rc != CLC_OK) return rc;
    std::vector<double> q(pts);
    const tv::Normalizer t = tv::normalizer(img_w, img_h);
    tv::condition(t, h_x1, N, q.data());
    tv::condition(t, h_x2, N, q.data() + (size_t)2 * N);
    double* d = dv.x1;
    int32_t* d_smp = dv.samples;
    double* d_out = dv.out;
    CLC_HIP(ctx, hipMemcpyAsync(d, q.data(), sizeof(double) * pts, hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, hipMemcpyAsync(d_smp, h_samples, sizeof(int32_t) * (size_t)S * m, hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, launch_twoview_minimal(kind, dv.x1, dv.x2, N, d_smp, S, d_out, ctx->stream));
    CLC_HIP(ctx, hipMemcpyAsync(h_models, d_out, sizeof(double) * out, hipMemcpyDeviceToHost, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CLC_OK;
}

// The 3-D similarity NEW -> OLD between two landmark sets (sim3_math.h; the project's own statement, include/coloc_hip.h)
int clc_sim3_acransac(clc_ctx* ctx, const double* h_x_new, const double* h_x_old, int N, int max_iteration, uint64_t seed, double precision,
                      double* s, double* h_R, double* h_t, double* h_A, uint8_t* h_inlier_mask, int32_t* h_inliers, int* n_inliers,
                      double* error_max, double* min_nfa, int* iterations, int* valid, int* refit)
{
    Sim3Out o{};
    AcrRun run;
    run.ctx = ctx; run.kind = kAcrSimilarity; run.h_a = h_x_new; run.h_b = h_x_old; run.N = N;
    run.max_iteration = max_iteration; run.seed = seed; run.precision = precision;
    run.sim = &o; run.h_mask = h_inlier_mask; run.h_inliers = h_inliers; run.n_inliers = n_inliers; run.error_max = error_max;
    run.min_nfa = min_nfa; run.iterations = iterations; run.valid = valid;
    const int rc = solve_one(run);
    if (o.s == 0.0) o = sim3_identity();      // (refused before begin() reached the record)
    if (s) *s = o.s;
    if (h_R) memcpy(h_R, o.R, sizeof o.R);
    if (h_t) memcpy(h_t, o.t, sizeof o.t);
    if (h_A) memcpy(h_A, o.A, sizeof o.A);
    if (refit) *refit = o.refit;
    return rc;
}

int clc_sim3_minimal(clc_ctx* ctx, const double* h_x_new, const double* h_x_old, int N, const int32_t* h_samples, int S, double* h_models)
{
    if (!ctx || N <= 0 || S < 0 || !h_x_new || !h_x_old || (S > 0 && (!h_samples || !h_models)))
        return fail(ctx, CLC_ERR_BAD_ARG, "sim3_minimal: bad argument");
    if (S == 0) return CLC_OK;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    Sim3MinDev dv;
    const int rc = ensure_pnp(ctx, [&](Carve& c) { dv.carve(c, (size_t)N, (size_t)S); });
    if (rc != CLC_OK) return rc;
    CLC_HIP(ctx, hipMemcpyAsync(dv.x, h_x_new, sizeof(double) * 3 * (size_t)N, hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, hipMemcpyAsync(dv.y, h_x_old, sizeof(double) * 3 * (size_t)N, hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, hipMemcpyAsync(dv.samples, h_samples, sizeof(int32_t) * 3 * (size_t)S, hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, launch_sim3_minimal(dv.x, dv.y, N, dv.samples, S, dv.out, ctx->stream));
    CLC_HIP(ctx, hipMemcpyAsync(h_models, dv.out, sizeof(double) * 12 * (size_t)S, hipMemcpyDeviceToHost, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CLC_OK;
}

} // extern "C"

namespace {

void two_view_run(AcrRun& r, clc_ctx* ctx, clc_two_view_job& jb, double* EF, const int kind)
{
    if (jb.E) memset(jb.E, 0, sizeof(double) * 9);
    if (jb.F) memset(jb.F, 0, sizeof(double) * 9);
    jb.n_inliers = 0; jb.iterations = 0; jb.error_max = 0.0; jb.min_nfa = INFINITY;
    r.ctx = ctx; r.kind = kind; r.h_a = jb.x1; r.h_b = jb.x2; r.N = jb.n; r.h_K1 = jb.K1; r.h_K2 = jb.K2; r.img_w = jb.img_w; r.img_h = jb.img_h;
    r.max_iteration = jb.max_iteration; r.seed = jb.seed; r.precision = jb.precision; r.refine_huber = -1.0;
    r.h_model = EF; r.h_mask = jb.inlier_mask; r.h_inliers = jb.inliers; r.n_inliers = &jb.n_inliers; r.error_max = &jb.error_max;
    r.min_nfa = &jb.min_nfa; r.iterations = &jb.iterations;
}


} // namespace

namespace clc {

hipError_t order_behind(Event& ev, hipStream_t producer, const hipStream_t* consumers, const size_t n)
{
    bool ok = ev.create(hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, producer) == hipSuccess;
    for (size_t i = 0; i < n && ok; ++i)
        if (consumers[i] != producer) ok = hipStreamWaitEvent(consumers[i], ev, 0) == hipSuccess;
    return ok ? hipSuccess : hipStreamSynchronize(producer);
}

int check_batch_contexts(clc_ctx* const* ctxs, int n_jobs, const char* what)
{
    for (int i = 0; i < n_jobs; ++i) {
        if (!ctxs[i]) return CLC_ERR_BAD_ARG;
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) return fail(ctxs[i], CLC_ERR_BAD_ARG, what);
        if (ctxs[i]->device != ctxs[0]->device) return fail(ctxs[i], CLC_ERR_BAD_ARG, "batch: the contexts must live on one device");
    }
    return CLC_OK;
}


int sim3_solve_dev(clc_ctx* ctx, const double* d_x_new, const double* d_x_old, int N, const double* box, int max_iteration, uint64_t seed,
                   double precision, Sim3Out* out, uint8_t* h_mask, int* n_inliers, double* error_max, double* min_nfa, int* iterations)
{
    AcrRun run;
    run.ctx = ctx; run.kind = kAcrSimilarity; run.dev_a = d_x_new; run.dev_b = d_x_old; run.box = box; run.N = N;
    run.max_iteration = max_iteration; run.seed = seed; run.precision = precision;
    run.sim = out; run.h_mask = h_mask; run.n_inliers = n_inliers; run.error_max = error_max; run.min_nfa = min_nfa; run.iterations = iterations;
    return solve_one(run);
}

// The model matrix -> job.E (RelativePose_Info::essential_matrix receives it, whatever the model: RobustMatcher.hpp:141, :207), the
// fundamental matrix that goes with it -> job.F (AcrRun::model_out)
int acr_two_view_batch(clc_ctx* const* ctxs, clc_two_view_job* const* jobs, int n_jobs, int kind)
{
    std::vector<AcrRun> runs((size_t)n_jobs);
    std::vector<double> EF((size_t)18 * n_jobs, 0.0);
    for (int i = 0; i < n_jobs; ++i) two_view_run(runs[(size_t)i], ctxs[i], *jobs[i], &EF[(size_t)18 * i], kind);
    acr_drive(runs.data(), n_jobs, acr_lockstep(kind, n_jobs));
    return finish_all(runs, [&](const size_t i, const int status) {
        jobs[i]->status = status;
        if (jobs[i]->E) memcpy(jobs[i]->E, &EF[18 * i], sizeof(double) * 9);
        if (jobs[i]->F) memcpy(jobs[i]->F, &EF[18 * i + 9], sizeof(double) * 9);
    });
}

} // namespace clc

extern "C" {

// who: the entry point's name, as its error text carries it
static int two_view_batch_entry(const char* who, clc_ctx* const* ctxs, int model, clc_two_view_job* jobs, int n_jobs)
{
    const int kind = acr_kind_of_model(model);
    if (!acr_is_kind(kind) || n_jobs < 0 || (n_jobs > 0 && (!ctxs || !jobs))) return CLC_ERR_BAD_ARG;
    if (n_jobs == 0) return CLC_OK;
    const int rc0 = check_batch_contexts(ctxs, n_jobs, (std::string(who) + ": every job needs a context of its own").c_str());
    if (rc0 != CLC_OK) return rc0;
    std::vector<clc_two_view_job*> ptr((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) ptr[(size_t)i] = &jobs[i];
    return acr_two_view_batch(ctxs, ptr.data(), n_jobs, kind);
}

int clc_essential_acransac_batch(clc_ctx* const* ctxs, clc_two_view_job* jobs, int n_jobs)
{
    return two_view_batch_entry("essential_acransac_batch", ctxs, CLC_MODEL_ESSENTIAL, jobs, n_jobs);
}

int clc_two_view_acransac_batch(clc_ctx* const* ctxs, int model, clc_two_view_job* jobs, int n_jobs)
{
    return two_view_batch_entry("two_view_acransac_batch", ctxs, model, jobs, n_jobs);
}

} // extern "C"

// ---- the solves that start from device matches (include/coloc_hip.h: clc_track_localize*_dev, clc_pair_filter*_dev) -------------------
// Localizer::localizeImage from device tracks, RobustMatcher::computeRelativePose from device pairs.  The gather kernel (gather.hip) writes
// each job's correspondences into its context's block -- the pairs in PIXELS -- and the count N into a pinned word; the host waits for
// that one number -- AcrRun::begin_body lays the workspace out by N and builds the N-dependent NFA tables --, then the runs go through
// acr_drive like every other solve.  The staging launch reads TWO sources per run: a | b from the block -- conditioned for 'F' / 'H' on
// the way, where it costs no launch and leaves the block's pinned mirrors in pixels for the pose from E --, K, the tables and the initial
// state from the pinned block (launch_acr_stage); no gather launch of its own, and nothing sized by N sits in front of the count.
namespace {

// What differs between the two paths, for gather_solve: the job, its block, the outputs it asks the kernel for, its solve and its results.
// K / model: 18 doubles each of the driver's, alive until the job's results are out.
struct TrackPath {
    using Job = clc_track_job; using Dev = TrackJobDev; using Jobs = TrackJobs;
    static constexpr const char* who = "track_localize";
    static constexpr GatherLayout layout = kTrackLayout;
    static GatherBlock& block(clc_ctx* c) { return c->trk; }
    static int& count(Job& jb) { return jb.n_tracks; }
    static void reset(Job& jb)
    {
        if (jb.Rt) memset(jb.Rt, 0, sizeof(double) * 12);
        if (jb.cov) memset(jb.cov, 0, sizeof(double) * 36);
        jb.n_tracks = 0; jb.n_inliers = 0; jb.iterations = 0; jb.status = CLC_OK; jb.error_max = 0.0; jb.rmse = 0.0;
    }
    static void pack(Jobs& p, const clc_ctx* c0) { p.map_X = c0->d_map_X.as<double>(); p.map_n = c0->map_X_n; }
    static void outputs(Dev& d, const GatherView& v, const Job& jb)
    {
        d.X = v.a; d.x = v.b; d.query = v.q; d.map = v.t;
        d.h_query = jb.track_query ? v.h_q : nullptr;
        d.h_map = jb.track_map ? v.h_t : nullptr;
    }
    static void solve(AcrRun& r, Job& jb, int, double* K, double*)
    {
        K[0] = jb.cam.focal; K[2] = jb.cam.ppx; K[4] = jb.cam.focal; K[5] = jb.cam.ppy; K[8] = 1.0;      // Pinhole_Intrinsic_Radial_K3::K()
        r.h_K1 = K;
        r.refine_huber = refine_huber_of(jb.refine, jb.huber_a);
        r.h_model = jb.Rt; r.h_cov = jb.cov; r.rmse = &jb.rmse;
    }
    // trackedFeatures
    static void results(Job& jb, const GatherView& v, const size_t n, const double*)
    {
        if (jb.track_query && n) memcpy(jb.track_query, v.h_q, sizeof(int32_t) * n);
        if (jb.track_map && n) memcpy(jb.track_map, v.h_t, sizeof(int32_t) * n);
    }
};

struct PairPath {
    using Job = clc_pair_job; using Dev = PairJobDev; using Jobs = PairJobs;
    static constexpr const char* who = "pair_filter";
    static constexpr GatherLayout layout = kPairLayout;
    static GatherBlock& block(clc_ctx* c) { return c->pair; }
    static int& count(Job& jb) { return jb.n_pairs; }
    static void reset(Job& jb)
    {
        if (jb.M) memset(jb.M, 0, sizeof(double) * 9);
        if (jb.F) memset(jb.F, 0, sizeof(double) * 9);
        jb.n_pairs = 0; jb.n_inliers = 0; jb.iterations = 0; jb.status = CLC_OK; jb.error_max = 0.0; jb.min_nfa = INFINITY;
    }
    static void pack(Jobs&, const clc_ctx*) {}
    static void outputs(Dev& d, const GatherView& v, const Job& jb)
    {
        d.x1 = v.a; d.x2 = v.b; d.pair_q = v.q; d.pair_t = v.t;
        d.h_q = jb.pair_q ? v.h_q : nullptr;
        d.h_t = jb.pair_t ? v.h_t : nullptr;
        d.h_x1 = jb.x1 ? v.h_a : nullptr;
        d.h_x2 = jb.x2 ? v.h_b : nullptr;
    }
    static void solve(AcrRun& r, Job& jb, const int kind, double* K, double* model)
    {
        K[0] = jb.cam_a.focal; K[2] = jb.cam_a.ppx; K[4] = jb.cam_a.focal; K[5] = jb.cam_a.ppy; K[8] = 1.0;      // Pinhole_Intrinsic_Radial_K3::K()
        K[9] = jb.cam_b.focal; K[11] = jb.cam_b.ppx; K[13] = jb.cam_b.focal; K[14] = jb.cam_b.ppy; K[17] = 1.0;  // of the two cameras
        if (acr_kind(kind).needs_K1) r.h_K1 = K;
        if (acr_kind(kind).needs_K2) r.h_K2 = K + 9;
        r.img_w = jb.img_w; r.img_h = jb.img_h;
        r.h_model = model; r.min_nfa = &jb.min_nfa;
    }
    // model: the model matrix, then the fundamental matrix that goes with it (AcrRun::model_out) -- as clc_two_view_acransac
    static void results(Job& jb, const GatherView& v, const size_t n, const double* model)
    {
        if (jb.M) memcpy(jb.M, model, sizeof(double) * 9);
        if (jb.F) memcpy(jb.F, model + 9, sizeof(double) * 9);
        if (jb.pair_q && n) memcpy(jb.pair_q, v.h_q, sizeof(int32_t) * n);
        if (jb.pair_t && n) memcpy(jb.pair_t, v.h_t, sizeof(int32_t) * n);
        if (jb.x1 && n) memcpy(jb.x1, v.h_a, sizeof(double) * 2 * n);
        if (jb.x2 && n) memcpy(jb.x2, v.h_b, sizeof(double) * 2 * n);
    }
};

// inliers (nullable): where every run's inlier list lies for the device afterwards (pair_filter_essential, clc_ctx.h)
template <class Path> int gather_solve(clc_ctx* const* ctxs, const int kind, typename Path::Job* jobs, const int n_jobs, const int32_t** inliers = nullptr)
{
    clc_ctx* c0 = ctxs[0];
    const std::string who = Path::who;
    for (int i = 0; i < n_jobs; ++i) Path::reset(jobs[i]);
    CLC_HIP(c0, hipSetDevice(c0->device));
    hipStream_t st = c0->stream;
    std::vector<typename Path::Dev> dev((size_t)n_jobs);
    for (int i = 0; i < n_jobs; ++i) {
        int rc = gather_inputs(c0, jobs[i], dev[(size_t)i], (who + ": bad argument").c_str());
        if (rc == CLC_OK && jobs[i].max_iteration < 0) rc = fail(c0, CLC_ERR_BAD_ARG, (who + ": negative max_iteration").c_str());
        if (rc == CLC_OK) rc = ensure_gather(ctxs[i], Path::block(ctxs[i]), (size_t)std::min(jobs[i].nq, kAcrMaxN), Path::layout);
        if (rc != CLC_OK) {
            if (ctxs[i] != c0) (void)fail(ctxs[i], rc, clc_last_error_string(c0));
            jobs[i].status = rc;
            return rc;
        }
    }
    // behind whatever produced the inputs: an event on the producer's stream, no host synchronisation
    for (int i = 0; i < n_jobs; ++i) {
        hipStream_t prod = (hipStream_t)jobs[i].after_stream;
        if (prod && prod != st) CLC_HIP(ctxs[i], order_behind(ctxs[i]->ev_track, prod, &st, 1));
    }
    // the correspondences of all jobs: one launch per kMaxBatch of them
    for (int k = 0; k < n_jobs; k += kMaxBatch) {
        const int n = std::min(kMaxBatch, n_jobs - k);
        typename Path::Jobs pack{};
        Path::pack(pack, c0);
        for (int i = 0; i < n; ++i) {
            const GatherView v(Path::block(ctxs[k + i]), Path::layout);
            typename Path::Dev& d = dev[(size_t)(k + i)];
            d.n = v.n; d.h_n = v.h_n;
            d.cap = std::min(jobs[k + i].nq, kAcrMaxN);
            Path::outputs(d, v, jobs[k + i]);
            __atomic_store_n(v.h_n, 0xFFFFFFFFu, __ATOMIC_RELAXED);
            pack.j[i] = d;
        }
        CLC_HIP(c0, launch_gather(pack, n, st));
    }
    const bool shared = acr_lockstep(kind, n_jobs);
    if (!shared && n_jobs > 1) {
        // every other run stages from its block on its context's OWN stream: behind the gather launch
        std::vector<hipStream_t> own;
        for (int i = 0; i < n_jobs; ++i) own.push_back(ctxs[i]->stream);
        CLC_HIP(c0, order_behind(c0->ev_track, st, own.data(), own.size()));
    }
    // the one number the host needs: poll the pinned words, the stream synchronisation as the fallback (which also surfaces errors)
    std::vector<AcrRun> runs((size_t)n_jobs);
    std::vector<double> Ks((size_t)18 * n_jobs, 0.0), models((size_t)18 * n_jobs, 0.0);
    const std::string no_count = who + ": the gather launch left no count";
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n_jobs; ++i) {
        const GatherView v(Path::block(ctxs[i]), Path::layout);
        if (const int rc = wait_pinned(c0, v.h_n, 0xFFFFFFFFu, st, t0, 2, no_count.c_str())) return rc;
        const uint32_t w = __atomic_load_n(v.h_n, __ATOMIC_ACQUIRE);
        typename Path::Job& jb = jobs[i];
        Path::count(jb) = (int)w;
        AcrRun& r = runs[(size_t)i];
        r.ctx = ctxs[i]; r.kind = kind; r.N = (int)w; r.dev_a = v.a; r.dev_b = v.b;
        r.max_iteration = jb.max_iteration; r.seed = jb.seed; r.precision = jb.precision;
        r.h_mask = jb.inlier_mask; r.h_inliers = jb.inliers; r.n_inliers = &jb.n_inliers; r.error_max = &jb.error_max;
        r.iterations = &jb.iterations;
        Path::solve(r, jb, kind, &Ks[(size_t)18 * i], &models[(size_t)18 * i]);
    }
    acr_drive(runs.data(), n_jobs, shared);
    return finish_all(runs, [&](const size_t i, const int status) {
        typename Path::Job& jb = jobs[i];
        if (inliers) inliers[i] = runs[i].p_inl;
        jb.status = status;
        // the kernel wrote the pinned mirrors before the count came out
        const GatherView v(Path::block(ctxs[i]), Path::layout);
        Path::results(jb, v, (size_t)std::min(Path::count(jb), std::min(jb.nq, kAcrMaxN)), &models[18 * i]);
    });
}

} // namespace

int clc::pair_filter_essential(clc_ctx* const* ctxs, clc_pair_job* jobs, const int n_jobs, const int32_t** inliers)
{
    for (int i = 0; i < n_jobs; ++i) inliers[i] = nullptr;
    return gather_solve<PairPath>(ctxs, kAcrEssential, jobs, n_jobs, inliers);
}

// The resection of the grow step (map_build.hip): ONE AcrRun filled from the context's track block as gather_solve fills it -- no
// refinement -- and driven like every other solve.
int clc::resect_solve(clc_ctx* ctx, const int N, const clc_camera_k3& cam, const int max_iteration, const uint64_t seed, const double precision,
                      double* Rt, int* n_inliers, double* error_max)
{
    const double K[9] = { cam.focal, 0.0, cam.ppx, 0.0, cam.focal, cam.ppy, 0.0, 0.0, 1.0 };      // Pinhole_Intrinsic_Radial_K3::K()
    memset(Rt, 0, sizeof(double) * 12);
    const GatherView v(ctx->trk, kTrackLayout);
    AcrRun run;
    run.ctx = ctx; run.kind = kAcrResection; run.N = N; run.dev_a = v.a; run.dev_b = v.b; run.h_K1 = K;
    run.max_iteration = max_iteration; run.seed = seed; run.precision = precision;
    run.h_model = Rt; run.n_inliers = n_inliers; run.error_max = error_max;
    return solve_one(run);
}

extern "C" {

int clc_track_localize_batch_dev(clc_ctx* const* ctxs, clc_track_job* jobs, int n_jobs)
{
    if (n_jobs < 0 || (n_jobs > 0 && (!ctxs || !jobs))) return CLC_ERR_BAD_ARG;
    if (n_jobs == 0) return CLC_OK;
    const int rc0 = check_batch_contexts(ctxs, n_jobs, "track_localize_batch: every job needs a context of its own");
    if (rc0 != CLC_OK) return rc0;
    return gather_solve<TrackPath>(ctxs, kAcrResection, jobs, n_jobs);
}

int clc_track_localize_dev(clc_ctx* ctx, clc_track_job* job)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "track_localize: null context / job");
    return gather_solve<TrackPath>(&ctx, kAcrResection, job, 1);
}

int clc_pair_filter_batch_dev(clc_ctx* const* ctxs, int model, clc_pair_job* jobs, int n_jobs)
{
    const int kind = acr_kind_of_model(model);
    if (n_jobs < 0 || (n_jobs > 0 && (!ctxs || !jobs))) return CLC_ERR_BAD_ARG;
    if (n_jobs == 0) return acr_is_kind(kind) ? CLC_OK : CLC_ERR_BAD_ARG;
    const int rc0 = check_batch_contexts(ctxs, n_jobs, "pair_filter_batch: every job needs a context of its own");
    if (rc0 != CLC_OK) return rc0;
    if (!acr_is_kind(kind)) return fail(ctxs[0], CLC_ERR_BAD_ARG, "pair_filter_batch: model must be 'E', 'F' or 'H'");
    return gather_solve<PairPath>(ctxs, kind, jobs, n_jobs);
}

int clc_pair_filter_dev(clc_ctx* ctx, int model, clc_pair_job* job)
{
    if (!ctx || !job) return fail(ctx, CLC_ERR_BAD_ARG, "pair_filter: null context / job");
    const int kind = acr_kind_of_model(model);
    if (!acr_is_kind(kind)) return fail(ctx, CLC_ERR_BAD_ARG, "pair_filter: model must be 'E', 'F' or 'H'");
    return gather_solve<PairPath>(&ctx, kind, job, 1);
}

} // extern "C"

// k2nn_sweep.h -- the popcount sweep, stated once: lane = query, the train row wave-uniform in SGPRs (k2nn.hip's header describes the
// formulation).  The GATE is the body's only parameter: NoGate is the plain sweep (k2nn.hip: k2nn_sweep_kernel), LineGate / PointGate
// the gated ones (k2nn_guided.hip: k2nn_sweep_guided_kernel).  Here: the workgroup's shape and the key layout, the per-row step
// (sweep_one), the query load, the wave's share, the pipelined scalar-load loop and the LDS fold of the waves (sweep_split), the
// atomic fold of a split with the arrival counter and the finalize (sweep_fold_finalize), the acceptance rule and the answer of a row
// (accept / emit_result, which k2nn_binned.hip and the matrix sweep use as well) and the answer of a job without train rows
// (nomatch_rows).  A kernel keeps what is its own: its job record and how the live counts are read from it, its exits (the plain
// kernel's slab rows, the gated kernel's return when nothing is planned) and the acceptance rule it is compiled for.
// The matrix sweep (k2nn.hip: k2nn_sweep_mx_kernel) folds a row with the same top2_row_fold and answers with the same emit_result, but
// keeps its own statement of the arrival (a workgroup barrier, one thread per query) and of the last arrival's exchanges: with those
// behind a shared function as well the instructions of its finalize changed order, and its text is held identical (see accept below).
#ifndef CLC_K2NN_SWEEP_H
#define CLC_K2NN_SWEEP_H

#include "clc_internal.h"
#include "k2nn_top2.h"

namespace clc {

static constexpr int kR = 2;                 // queries per lane
static constexpr int kWaves = 8;             // waves per workgroup
static constexpr int kQPerBlock = 64 * kR;   // the kWaves waves of a workgroup share these queries and cut the train slice in kWaves
static constexpr uint32_t kKeyShift = 22;    // distance <= 512 needs 10 bits; 22 bits of index
static constexpr uint32_t kIdxMask = (1u << kKeyShift) - 1u;
static constexpr uint32_t kEmpty = 0xFFFFFFFFu;

// Pointers arrive inside a job record read from memory, so the compiler only knows them as
// generic.  Re-type them: train rows as CONSTANT address space (wave-uniform address -> s_load),
// query rows / partials as GLOBAL (global_load / global_store instead of flat_*).
// (builtin vector types: HIP's uint4 class has no constructors from qualified address spaces)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef const u32x4 __attribute__((address_space(4)))* const_u4_ptr;
typedef const u32x2 __attribute__((address_space(4)))* const_u2_ptr;
typedef const u32x4 __attribute__((address_space(1)))* global_cu4_ptr;
typedef const float __attribute__((address_space(1)))* global_cf_ptr;
typedef u32x2 __attribute__((address_space(1)))* global_u2_ptr;

// The acceptance rule (K2nnJobDev.rule) on the folded top-2: distances, or the CUDAK2NN.cu:54 sentinels 100000 / 200000 where fewer
// than two / one train rows were swept.  K2NN: CUDAK2NN.cu:75.  Ratio: the sentinel second is checked FIRST -- with one train row the
// 100000 would pass the ratio test -- then (float)d1 < r2 * (float)d2 (oracle/clc_oracle.c orc_k2nn_omp_ex, rule 1; no contraction:
// the build has -ffp-contract=off).  A compile-time parameter of the sweep kernels, not a runtime branch in them: the rule is uniform
// per launch (launch_k2nn), and any change to the finalize of k2nn_sweep_mx_kernel moves its register allocation: with a runtime branch
// here the compiler (ROCm 7, -O3) put 16 v_mov into the K2NN tile loop; with the template the K2NN instantiations keep their tile loop
// (check: hipcc -S --cuda-device-only on k2nn.hip, the tile block of k2nn_sweep_mx_kernel<false, false, false, false>).
// Job: any record with out, best_out, second_out and thr (K2nnJobDev, GuidedJobDev, BinJobDev); r2 is read under RATIO only.
template <bool RATIO, class Job>
__device__ __forceinline__ bool accept(const Job& job, const int best_i, const int best_v, const int second_v)
{
    if (best_i < 0) return false;
    if constexpr (RATIO) return second_v <= 512 && (float)best_v < job.r2 * (float)second_v;
    else return second_v - best_v > (int)job.thr;
}

// {best_key, second_key} of one query -> the reference's outputs (CUDAK2NN.cu:54 sentinels, :75 acceptance)
template <bool RATIO, class Job>
__device__ __forceinline__ void emit_result(const Job& job, const uint32_t qi, const uint32_t bkey, const uint32_t skey)
{
    int best_v = 100000, second_v = 200000, best_i = -1;
    if (bkey != kEmpty) {
        best_v = (int)(bkey >> kKeyShift);
        best_i = (int)(bkey & kIdxMask);
        second_v = skey == kEmpty ? 100000 : (int)(skey >> kKeyShift);
    }
    job.out[qi] = accept<RATIO>(job, best_i, best_v, second_v) ? best_i : -1;
    if (job.best_out) job.best_out[qi] = (uint16_t)min(best_v, 65535);
    if (job.second_out) job.second_out[qi] = (uint16_t)min(second_v, 65535);
}

// Atomic mode, jobs with an EMPTY planned train set only (no sweep workgroup exists that could finalize them): the reference leaves
// best_i uninitialised there (CUDAK2NN.cu:54,75); defined here as "no match".  The body of the 256-thread kernels that answer them.
template <class List>
__device__ __forceinline__ void nomatch_rows(const List& jobs)
{
    const auto& job = jobs.j[blockIdx.y];
    const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
    if (job.nt != 0u || qi >= job.nq) return;
    emit_result<false>(job, qi, kEmpty, kEmpty);                      // no best row: -1 under either rule
}

// ---- the gate ---------------------------------------------------------------------------------------------------------------------
// A gate names kF, the floats of a query that stay in the lane's registers, and pass(), its ONE statement (k2nn_guided.hip: LineGate,
// PointGate).  NoGate has none: no float is kept, no train point is loaded, and the per-row step is the ungated one.
struct NoGate { static constexpr int kF = 0; };
template <class Gate> static constexpr int kGateF = Gate::kF ? Gate::kF : 1;      // a lane's floats per query, as an array bound (NoGate's one is never touched)

// ---- the per-row step -------------------------------------------------------------------------------------------------------------
// One train vector (16 wave-uniform dwords in SGPRs) against the R queries of this lane.
//
// Per query: 16 x (v_xor_b32 with the scalar train word, immediately consumed by v_bcnt_u32_b32 with accumulate), then
// key = (distance << 22) + index; second = med3(best, second, key); best = min(best, key).
// The exact instruction pattern is measured, not guessed (20k x 20k sweep, same device):
//     v_xor ; v_bcnt ; s_nop 0     311-313 us   <- this file
//     v_xor ; v_bcnt               368 us       (back to back: the SGPR-operand v_xor after a v_bcnt costs a full 4 cycles)
//     v_xor ; s_nop 0 ; v_bcnt     324 us       v_xor ; s_nop ; v_bcnt ; s_nop   377 us
//     ... ; s_nop 1 / two s_nop 0 / s_nop 3 after the pair   316 / 317 / 314 us
// i.e. the v_bcnt must directly follow the v_xor that feeds it and ONE idle issue slot must follow the pair: then a
// pair issues in ~6.3 cycles instead of 8 (profiles/r01_valu_issue_rates.txt).  The compiler used to supply that
// s_nop by accident (it pads every asm statement with a hazard nop); it is spelled out here so that the pattern does
// not depend on it (an s_nop inside the three top-2 instructions, or the VOP3 encoding of the v_xor, changed nothing or
// cost 1-2 %).  The first v_bcnt accumulates onto the literal 0 (no v_mov to clear the accumulator).
#define K2NN_PAIR(t, q, accin) "v_xor_b32 %1, " t ", " q "\n\tv_bcnt_u32_b32 %0, %1, " accin "\n\ts_nop 0\n\t"

// words 0..7 of the row: the first half of either step
__device__ __forceinline__ uint32_t sweep_head(const uint32_t (&q)[16], const u32x4 a, const u32x4 b)
{
    uint32_t acc, tmp;
    asm volatile(K2NN_PAIR("%10", "%2", "0") K2NN_PAIR("%11", "%3", "%0") K2NN_PAIR("%12", "%4", "%0") K2NN_PAIR("%13", "%5", "%0")
                 K2NN_PAIR("%14", "%6", "%0") K2NN_PAIR("%15", "%7", "%0") K2NN_PAIR("%16", "%8", "%0") K2NN_PAIR("%17", "%9", "%0")
                 : "=&v"(acc), "=&v"(tmp)
                 : "v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]), "v"(q[4]), "v"(q[5]), "v"(q[6]), "v"(q[7]),
                   "s"(a.x), "s"(a.y), "s"(a.z), "s"(a.w), "s"(b.x), "s"(b.y), "s"(b.z), "s"(b.w));
    return acc;
}

// words 8..15.  Ungated: ONE asm statement holds the last 8 pairs together with the key and the med3 / min pair (the measured form).
// Gated: the pairs, then the key formed and gated in C++ behind them -- kEmpty where the gate says no -- in front of the med3 / min pair
// (LineGate: v_fma, v_fma, v_cmp, v_cndmask per pair, no branch; each reads at most one scalar operand, the one-SGPR rule of the gfx9
// vector ALU, so no v_mov copies a scalar into the loop).  g: the gate's floats of the lane's queries, p: the train row's point, lim: the
// gate's limit (none of them read without a gate).
template <int R, class Gate>
__device__ __forceinline__ void sweep_one(const uint32_t (&q)[R][16], const float (&g)[R][kGateF<Gate>], const u32x4 a, const u32x4 b, const u32x4 c,
                                          const u32x4 d, const u32x2 p, const float lim, const uint32_t t_rel, uint32_t (&best)[R], uint32_t (&second)[R])
{
    [[maybe_unused]] const float x = __uint_as_float(p.x), y = __uint_as_float(p.y);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t acc = sweep_head(q[r], a, b), tmp;
        if constexpr (Gate::kF == 0) {
            asm volatile(K2NN_PAIR("%12", "%4", "%0") K2NN_PAIR("%13", "%5", "%0") K2NN_PAIR("%14", "%6", "%0") K2NN_PAIR("%15", "%7", "%0")
                         K2NN_PAIR("%16", "%8", "%0") K2NN_PAIR("%17", "%9", "%0") K2NN_PAIR("%18", "%10", "%0") K2NN_PAIR("%19", "%11", "%0")
                         "v_lshl_add_u32 %1, %0, 22, %20\n\tv_med3_u32 %3, %2, %3, %1\n\tv_min_u32 %2, %2, %1"
                         : "+v"(acc), "=&v"(tmp), "+v"(best[r]), "+v"(second[r])
                         : "v"(q[r][8]), "v"(q[r][9]), "v"(q[r][10]), "v"(q[r][11]), "v"(q[r][12]), "v"(q[r][13]), "v"(q[r][14]), "v"(q[r][15]),
                           "s"(c.x), "s"(c.y), "s"(c.z), "s"(c.w), "s"(d.x), "s"(d.y), "s"(d.z), "s"(d.w), "s"(t_rel));
        } else {
            asm volatile(K2NN_PAIR("%10", "%2", "%0") K2NN_PAIR("%11", "%3", "%0") K2NN_PAIR("%12", "%4", "%0") K2NN_PAIR("%13", "%5", "%0")
                         K2NN_PAIR("%14", "%6", "%0") K2NN_PAIR("%15", "%7", "%0") K2NN_PAIR("%16", "%8", "%0") K2NN_PAIR("%17", "%9", "%0")
                         : "+v"(acc), "=&v"(tmp)
                         : "v"(q[r][8]), "v"(q[r][9]), "v"(q[r][10]), "v"(q[r][11]), "v"(q[r][12]), "v"(q[r][13]), "v"(q[r][14]), "v"(q[r][15]),
                           "s"(c.x), "s"(c.y), "s"(c.z), "s"(c.w), "s"(d.x), "s"(d.y), "s"(d.z), "s"(d.w));
            uint32_t key = (acc << kKeyShift) + t_rel;
            key = Gate::pass(g[r], x, y, lim) ? key : kEmpty;
            second[r] = top2_med3(best[r], second[r], key);
            best[r] = top2_min(best[r], key);
        }
    }
}
#undef K2NN_PAIR

// ---- one workgroup's split ----------------------------------------------------------------------------------------------------------
// where a workgroup stands in its job and what wave 0 holds of it behind sweep_split
template <int R> struct SweepSplit {
    uint32_t qblock, split;      // blockIdx.x = qblock * splits + split
    uint32_t lane, qbase;        // the lane's first query row (its r-th is qbase + 64 r)
    uint32_t s0;                 // first train row of the split: the keys' index field is relative to it
    uint32_t best[R], second[R];
};

// One workgroup's (query block, split) of the 2-D decomposition, in four parts: the lane's query rows into registers, the wave's share of
// the split, the pipelined loop over it, the fold of the waves through LDS.  False for a workgroup past the job's grid and for waves
// 1 .. kWaves - 1, which are done; true for wave 0, which holds the split's {best, second} of its lane's R queries in sp, keys relative
// to sp.s0.  job_nq / job_nt: the LIVE counts, as the kernel's record states them.
// (The four parts are ONE function on purpose, and the running pairs are its locals: a callee is optimised on its own before it is
// inlined, where the loop's bounds are not known to be wave-uniform.  With the loop in a function of its own its counter ended up in a
// VGPR; with the query load in one, or the pairs kept in sp, the line gate's arithmetic was packed across the lane's two queries and
// moved in between the xor / popcount pairs.)
template <int R, class Gate, class Job>
__device__ __forceinline__ bool sweep_split(const Job& job, const uint32_t job_nq, const uint32_t job_nt, SweepSplit<R>& sp)
{
    constexpr bool kGated = Gate::kF != 0;
    __shared__ uint32_t s_best[kWaves - 1][R][64], s_second[kWaves - 1][R][64];
    // XCD-aware tile order.  Workgroups go to the 8 XCDs round-robin by linear id and every XCD has its own L2.
    // The planner makes `splits` a multiple of 8 (and with it gridDim.x), so XCD x only ever sees the train splits
    // with (split & 7) == x: each L2 holds an eighth of T plus the queries, the 8 L2s together pull 8 Q + T from HBM
    // instead of 8 (Q + T), and every XCD gets exactly the same number of workgroups.  (A 2 x 4 arrangement -- half
    // of Q, a quarter of T per XCD -- fetches less still but leaves the XCDs 8 % out of balance at 79 query blocks
    // x 78 splits: measured 2 % slower.)
    const uint32_t nblk = job.qblocks * job.splits;
    if (blockIdx.x >= nblk) return false;
    const uint32_t qblock = blockIdx.x / job.splits;
    const uint32_t split = blockIdx.x - qblock * job.splits;

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t qbase = qblock * (64u * R) + lane;

    // the lane's R query rows, and the gate's floats of each
    uint32_t q[R][16];
    float g[R][kGateF<Gate>];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t qi = qbase + 64u * r;
        if (qi >= job_nq) qi = job_nq ? job_nq - 1u : 0u;   // clamp: duplicate work, never stored (row 0 of the block always exists)
        const global_cu4_ptr qp = (global_cu4_ptr)(uintptr_t)job.q + (size_t)qi * 4u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32x4 v = qp[k];
            q[r][4 * k + 0] = v.x; q[r][4 * k + 1] = v.y; q[r][4 * k + 2] = v.z; q[r][4 * k + 3] = v.w;
        }
        if constexpr (kGated) {
            const global_cf_ptr lp = (global_cf_ptr)(uintptr_t)job.L + (size_t)qi * (size_t)Gate::kF;
#pragma unroll
            for (int k = 0; k < Gate::kF; ++k) g[r][k] = lp[k];
        }
    }
    uint32_t best[R], second[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { best[r] = kEmpty; second[r] = kEmpty; }
    float lim = 0.f;                                        // the gate's limit
    if constexpr (kGated) lim = job.band;

    // this wave's share [t0, t1) of the workgroup's split [s0, s1)
    const uint32_t s0 = min(split * job.t_per_split, job_nt);
    const uint32_t s1 = min(s0 + job.t_per_split, job_nt);
    const uint32_t per_wave = (s1 - s0 + kWaves - 1) / kWaves;
    const uint32_t t0 = min(s0 + wave * per_wave, s1);
    const uint32_t t1 = min(t0 + per_wave, s1);

    // Software-pipelined scalar loads: wait for the CURRENT train vector, immediately issue the
    // s_load_dwordx16 of the NEXT one, then run the 70 VALU ops of the current one while it is in
    // flight.  (Left to itself the compiler issues the load and waits for it at the loop top; the
    // explicit order is worth ~11 % at 8 waves/SIMD.)  A gate's train point rides beside the train row in both buffers: one
    // s_load_dwordx2 beside the s_load_dwordx16, a vector ahead.  Neither prefetch reads past the slice.
    // Keys carry the index relative to s0 (the workgroup's split), so the waves' results merge by key.
    const_u4_ptr tp = (const_u4_ptr)(uintptr_t)job.t + (size_t)t0 * 4u;   // wave-uniform -> s_load_dwordx16
    [[maybe_unused]] const_u2_ptr pp = nullptr;
    if constexpr (kGated) pp = (const_u2_ptr)(uintptr_t)job.pos + (size_t)t0;      // wave-uniform -> s_load_dwordx2
    if (t0 < t1) {
        // two SGPR buffers used alternately (no register copies: the scalar ALU is shared by the CU and
        // 16 s_mov per train vector made it the bottleneck); an odd tail vector is handled after the loop
        const uint32_t n = t1 - t0;
        u32x4 a0 = tp[0], b0 = tp[1], c0 = tp[2], d0 = tp[3];
        u32x2 p0 = { 0u, 0u };
        if constexpr (kGated) p0 = pp[0];
        uint32_t t = t0;
        for (uint32_t pair = 0; pair < (n >> 1); ++pair, t += 2) {
            __builtin_amdgcn_s_waitcnt(0xC07F);                 // lgkmcnt(0): buffer 0 (vector t) has landed
            __builtin_amdgcn_sched_barrier(0);
            const u32x4 a1 = tp[4], b1 = tp[5], c1 = tp[6], d1 = tp[7];          // vector t+1 -> buffer 1
            u32x2 p1 = { 0u, 0u };
            if constexpr (kGated) p1 = pp[1];
            __builtin_amdgcn_sched_barrier(0);
            sweep_one<R, Gate>(q, g, a0, b0, c0, d0, p0, lim, t - s0, best, second);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);                 // buffer 1 has landed
            __builtin_amdgcn_sched_barrier(0);
            const bool more = t + 2 < t1;                       // vector t+2 -> buffer 0 (never past the slice)
            const_u4_ptr np = more ? tp + 8 : tp;
            [[maybe_unused]] const_u2_ptr npp = more ? pp + 2 : pp;
            a0 = np[0]; b0 = np[1]; c0 = np[2]; d0 = np[3];
            if constexpr (kGated) p0 = npp[0];
            __builtin_amdgcn_sched_barrier(0);
            sweep_one<R, Gate>(q, g, a1, b1, c1, d1, p1, lim, t + 1 - s0, best, second);
            __builtin_amdgcn_sched_barrier(0);
            tp += 8;
            if constexpr (kGated) pp += 2;
        }
        if (n & 1u) sweep_one<R, Gate>(q, g, a0, b0, c0, d0, p0, lim, t - s0, best, second);
    }

    // fold the kWaves waves through LDS: keys are unique and totally ordered, so
    // (b, s) (+) (b', s') = (min(b, b'), min(max(b, b'), s, s')) in any order
    if (wave != 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) { s_best[wave - 1][r][lane] = best[r]; s_second[wave - 1][r][lane] = second[r]; }
    }
    __syncthreads();
    if (wave != 0) return false;
#pragma unroll
    for (int w = 0; w < kWaves - 1; ++w) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t ob = s_best[w][r][lane], os = s_second[w][r][lane];
            second[r] = min(min(second[r], os), max(best[r], ob));
            best[r] = min(best[r], ob);
        }
    }
    sp.qblock = qblock; sp.split = split; sp.lane = lane; sp.qbase = qbase; sp.s0 = s0;
#pragma unroll
    for (int r = 0; r < R; ++r) { sp.best[r] = best[r]; sp.second[r] = second[r]; }
    return true;
}

// ---- the atomic fold of a split, the arrival counter, the finalize ------------------------------------------------------------------
// Fold one split's {bkey, skey} of query qi (bkey != kEmpty) into the query's global top-2 row with two 32-bit atomicMin.  Keys carry the
// GLOBAL train index here (s0 + index in split < 2^22), so unsigned order on keys is the total
// order (distance, index) and the fold is commutative: whichever value leaves the `best` slot
// (because a smaller key arrived) is offered to `second` by the arrival that displaced it.
// Returns what the atomics returned: the caller waits on it before it counts its workgroup in (below).
__device__ __forceinline__ uint32_t top2_row_fold(unsigned int* top, const uint32_t qi, const uint32_t bkey, const uint32_t skey)
{
    const uint32_t old = atomicMin(top + 2u * qi, bkey);
    const uint32_t cand = bkey < old ? min(old, skey) : bkey;
    uint32_t seen = old;
    if (cand != kEmpty) seen |= atomicMin(top + 2u * qi + 1u, cand);
    return seen;
}

// Wave 0 behind sweep_split, atomic mode: fold the split into the queries' global top-2 rows, count the workgroup in, and -- the last
// arrival of a query block only -- turn the rows into results and re-arm them.
template <int R, bool RATIO, class Job>
__device__ __forceinline__ void sweep_fold_finalize(const Job& job, const uint32_t job_nq, uint2* __restrict__ partial, const SweepSplit<R>& sp)
{
    unsigned int* top = reinterpret_cast<unsigned int*>(partial + job.partial_off);
    uint32_t seen = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t qi = sp.qbase + 64u * r;
        if (qi < job_nq && sp.best[r] != kEmpty) {
            const uint32_t bkey = sp.best[r] + sp.s0;
            const uint32_t skey = sp.second[r] == kEmpty ? kEmpty : sp.second[r] + sp.s0;
            seen |= top2_row_fold(top, qi, bkey, skey);
        }
    }
    // Arrival counter of this query block (armed at all-ones like the rows, so the n-th arrival reads n - 2).
    // Every atomic above RETURNS a value and the wave waits for all of them (vmcnt(0)), i.e. they have been
    // performed at the memory side -- agent-scope atomics bypass the XCD-local L2 -- before lane 0 counts this
    // workgroup in.  Whoever arrives last therefore knows every split has been folded and turns the rows into
    // results; rows and counter are read AND re-armed by atomic exchange, so no cached copy is ever consulted.
    // (A __threadfence() here would be the textbook release, but its L2 write-back + invalidate per workgroup
    // evicts the train slices the other workgroups are streaming: measured +50 % on the whole sweep.)
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(seen) : : "memory");
    unsigned int* cnt = reinterpret_cast<unsigned int*>(partial) + job.cnt_off + sp.qblock;
    uint32_t arrival = 0;
    if (sp.lane == 0) arrival = atomicAdd(cnt, 1u) + 1u;
    arrival = __builtin_amdgcn_readfirstlane(arrival);
    if (arrival != job.splits - 1u) return;
    if (sp.lane == 0) atomicExch(cnt, kEmpty);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t qi = sp.qbase + 64u * r;
        if (qi < job.nq) {          // every PLANNED row gets an answer; rows past a device-side count hold no key -> -1
            const uint32_t bkey = atomicExch(top + 2u * qi, kEmpty);
            const uint32_t skey = atomicExch(top + 2u * qi + 1u, kEmpty);
            emit_result<RATIO>(job, qi, bkey, skey);
        }
    }
}

} // namespace clc
#endif

// k2nn.hip -- brute-force 2-NN matcher for 512-bit descriptors on gfx950 (MI355X).
//
// Semantics: reference src/CUDAK2NN.cu:46-75 (per query: running best / second-best Hamming
// distance over all train vectors in index order, accept iff second - best > threshold, ties for
// the minimum keep the lowest train index).  The ARCHITECTURE is not the reference's (a 1-D grid of
// 256 queries per block, 40 blocks at 10k queries, CUDAK2NN.cu:79, around a 32-lane shuffle butterfly).
//
// Two formulations of the same sweep live here; both produce the same {best_key, second_key} rows and share the
// in-launch finalize (atomic fold + arrival counter) and the slab/merge fallback.  Selected per context
// (CLC_K2NN_FORMULATION=popcount|matrix, default matrix); the tests run both against the oracle.
//
// (A) matrix pipe -- k2nn_sweep_mx_kernel (default).  d(q, t) = (512 - <q, t>) / 2 with bits as +-1.
//   v_mfma_scale_f32_32x32x64_f8f6f4 takes FP4 (E2M1) operands, 64 k-values per instruction, in the cycles of the bf16
//   32x32x16 form: 8 MFMAs give the 1024 distances of a 32-train x 32-query tile, 0.25 cycles per comparison per SIMD
//   against ~1.8 for the popcount form.  Everything stays exact:
//     query bit b -> nibble 0x2 | b << 3 (+1 / -1), train bit b -> nibble 0x2 | ~b << 3 (-1 / +1): sum = 2 d - 512;
//     the A (train) operand carries the E8M0 block scale 2^12 and C = 2^23 + 2^21 + (train index inside the split,
//     < 8192), so the accumulator is 2^23 + (d << 13) + index: an integer below 2^24, exact in fp32 in any order, whose
//     FLOAT BITS 0x4B000000 + (d << 13) + index are already the (distance, index) key, ordered like the floats.
//   Top-2 per query = three-input min / med instructions on the raw accumulator registers (lane = query column, the 16
//   accumulator registers = 16 train rows; the network of k2nn_top2.h, 21 per chain); no key-forming instruction.  Descriptors stay in their 64-byte bit form in memory:
//   a wave expands its 64 queries into B operands once (registers), the workgroup expands each 32-train tile into
//   LDS (coalesced 8-byte loads, 7 VALU ops per 16 bytes of FP4) for its four waves.
//
// (B) popcount -- k2nn_sweep_kernel (round 1's kernel, kept as the measured A/B reference; its body is k2nn_sweep.h, which the gated
//   sweeps of k2nn_guided.hip run as well):
//
//   * lane = query.  Each lane keeps R complete 512-bit queries in VGPRs (16 dwords each), so a
//     distance needs NO cross-lane traffic at all.
//   * the train vector is wave-uniform: it is fetched with ONE scalar load (s_load_dwordx16, 64 B)
//     into SGPRs and used directly as the scalar operand of v_xor_b32 -- no LDS, no VGPRs, no
//     vector-memory instructions in the inner loop; the load of vector t+1 is issued before the
//     VALU work on vector t (explicit double buffer in SGPRs).  Per (query, train) pair the VALU executes
//     16 x (v_xor_b32 + v_bcnt_u32_b32 with accumulate) = 32 lane-ops.
//   * every v_xor is directly followed by the v_bcnt that consumes it (one asm statement per word).
//   * top-2 without branches or an index register: key = (distance << 22) | train_index_in_split.
//     Unsigned order on keys is (distance, index) lexicographic, so best' = min(best, key) keeps
//     the lowest index among equal distances, and second' = med3(best, second, key) is the second
//     smallest key = the second smallest distance of the multiset.  3 more lane-ops per pair.
//
// Both: 2-D decomposition (query block) x (train split) so that 10k x 10k fills 256 CUs (the reference's 1-D grid
//     would be 40 blocks).  Splits are folded into one {best_key, second_key} row per query with two
//     atomicMin (keys carry the global train index, so the fold is order-free and exact -- the
//     merge rule of SURVEY.md 8(a) note N1 with "lowest index wins" built into the key order); the
//     workgroup whose arrival completes a query block (a per-block arrival counter) applies the threshold,
//     writes the int32 results and re-arms rows and counter -- no second launch, no spinning.
//     Train sets beyond 2^22 vectors fall back to per-split slabs + an ordered merge kernel.
#include "clc_internal.h"
#include "k2nn_sweep.h"      // the popcount sweep's body, the key layout, the pointer types, accept / emit_result
#include "k2nn_top2.h"
#include <algorithm>

namespace clc {

// matrix-pipe formulation
static constexpr int kMxQT = 2;                          // 32-query tiles per wave (B operands: 32 VGPRs each)
static constexpr int kMxWaves = 4;                       // waves per workgroup; they share the train tiles through LDS
static constexpr int kMxQPerBlock = 32 * kMxQT * kMxWaves;
static constexpr uint32_t kMxIdxBits = 13;               // train index inside a split rides in the accumulator: splits <= 8192 rows
static constexpr uint32_t kMxMaxSplit = 1u << kMxIdxBits;
static constexpr uint32_t kMxMagic = 0x4B000000u;        // float bits of 2^23
static constexpr uint32_t kMxInf = 0x7F800000u;          // "no key yet": above every accumulator value
static constexpr uint32_t kMxResident = 3;               // workgroups of the matrix sweep a CU holds (152 VGPRs x 4 waves, 19.5 KB of LDS)
static_assert((kK2nnXcds & (kK2nnXcds - 1u)) == 0u && kK2nnXcds == 8u, "k2nn_sweep_mx_kernel's id -> (query block, split) map is written with & 7 / >> 3");
// per-XCD unequal-share table entry (K2nnJobList.bias_tab, bias_magic == 0): query block of the XCD in bits 0..4 (at most 32 per XCD),
// first train tile in bits 5..22 (2^18 tiles = 2^23 rows: above the 2^22 rows of the atomic fold), train tiles in bits 23..31 (a
// split holds at most 256 tiles, the 13-bit index inside a split).  k2nn_plan refuses the plan when a field would not hold its value.
static constexpr uint32_t kBiasQlBits = 5, kBiasQlMask = (1u << kBiasQlBits) - 1u;
static constexpr uint32_t kBiasBeginShift = kBiasQlBits, kBiasBeginBits = 18, kBiasBeginMask = (1u << kBiasBeginBits) - 1u;
static constexpr uint32_t kBiasSizeShift = kBiasBeginShift + kBiasBeginBits, kBiasSizeMax = (1u << (32u - kBiasSizeShift)) - 1u;
static_assert(kBiasSizeMax >= kMxMaxSplit / 32u, "a split of 256 tiles must fit the size field");
static_assert(((kIdxMask + 1u) >> 5) <= kBiasBeginMask + 1u, "every tile of an atomically folded train set must fit the begin field");

int k2nn_queries_per_block(int formulation) { return formulation == K2NN_POPCOUNT ? kQPerBlock : kMxQPerBlock; }

// The plain popcount sweep: the one body of k2nn_sweep.h without a gate.  The kernel's own: K2nnJobDev and its live counts (k2nn_job_nq
// with q_row0, k2nn_job_nt), the acceptance rule it is compiled for, and the slab rows of a plan without the atomic fold.
template <int R, bool RATIO = false>
__global__ __launch_bounds__(64 * kWaves) void k2nn_sweep_kernel(const K2nnJobList jobs,
                                                                  uint2* __restrict__ partial)
{
    const K2nnJobDev& job = jobs.j[blockIdx.y];
    const uint32_t job_nq = k2nn_job_nq(job), job_nt = k2nn_job_nt(job);     // == job.nq / job.nt unless the counts live on the device
    SweepSplit<R> sp;
    if (!sweep_split<R, NoGate>(job, job_nq, job_nt, sp)) return;
    if (job.atomic_merge) {
        sweep_fold_finalize<R, RATIO>(job, job_nq, partial, sp);
        return;
    }
    const global_u2_ptr prow = (global_u2_ptr)(uintptr_t)partial + job.partial_off + (size_t)sp.split * job.nq_pad;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t qi = sp.qbase + 64u * r;
        if (qi < job.nq) prow[qi] = qi < job_nq ? u32x2{ sp.best[r], sp.second[r] } : u32x2{ kEmpty, kEmpty };
    }
}

// ---- (A) matrix-pipe sweep ---------------------------------------------------------------------------------------
typedef int mx_v4i __attribute__((ext_vector_type(4)));
typedef int mx_v8i __attribute__((ext_vector_type(8)));
typedef float mx_v16f __attribute__((ext_vector_type(16)));
typedef const uint32_t __attribute__((address_space(1)))* global_cu32_ptr;
typedef const u32x2 __attribute__((address_space(1)))* global_cu2_ptr;

// 32 descriptor bits -> 32 FP4 nibbles 0x2 | bit << 3 (+1.0 / -1.0).  Nibble k of dword m holds bit 4 k + m: the
// k order inside a row is arbitrary as long as queries and trains use the same one.
__device__ __forceinline__ u32x4 mx_expand(const uint32_t x)
{
    u32x4 y;
    y.x = ((x << 3) & 0x88888888u) | 0x22222222u;
    y.y = ((x << 2) & 0x88888888u) | 0x22222222u;
    y.z = ((x << 1) & 0x88888888u) | 0x22222222u;
    y.w = (x & 0x88888888u) | 0x22222222u;
    return y;
}
// the same for the COMPLEMENT of x, written so that each output is one shift + one three-input bit op (v_bitop3_b32):
// complementing first and shifting the complement costs a v_not and separate and / or per output (22 instead of 14
// instructions for the 8 train bytes a thread expands per tile)
__device__ __forceinline__ u32x4 mx_expand_not(const uint32_t x)
{
    u32x4 y;
    y.x = (~(x << 3) & 0x88888888u) | 0x22222222u;
    y.y = (~(x << 2) & 0x88888888u) | 0x22222222u;
    y.z = (~(x << 1) & 0x88888888u) | 0x22222222u;
    y.w = (~x & 0x88888888u) | 0x22222222u;
    return y;
}
// Keys are positive finite floats, "none" is +inf: float order == unsigned order of the bits, and the top-2 network (k2nn_top2.h) runs on
// the bits.  Plain C++ min / max nests there, NOT inline asm: the compiler pads the MFMA-result -> VALU-read hazard only for instructions
// it can see (an asm v_med3_u32 placed straight after the last MFMA of a tile read the PREVIOUS tile's accumulator register).

// accumulator bits -> the canonical key (distance << 22) | (t0 + index in split); kEmpty for "none" and for the
// penalised padding rows of a partial last tile (their distance field is above 512)
__device__ __forceinline__ uint32_t mx_decode(const uint32_t bits, const uint32_t t0)
{
    const uint32_t rel = bits - kMxMagic;
    const uint32_t d = rel >> kMxIdxBits;
    if (bits == kMxInf || d > 512u) return kEmpty;
    return (d << kKeyShift) | (t0 + (rel & (kMxMaxSplit - 1u)));
}

// the same for a key whose index field is relative to `end` (the row behind the split): value = 2^23 + (distance << 13) + rel,
// rel in [-8192, -1].  Through the float VALUE, not its bits: with distance 0 the value lies below 2^23, where floats step by 0.5.
__device__ __forceinline__ uint32_t mx_decode_rel(const uint32_t bits, const uint32_t end)
{
    if (bits == kMxInf) return kEmpty;
    const int v = (int)__uint_as_float(bits) - 8388608 + (int)kMxMaxSplit;          // (distance << 13) + rel + 8192, >= 0
    const uint32_t d = (uint32_t)v >> kMxIdxBits;
    if (d > 512u) return kEmpty;
    return (d << kKeyShift) | (end - kMxMaxSplit + ((uint32_t)v & (kMxMaxSplit - 1u)));
}

// STAMP: diagnostic build for the clock check (MI355X guide, DVFS item 6): lane 0 of every workgroup brackets its tile loop
// with s_memtime (shader clock) / s_memrealtime (constant 100 MHz) and stores them, with its entry / folded-in times and its
// XCC id (tools/archive/k2nn_timeline.py), in a buffer nothing else reads.  The product kernel (STAMP = false) contains no stamp.
//
// The loop (round 3): the two 32-query tiles of a wave are swept as two MFMA chains of eight, one after the other, and the
// running top-2 of a chain's accumulators is updated in the shadow of the NEXT chain's MFMAs (sched_group_barrier spells the
// interleave out: one MFMA, one A-operand read, five vector instructions).  No second accumulator set is needed -- chain 1 of tile
// t covers the top-2 of chain 0 of tile t, chain 0 of tile t + 1 covers the top-2 of chain 1 of tile t -- so the kernel keeps its
// three waves per SIMD; the price is that every A operand is read from LDS twice.  (Round 2's loop -- k-step outer, both chains per
// A read, then all 64 v_med3 -- was kept as an A/B formulation through round 5: profiles/r06_removed_variants.patch.)
// PROBE: the same code under another symbol, for the launches of the per-device share probe at context creation (capi_match.hip k2nn_probe_bias):
// a kernel trace of an application then shows ITS sweeps under k2nn_sweep_mx_kernel<false, false, false> and the probe's -- run from cold
// clocks, under four different share pairs -- under <..., true>, instead of one average over both.
// RATIO: the acceptance rule of the launch's jobs (accept()).
template <bool STAMP, bool GLOBAL = false, bool PROBE = false, bool RATIO = false>
__global__ __launch_bounds__(64 * kMxWaves) void k2nn_sweep_mx_kernel(const K2nnJobList jobs, uint2* __restrict__ partial,
                                                                      uint64_t* __restrict__ stamps)
{
    constexpr int QT = kMxQT;
    constexpr int kStride = 65;      // uint4 per k-step of a train tile in LDS: 64 lanes + 1 pad, so that the 8 k-steps
                                     // one row is expanded into land in different banks (ds_write_b128, 8 lanes per pass)
    constexpr int kQRow = 17;        // dwords per staged query row: 16 + 1 pad -> the 32 rows a half-wave reads hit 32 banks
    constexpr int kStageDw = kMxWaves * QT * 32 * kQRow;
    constexpr int kTileDw = 2 * 8 * kStride * 4;
    // one buffer, two lives: the prologue stages the raw query rows in it (per wave), the loop keeps the expanded train tiles
    __shared__ __attribute__((aligned(16))) uint32_t s_mem[kStageDw > kTileDw ? kStageDw : kTileDw];
    u32x4 (*s_a)[8 * kStride] = reinterpret_cast<u32x4 (*)[8 * kStride]>(s_mem);
    __shared__ uint32_t s_best[kMxQPerBlock], s_second[kMxQPerBlock];
    __shared__ uint32_t s_arrival;
    const K2nnJobDev& job = jobs.j[blockIdx.y];
    const uint32_t job_nq = k2nn_job_nq(job), job_nt = k2nn_job_nt(job);     // == job.nq / job.nt unless the counts live on the device
    uint64_t st_entry = 0;
    if (STAMP) st_entry = __builtin_amdgcn_s_memrealtime();
    // XCD-aware order (speed only): workgroups are dealt to the 8 XCDs round-robin by linear id, each XCD has its own
    // L2.  Workgroup L works on query block (L & 7) + 8 ((L >> 3) / splits): every split of a query block lands on ONE
    // XCD, so an XCD's L2 pulls an eighth of the queries plus the train set instead of all of both (PMC, 10k x 10k:
    // 10.1 MB fetched with the plain order = 8 x (Q + T)).  The grid is padded to a multiple of 8 query blocks.
    const uint32_t within = blockIdx.x >> 3;
    const bool biased = job.bias_a != 0u;
    // biased shares: the query blocks of an XCD are INTERLEAVED over its workgroups (query block = within % nqx), so that every query
    // block has splits on all three wave slots (blocked, as below, the 19 splits of a query block sit on one slot)
    // ... when the query blocks come in whole eights.  Otherwise (bias_magic != 0) they are interleaved over ALL workgroup ids -- query block =
    // id % qblocks, split = id / qblocks, nothing padded, a query block's splits spread over the XCDs: measured 0.8-1.5 us faster than the
    // padded per-XCD order for 36 / 34 / 28 / 47 query blocks, 0.8-1.4 us slower than the per-XCD interleave for 40 / 32 / 24 (each L2 then
    // pulls both sets whole)
    // (a template parameter, not a run-time flag: with both orders in one instantiation the register allocator copied the sixteen C registers
    // in front of every chain -- 32 v_mov per tile, +0.7 us on the 10k x 10k sweep)
    constexpr bool global_order = GLOBAL;
    const uint32_t bias_k = global_order ? (uint32_t)__builtin_amdgcn_readfirstlane((int)__umulhi(blockIdx.x, job.bias_magic)) : 0u;   // (wave-uniform: keep it scalar)
    const uint32_t bias_q = blockIdx.x - bias_k * job.qblocks;
    const uint32_t bias_e = biased ? jobs.bias_tab[global_order ? (bias_q & 127u) : (within < 96u ? within : 95u)] : 0u;
    const uint32_t qblock = global_order ? bias_q
                          : (biased ? ((blockIdx.x + 8u - job.xcd_rot) & 7u) + 8u * (bias_e & kBiasQlMask)
                                    : ((blockIdx.x + 8u - job.xcd_rot) & 7u) + 8u * (within / job.splits));
    const uint32_t split = global_order ? bias_k : (biased ? (STAMP ? within / (job.qblocks >> 3) : 0u) : within % job.splits);
    if (qblock >= job.qblocks || (global_order && split >= job.splits) || (biased && !global_order && within >= (job.qblocks >> 3) * job.splits)) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // B operands: lane (row = l & 31, half h = l >> 5) holds the 32 k-values of words 2 j + h of its query row.
    // The wave's 64 rows are fetched with COALESCED 16-byte loads (4 KB = four wave instructions) and handed round
    // through the wave's own LDS staging area; every lane then picks its 8 words per tile.  (Each lane loading its own
    // words straight from memory -- 16 strided dword loads touching 32 cache lines per instruction -- took 11 k cycles
    // per wave, a quarter of the kernel, measured with in-kernel stamps: tools/archive/k2nn_mfma.hip.)
    mx_v4i b[QT][8];
    {
        uint32_t* stage = s_mem + wave * (QT * 32 * kQRow);
        const global_cu4_ptr qbase = (global_cu4_ptr)(uintptr_t)job.q;
#pragma unroll
        for (int i = 0; i < 2 * QT; ++i) {
            const uint32_t idx = (uint32_t)i * 64u + lane;               // 16-byte chunk of the wave's QT x 32 rows
            const uint32_t r_local = idx >> 2, chunk = idx & 3u;
            uint32_t row = qblock * kMxQPerBlock + wave * (QT * 32u) + r_local;
            if (row >= job_nq) row = job_nq ? job_nq - 1u : 0u;          // clamp: duplicate work, never stored (row 0 of the block always exists)
            const u32x4 v = qbase[(size_t)row * 4u + chunk];
            uint32_t* d = stage + r_local * kQRow + chunk * 4u;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            const uint32_t* src = stage + ((uint32_t)qt * 32u + (lane & 31u)) * kQRow + (lane >> 5);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const u32x4 v = mx_expand(src[2 * j]);
                b[qt][j] = mx_v4i{ (int)v.x, (int)v.y, (int)v.z, (int)v.w };
            }
        }
    }
    __syncthreads();                 // the staging area becomes the train-tile buffer
    // C of the first MFMA of a tile: 2^23 + 2^21 + index (inside the TILE) of the lane's 16 train rows; the same for every tile
    // (C/D layout of the 32x32 forms: column = lane & 31, row = 8 (reg >> 2) + 4 (lane >> 5) + (reg & 3))
    float cinit[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) cinit[i] = 8388608.0f + 2097152.0f + (float)(8 * (i >> 2) + 4 * (int)(lane >> 5) + (i & 3));
    uint32_t best[QT], second[QT];   // the running pairs, as key bits (k2nn_top2.h)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) { best[qt] = kMxInf; second[qt] = kMxInf; }

    // this workgroup's train rows [s0, s1): t_per_split is a multiple of 32, so only the train set's last tile can be partial
    uint32_t s0 = min(split * job.t_per_split, job_nt);
    uint32_t s1 = min(s0 + job.t_per_split, job_nt);
    if (biased && !global_order) {
        s0 = min(((bias_e >> kBiasBeginShift) & kBiasBeginMask) * 32u, job_nt);
        s1 = min(s0 + (bias_e >> kBiasSizeShift) * 32u, job_nt);
    }
    if (global_order) {
        // the query block's splits in id order: n0 on slot 0 with bias_a tiles each, n1 on slot 1 with bias_b, the rest on slot 2 with c
        // (the first `extra` of them c + 1) tiles; the last split ends with the train set
        const uint32_t n0 = bias_e & 0xFFu, n1 = (bias_e >> 8) & 0xFFu, c = (bias_e >> 16) & 0xFFu, extra = bias_e >> 24;
        const uint32_t k0 = min(split, n0), k1 = min(split - k0, n1), k2 = split - k0 - k1;
        const uint32_t begin = k0 * job.bias_a + k1 * job.bias_b + k2 * c + min(k2, extra);
        const uint32_t size = split < n0 ? job.bias_a : (split < n0 + n1 ? job.bias_b : c + (k2 < extra ? 1u : 0u));
        s0 = min(begin * 32u, job_nt);
        s1 = split + 1u == job.splits ? job_nt : min(s0 + size * 32u, job_nt);
    }
    if (global_order) {
        s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s0);
        s1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s1);
    }
    const uint32_t ntiles = (s1 - s0 + 31u) >> 5;
    const int scale_a = 0x8B8B8B8B, scale_b = 0x7F7F7F7F;            // E8M0 block scales: 2^12 (trains), 1 (queries)
    // train tile = 32 rows x 64 B = 2 KB contiguous: thread tid owns its 8 bytes number tid = row tid >> 3, words
    // 2 j', 2 j' + 1 (j' = tid & 7), i.e. both lane halves of k-step j' of that row
    const uint32_t my_row = tid >> 3, my_j = tid & 7u;
    const uint32_t dst = my_j * kStride + my_row;
    const global_cu2_ptr tbase = (global_cu2_ptr)(uintptr_t)job.t + (size_t)my_j;
    const uint32_t last_row = job_nt ? job_nt - 1u : 0u;             // in a register: read through `job` it is a scalar load
                                                                     // (+ wait) from the kernel arguments in every tile
    auto load_bits = [&](const uint32_t tile) -> u32x2 {
        const uint32_t row = min(s0 + tile * 32u + my_row, last_row);   // stays in bounds; such rows are penalised through C
        return tbase[(size_t)row * 8u];
    };
    u32x2 r0 = u32x2{ 0u, 0u }, r1 = u32x2{ 0u, 0u };
    if (ntiles) { r0 = load_bits(0u); r1 = load_bits(min(1u, ntiles - 1u)); }   // (an empty split -- device-side count -- reads nothing)
    mx_v16f acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = __uint_as_float(kMxInf); acc1[i] = __uint_as_float(kMxInf); }
    uint64_t st_clk = 0, st_real = 0;
    if (STAMP) { st_clk = __builtin_amdgcn_s_memtime(); st_real = __builtin_amdgcn_s_memrealtime(); }
    for (uint32_t t = 0; t < ntiles; ++t) {
        const uint32_t buf = t & 1u;
        s_a[buf][dst] = mx_expand_not(r0.x);
        s_a[buf][dst + 32] = mx_expand_not(r0.y);
        r0 = r1;
        __syncthreads();          // one barrier per tile: buffer `buf` was last read two iterations ago, before the previous barrier
        if (t + 2u < ntiles) r1 = load_bits(t + 2u);                // bits of the tile after next: in flight for a whole tile
        if (t + 1u == ntiles && ((s1 - s0) & 31u)) {
            // partial last tile: rows past the end get a penalty that puts their distance field above 512
            const uint32_t valid = (s1 - s0) & 31u;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if ((uint32_t)(8 * (i >> 2) + 4 * (int)(lane >> 5) + (i & 3)) >= valid) cinit[i] += 4194304.0f + 8192.0f;
        }
        static_assert(QT == 2, "the pipelined loop is written for two chains");
        // chain c of this tile (8 MFMAs) with the top-2 update of `prev` (the accumulators of the chain before it) in its shadow
        // sixteen steps: step s = MFMA j = s & 7 of chain s >> 3; the A operand of step s + kAhead is requested at step s (an LDS
        // read takes longer than one MFMA: with the next step's operand only, every MFMA waited for its read)
#ifndef CLC_K2NN_AHEAD
#define CLC_K2NN_AHEAD 3
#endif
        constexpr int kAhead = CLC_K2NN_AHEAD;
        u32x4 ring[kAhead];
        clc::Top2Wait wait;
#pragma unroll
        for (int k = 0; k < kAhead; ++k) ring[k] = s_a[buf][k * kStride + lane];
#pragma unroll
        for (int st = 0; st < 16; ++st) {
            const int c = st >> 3, j = st & 7;
            const u32x4 av = ring[st % kAhead];
            const mx_v8i a8 = { (int)av.x, (int)av.y, (int)av.z, (int)av.w, 0, 0, 0, 0 };
            const mx_v8i b8 = { b[c][j].x, b[c][j].y, b[c][j].z, b[c][j].w, 0, 0, 0, 0 };
            if (st + kAhead < 16) ring[st % kAhead] = s_a[buf][((st + kAhead) & 7) * kStride + lane];
            mx_v16f& acc = c ? acc1 : acc0;
            const mx_v16f& prev = c ? acc0 : acc1;       // chain 0 folds in chain 1 of the tile before, chain 1 folds in chain 0
            const int pq = c ? 0 : 1;
            mx_v16f ci;
            if (j == 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) ci[i] = cinit[i];
            } else ci = acc;
            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, ci, 4, 4, 0, scale_a, 0, scale_b);
            // step j of the fold of the chain before (k2nn_top2.h: 21 three-input instructions for its sixteen keys, three or fewer per
            // step), in this MFMA's shadow (32 cycles of matrix pipe, 8 of them holding the vector issue: four such instructions fit)
            uint32_t pk[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) pk[i] = __float_as_uint(prev[i]);
            clc::top2_fold16_step(j, best[pq], second[pq], wait, pk);
            // the step back of the chain just folded in: instead of advancing the index part of the sixteen C registers per tile, the
            // running pair steps BACK by one tile -- its index field is then relative to the tile about to be processed (negative for
            // the tiles behind; the integer stays exact in fp32, order and tie rule unchanged: a lower global index is a lower value)
            if (j == 7) { best[pq] = clc::top2_step_back(best[pq]); second[pq] = clc::top2_step_back(second[pq]); }
            __builtin_amdgcn_sched_barrier(0);                           // keep the groups in this order
        }
    }
    {                  // the last tile's second chain is still to be folded in
        uint32_t pk[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) pk[i] = __float_as_uint(acc1[i]);
        clc::top2_fold16(best[1], second[1], pk);
        best[1] = clc::top2_step_back(best[1]); second[1] = clc::top2_step_back(second[1]);
    }

    if (STAMP) {
        const uint64_t en_clk = __builtin_amdgcn_s_memtime(), en_real = __builtin_amdgcn_s_memrealtime();
        if (tid == 0) {
            uint64_t* o = stamps + 8u * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
            o[0] = st_clk; o[1] = st_real; o[2] = en_clk; o[3] = en_real; o[4] = st_entry;
        }
    }
    // lanes l and l ^ 32 hold the same query column (different train rows): fold them, decode to canonical keys with the
    // index relative to s0 (slab mode) or global (atomic mode), and hand the workgroup's 256 results over through LDS so
    // that thread i finishes query i of the block with coalesced rows
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const uint32_t mb = best[qt], ms = second[qt];
        const uint32_t ob = __shfl_xor(mb, 32), os = __shfl_xor(ms, 32);
        if (lane < 32u) {
            const uint32_t slot = (wave * QT + qt) * 32u + lane;
            // after the last tile's step back every index is relative to the row BEHIND the split: -(rows of the split) .. -1
            const uint32_t end = (job.atomic_merge ? s0 : 0u) + 32u * ntiles;
            s_best[slot] = mx_decode_rel(min(mb, ob), end);
            s_second[slot] = mx_decode_rel(min(min(ms, os), max(mb, ob)), end);
        }
    }
    __syncthreads();
    const uint32_t qi = qblock * kMxQPerBlock + tid;
    const uint32_t bkey_l = s_best[tid], skey_l = s_second[tid];
    if (!job.atomic_merge) {
        const global_u2_ptr prow = (global_u2_ptr)(uintptr_t)partial + job.partial_off + (size_t)split * job.nq_pad;
        if (qi < job.nq) prow[qi] = qi < job_nq ? u32x2{ bkey_l, skey_l } : u32x2{ kEmpty, kEmpty };
        return;
    }
    // same fold / arrival / finalize protocol as the popcount sweep (k2nn_sweep.h, sweep_fold_finalize: why no fence is needed).  The fold of
    // a row is shared (top2_row_fold); the arrival and the last arrival's exchanges are this kernel's own per-thread statement (behind
    // a shared function the instructions of this finalize changed order, and the kernel's text is held as it was): every
    // thread's atomics RETURN, every wave waits for them, the workgroup barrier joins the four waves, then one lane
    // counts the workgroup in; the last arrival of a query block turns the rows into results and re-arms them.
    unsigned int* top = reinterpret_cast<unsigned int*>(partial + job.partial_off);
    uint32_t seen = 0;
    if (qi < job_nq && bkey_l != kEmpty) seen = top2_row_fold(top, qi, bkey_l, skey_l);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(seen) : : "memory");
    __syncthreads();
    unsigned int* cnt = reinterpret_cast<unsigned int*>(partial) + job.cnt_off + qblock;
    if (tid == 0) s_arrival = atomicAdd(cnt, 1u) + 1u;
    __syncthreads();
    if (STAMP && tid == 0) {          // folded in: everything but the finalize of the last arrival
        uint64_t* o = stamps + 8u * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        o[5] = __builtin_amdgcn_s_memrealtime();
        o[6] = ((uint64_t)qblock << 32) | split;
        // XCC_ID[3:0] | HW_ID << 8 (wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13]: where on the chip this workgroup's wave 0 sits)
        o[7] = (uint64_t)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | ((4 - 1) << 11)) |
               ((uint64_t)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | ((32 - 1) << 11)) << 8);
    }
    if (s_arrival != job.splits - 1u) return;
    if (tid == 0) atomicExch(cnt, kEmpty);
    if (qi < job.nq) {
        const uint32_t bkey = atomicExch(top + 2u * qi, kEmpty);
        const uint32_t skey = atomicExch(top + 2u * qi + 1u, kEmpty);
        emit_result<RATIO>(job, qi, bkey, skey);
    }
}

// jobs with an EMPTY train set, atomic mode (nomatch_rows, k2nn_sweep.h)
__global__ __launch_bounds__(256) void k2nn_nomatch_kernel(const K2nnJobList jobs) { nomatch_rows(jobs); }

// Fold the per-split partials of one query and threshold.
// The merge of two partial results is associative as long as the left operand holds the lower
// train indices, so the splits of a query are folded by kMergeGroups threads in parallel (each a
// contiguous run of splits, loads issued 4 deep) and the group results are folded in order through
// LDS.  Reads stay coalesced: consecutive lanes own consecutive queries of one split row.
static constexpr int kMergeQ = 32;        // queries per workgroup
static constexpr int kMergeGroups = 8;    // split groups per query

struct Top2 { int best_v, second_v, best_i; };

__device__ __forceinline__ void fold(Top2& a, const uint32_t bk, const uint32_t sk, const uint32_t t0)
{
    if (bk == kEmpty) return;
    const int b_best = (int)(bk >> kKeyShift);
    const int b_idx = (int)(t0 + (bk & kIdxMask));
    const int b_second = sk == kEmpty ? 100000 : (int)(sk >> kKeyShift);
    if (b_best < a.best_v) {
        a.second_v = min(a.best_v, b_second);
        a.best_v = b_best;
        a.best_i = b_idx;
    } else {
        a.second_v = min(a.second_v, b_best);
    }
}

__global__ __launch_bounds__(kMergeQ * kMergeGroups) void k2nn_merge_kernel(const K2nnJobList jobs,
                                                                             const uint2* __restrict__ partial)
{
    __shared__ Top2 sh[kMergeGroups][kMergeQ];
    const K2nnJobDev& job = jobs.j[blockIdx.y];
    const uint32_t qx = threadIdx.x & (kMergeQ - 1);
    const uint32_t g = threadIdx.x / kMergeQ;
    const uint32_t qi = blockIdx.x * kMergeQ + qx;
    if (blockIdx.x * kMergeQ >= job.nq) return;                       // whole workgroup past the end
    const uint32_t nsplit = job.nt ? job.splits : 0u;                  // nt == 0: nothing was swept -> -1
    const uint32_t per_g = (nsplit + kMergeGroups - 1) / kMergeGroups;
    const uint32_t s0 = min(g * per_g, nsplit), s1 = min(s0 + per_g, nsplit);
    Top2 a{ 100000, 200000, -1 };                                      // CUDAK2NN.cu:54 sentinels
    if (qi < job.nq) {
        const uint2* p = partial + job.partial_off + (size_t)s0 * job.nq_pad + qi;
        uint32_t s = s0;
        for (; s + 4 <= s1; s += 4, p += 4 * (size_t)job.nq_pad) {
            const uint2 e0 = p[0], e1 = p[job.nq_pad], e2 = p[2 * (size_t)job.nq_pad], e3 = p[3 * (size_t)job.nq_pad];
            fold(a, e0.x, e0.y, s * job.t_per_split);
            fold(a, e1.x, e1.y, (s + 1) * job.t_per_split);
            fold(a, e2.x, e2.y, (s + 2) * job.t_per_split);
            fold(a, e3.x, e3.y, (s + 3) * job.t_per_split);
        }
        for (; s < s1; ++s, p += job.nq_pad) {
            const uint2 e = *p;
            fold(a, e.x, e.y, s * job.t_per_split);
        }
    }
    sh[g][qx] = a;
    __syncthreads();
    if (g != 0 || qi >= job.nq) return;
    for (int k = 1; k < kMergeGroups; ++k) {                           // in order: group k holds higher indices
        const Top2 b = sh[k][qx];
        if (b.best_i < 0) continue;
        if (b.best_v < a.best_v) {
            a.second_v = min(a.best_v, b.second_v);
            a.best_v = b.best_v;
            a.best_i = b.best_i;
        } else {
            a.second_v = min(a.second_v, b.best_v);
        }
    }
    const bool ok = job.rule == K2NN_RULE_RATIO ? accept<true>(job, a.best_i, a.best_v, a.second_v) : accept<false>(job, a.best_i, a.best_v, a.second_v);
    job.out[qi] = ok ? a.best_i : -1;
    if (job.best_out) job.best_out[qi] = (uint16_t)min(a.best_v, 65535);
    if (job.second_out) job.second_out[qi] = (uint16_t)min(a.second_v, 65535);
}

// Unequal shares by wave slot (K2nnJobDev.bias_a), the arithmetic of one query block, stated once for the plan's checks and the launch's
// tables.  Query block q of nq_blocks interleaved ones has its split k on workgroup k nq_blocks + q of the id space, and slot_wgs ids
// make a wave slot: n0 of its splits sit on slot 0 (a tiles each), n1 on slot 1 (b tiles), and the n2 on slot 2 share the rest of the
// nt_tiles, c tiles each, the first `extra` of them one more (c = extra = 0 where nothing is left or n2 == 0).
struct SlotShares { uint32_t n0, n1, n2, used, c, extra; };
static SlotShares slot_shares(const uint32_t slot_wgs, const uint32_t q, const uint32_t nq_blocks, const uint32_t splits, const uint32_t a, const uint32_t b,
                              const uint32_t nt_tiles)
{
    SlotShares s;
    s.n0 = std::min((slot_wgs - q + nq_blocks - 1u) / nq_blocks, splits);
    s.n1 = std::min((2u * slot_wgs - q + nq_blocks - 1u) / nq_blocks, splits) - s.n0;
    s.n2 = splits - s.n0 - s.n1;
    s.used = s.n0 * a + s.n1 * b;
    const uint32_t rest = nt_tiles > s.used ? nt_tiles - s.used : 0u;
    s.c = s.n2 ? rest / s.n2 : 0u;
    s.extra = s.n2 ? rest - s.c * s.n2 : 0u;
    return s;
}
// what k2nn_plan asks of every query block: a slot-2 split exists, the slot-0 and slot-1 splits lie inside the train set, every slot-2 split
// is within the 13-bit index field (256 tiles) and none is below the two tiles the equal plan guarantees (min_per)
static bool slot_shares_fit(const SlotShares& s, const uint32_t nt_tiles)
{
    return s.n2 >= 1u && s.used < nt_tiles && s.c + (s.extra ? 1u : 0u) <= 255u && s.c >= 2u;
}

K2nnPlan k2nn_plan(K2nnJobDev* jobs, int njobs, int target_blocks, bool xcd_map, int formulation, int bias_a, int bias_b, K2nnDevice dev)
{
    // Everything below that speaks of XCDs, CUs or wave slots takes the numbers from the DEVICE (hipDeviceAttributeNumberOfXccs,
    // multiProcessorCount; clc_ctx_create) -- rounds 3-4 had 8 / 32 / 768 written in.  The sweep kernel's workgroup -> (query block, split)
    // map is compiled for kK2nnXcds XCDs; it is a permutation of the work on any device, but the balance arguments (one XCD's share of the
    // slots, the slot a workgroup id lands on) only hold where the device has that many: elsewhere the plan keeps equal shares and skips
    // the per-XCD fit.
    const bool xcd_known = dev.n_xcd == kK2nnXcds && dev.n_cu % kK2nnXcds == 0u;
    const uint32_t cu_x = dev.n_cu / kK2nnXcds;                    // CUs of one XCD = workgroups per wave slot and XCD (32 on MI355X)
    const uint32_t slots = kMxResident * dev.n_cu;                // resident workgroups of the matrix sweep (768)

    const bool mx = formulation != K2NN_POPCOUNT;
    const uint32_t qpb = mx ? kMxQPerBlock : kQPerBlock;
    K2nnPlan plan{0, true};
    for (int j = 0; j < njobs; ++j)
        if (jobs[j].nt > kIdxMask + 1u) plan.atomic_merge = false;
    uint32_t total_qblocks = 0;
    for (int j = 0; j < njobs; ++j) {
        jobs[j].qblocks = (jobs[j].nq + qpb - 1) / qpb;
        total_qblocks += jobs[j].qblocks;
    }
    if (total_qblocks == 0) total_qblocks = 1;
    // popcount: about target_blocks workgroups, several rounds of them; matrix: at most target_blocks (= the resident
    // slots, 3 workgroups per CU), so that the whole grid runs as ONE round -- a partial second round costs a full
    // round's time at a fraction of the machine
    uint32_t want = mx ? (uint32_t)target_blocks / total_qblocks : ((uint32_t)target_blocks + total_qblocks - 1) / total_qblocks;
    if (mx) {
        // Every split of a query block runs on ONE XCD (the kernel's XCD-aware order), so the round must also fit per XCD: an eighth
        // of the slots against the most query blocks any XCD takes.  34 query blocks (8.5 k queries) at 768 / 34 = 22 splits put
        // 5 x 22 = 110 workgroups on the 96 slots of XCDs 0 and 1 -- a second round there, measured 33 us instead of 26 for such a
        // grid.  Jobs continue round the XCDs where the previous one stopped (xcd_rot), so the maximum is ceil(total / 8).
        const uint32_t per_xcd = (total_qblocks + kK2nnXcds - 1u) / kK2nnXcds;
        const uint32_t fit = (uint32_t)target_blocks / kK2nnXcds / per_xcd;
        if (xcd_known && fit < want) want = fit;
    }
    if (want < 1) want = 1;
    size_t off = 0;
    uint32_t rot = 0;
    for (int j = 0; j < njobs; ++j) {
        K2nnJobDev& jb = jobs[j];
        jb.xcd_rot = mx ? rot : 0u;
        rot = (rot + jb.qblocks) & (kK2nnXcds - 1u);
        uint32_t splits = want;
        // popcount: >= 16 train vectors per wave; matrix: >= 2 tiles of 32 per workgroup
        const uint32_t min_per = mx ? 64u : 16u * kWaves;
        const uint32_t max_splits = jb.nt / min_per > 0 ? jb.nt / min_per : 1u;
        if (splits > max_splits) splits = max_splits;
        // popcount: a multiple of 8 splits pins train split s to XCD s & 7 (see that kernel).  The matrix kernel reads the
        // 64-byte rows themselves (a 10k-row set is 640 KB: every XCD's L2 holds all of it), so it keeps the exact count.
        if (!mx && xcd_map && splits >= 8u) splits = (splits + 4u) / 8u * 8u > max_splits ? splits / 8u * 8u : (splits + 4u) / 8u * 8u;
        uint32_t per = jb.nt ? (jb.nt + splits - 1) / splits : 1u;
        if (mx) {
            per = (per + 31u) & ~31u;                                     // whole tiles of 32 train rows
            if (per > kMxMaxSplit) per = kMxMaxSplit;                     // 13-bit index inside a split (in the accumulator)
        }
        if (per > kIdxMask + 1u) per = kIdxMask + 1u;                     // index field is 22 bits
        splits = jb.nt ? (jb.nt + per - 1) / per : 1u;
        jb.splits = splits;
        jb.t_per_split = per;
        jb.bias_a = jb.bias_b = jb.bias_magic = 0u;
        jb.slot_wgs = 0u;
        jb.nq_pad = (jb.nq + 63u) & ~63u;
        jb.partial_off = (uint32_t)off;
        jb.atomic_merge = plan.atomic_merge ? 1u : 0u;
        off += plan.atomic_merge ? (size_t)jb.nq_pad : (size_t)splits * jb.nq_pad;
        if (plan.atomic_merge) {                                          // arrival counters: one uint32 per query block
            jb.cnt_off = (uint32_t)(2u * off);
            off += (jb.qblocks + 1u) / 2u;
        }
    }
    // (one job only: the slot a workgroup id lands on is a property of the FIRST resident round of a launch -- the workgroups of a
    // launch's later jobs are dispatched as slots fall free, in no fixed relation to their ids; multi-pair launches also amortise the
    // tail the unequal shares remove: 22 us per pair in a 6-pair launch against 25 for one pair alone)
    if (mx && njobs == 1 && plan.atomic_merge && bias_a > 0 && bias_b > 0 && xcd_known && kMxResident * cu_x <= 96u) {
        // unequal shares by wave slot (K2nnJobDev.bias_a): one job whose grid is one round of three workgroups per CU -- every XCD holds
        // more than 64 and at most 96 of them -- with whole eights of query blocks (nothing padded) and counts known on the host
        K2nnJobDev& jb = jobs[0];
        const uint32_t per_xcd = (jb.qblocks >> 3) * jb.splits;
        const uint32_t nt_tiles = (jb.nt + 31u) >> 5;
        const uint32_t mean = jb.splits ? nt_tiles / jb.splits : 0u;
        // (with one or two query blocks per XCD the biased plan measured 0.3-0.8 us SLOWER -- 2048 x 60000, 4096 x 30000 --, from three on 1-2 us faster)
        if ((jb.qblocks & 7u) == 0u && jb.qblocks >= 24u && per_xcd > 2u * cu_x && per_xcd <= 3u * cu_x && !jb.cnt_q && !jb.cnt_t && jb.splits >= 6u && mean >= 8u) {
            // bias_a / bias_b arrive in 1/256 of the equal share (values below 64: tiles, for experiments)
            const uint32_t den = jb.splits * 256u;
            const uint32_t a = bias_a < 64 ? (uint32_t)bias_a : (nt_tiles * (uint32_t)bias_a + den / 2u) / den;
            const uint32_t b = bias_b < 64 ? (uint32_t)bias_b : (nt_tiles * (uint32_t)bias_b + den / 2u) / den;
            // every query block's split sizes as the kernel derives them (slot_shares_fit) ... and everything the 32-bit table entry
            // carries inside its field (a 12-bit begin field silently clamped train sets beyond 4096 tiles)
            const uint32_t nqx = jb.qblocks >> 3;
            bool ok = a >= 1u && b >= 1u && a <= 255u && b <= 255u && nqx <= kBiasQlMask + 1u && nt_tiles <= kBiasBeginMask;
            for (uint32_t ql = 0; ok && ql < nqx; ++ql) ok = slot_shares_fit(slot_shares(cu_x, ql, nqx, jb.splits, a, b, nt_tiles), nt_tiles);
            if (ok) { jb.bias_a = a; jb.bias_b = b; jb.bias_magic = 0u; jb.slot_wgs = cu_x; }
        }
        // the same for query-block counts that are NOT whole eights: interleaved over all workgroup ids (K2nnJobDev.bias_magic), the split
        // count taken anew (no per-XCD fit, nothing padded)
        const uint32_t QB = jb.qblocks;
        uint32_t sp = QB ? (uint32_t)target_blocks / QB : 0u;
        if (sp > nt_tiles / 8u) sp = nt_tiles / 8u;                            // >= 8 tiles per split on average
        if (jb.bias_a == 0u && (QB & 7u) != 0u && QB >= 24u && QB <= 128u && sp >= 6u && QB * sp > 2u * dev.n_cu && QB * sp <= slots && !jb.cnt_q && !jb.cnt_t &&
            (uint32_t)target_blocks == slots) {
            const uint32_t den = sp * 256u;
            const uint32_t a = bias_a < 64 ? (uint32_t)bias_a : (nt_tiles * (uint32_t)bias_a + den / 2u) / den;
            const uint32_t b = bias_b < 64 ? (uint32_t)bias_b : (nt_tiles * (uint32_t)bias_b + den / 2u) / den;
            bool ok = a >= 1u && b >= 1u && a <= 255u && b <= 255u;
            for (uint32_t q = 0; ok && q < QB; ++q) ok = slot_shares_fit(slot_shares(dev.n_cu, q, QB, sp, a, b, nt_tiles), nt_tiles);
            if (ok) {
                jb.bias_a = a; jb.bias_b = b;
                jb.bias_magic = (uint32_t)((0x100000000ull + QB - 1u) / QB);
                jb.slot_wgs = dev.n_cu;
                jb.splits = sp;
                jb.t_per_split = ((nt_tiles + sp - 1u) / sp) * 32u;             // (the equal share: reporting only)
            }
        }
    }
    plan.partial_elems = off;
    return plan;
}

hipError_t launch_k2nn(const K2nnJobDev* jobs, int njobs, uint2* d_partial, hipStream_t stream, Profiler* prof, int formulation,
                       uint64_t* d_stamps, bool probe)
{
    for (int base = 0, cnt = 0; base < njobs; base += cnt) {
        // the jobs of one launch share the acceptance rule (a template parameter of the sweep kernels)
        cnt = 1;
        while (cnt < kK2nnJobsPerLaunch && base + cnt < njobs && jobs[base + cnt].rule == jobs[base].rule) ++cnt;
        const bool ratio = jobs[base].rule == K2NN_RULE_RATIO;
        K2nnJobList list;
        uint32_t grid_x = 0, max_nq = 0, max_nq_empty = 0;
        for (int j = 0; j < cnt; ++j) {
            list.j[j] = jobs[base + j];
            // matrix kernel: query blocks are dealt to XCDs in eights (see the kernel) -> pad the count to a multiple of 8
            const uint32_t qb = formulation == K2NN_POPCOUNT ? list.j[j].qblocks : ((list.j[j].qblocks + 7u) & ~7u);
            const uint32_t gx = list.j[j].nt ? qb * list.j[j].splits : 0u;
            if (gx > grid_x) grid_x = gx;
            if (list.j[j].nq > max_nq) max_nq = list.j[j].nq;
            if (list.j[j].nt == 0u && list.j[j].nq > max_nq_empty) max_nq_empty = list.j[j].nq;
        }
        for (int j = cnt; j < kK2nnJobsPerLaunch; ++j) list.j[j] = K2nnJobDev{};
        for (uint32_t& e : list.bias_tab) e = 0u;
        if (cnt == 1 && list.j[0].bias_a != 0u && list.j[0].bias_magic != 0u && formulation != K2NN_POPCOUNT) {
            // interleaved over all ids: per query block q its split k is workgroup k QB + q, on wave slot (k QB + q) / 256 -- n0 splits on slot 0
            // (bits 0..7), n1 on slot 1 (8..15), tiles of a slot-2 split (16..23), how many of them take one more (24..31)
            const K2nnJobDev& jb = list.j[0];
            const uint32_t QB = jb.qblocks, nt_tiles = (jb.nt + 31u) >> 5;
            for (uint32_t q = 0; q < QB && q < 128u; ++q) {
                const SlotShares s = slot_shares(jb.slot_wgs, q, QB, jb.splits, jb.bias_a, jb.bias_b, nt_tiles);
                list.bias_tab[q] = s.n0 | (s.n1 << 8) | (std::min(s.c, 255u) << 16) | (std::min(s.extra, 255u) << 24);
            }
            grid_x = QB * jb.splits;                                          // nothing padded
        } else
        if (cnt == 1 && list.j[0].bias_a != 0u && formulation != K2NN_POPCOUNT) {
            // workgroup w of an XCD: query block w % nqx (the query blocks of an XCD interleaved, so that each has splits on all three wave
            // slots), its split k = w / nqx sits on slot w / 32: n0 splits of bias_a tiles, n1 of bias_b, the n2 slot-2 splits share the
            // rest (the first `extra` of them one tile more)
            const K2nnJobDev& jb = list.j[0];
            const uint32_t nqx = jb.qblocks >> 3, nt_tiles = (jb.nt + 31u) >> 5;
            for (uint32_t w = 0; w < nqx * jb.splits && w < 96u; ++w) {
                const uint32_t ql = w % nqx, k = w / nqx;
                const SlotShares s = slot_shares(jb.slot_wgs, ql, nqx, jb.splits, jb.bias_a, jb.bias_b, nt_tiles);
                const uint32_t k0 = std::min(k, s.n0), k1 = std::min(k - k0, s.n1), k2 = k - k0 - k1;
                const uint32_t begin = k0 * jb.bias_a + k1 * jb.bias_b + k2 * s.c + std::min(k2, s.extra);
                uint32_t size = k < s.n0 ? jb.bias_a : (k < s.n0 + s.n1 ? jb.bias_b : s.c + (k2 < s.extra ? 1u : 0u));
                if (k + 1u == jb.splits) size = nt_tiles > begin ? nt_tiles - begin : 0u;      // the last split takes what is left
                // (k2nn_plan has checked that every field holds its value; the clamps only keep a corrupted job record from aliasing)
                list.bias_tab[w] = (ql & kBiasQlMask) | (std::min(begin, kBiasBeginMask) << kBiasBeginShift) | (std::min(size, kBiasSizeMax) << kBiasSizeShift);
            }
        }
        if (max_nq == 0) continue;
        if (grid_x > 0) {
            prof_mark(prof, CLC_KERNEL_K2NN_SWEEP, true, stream);
            if (formulation == K2NN_POPCOUNT && ratio)
                hipLaunchKernelGGL((k2nn_sweep_kernel<kR, true>), dim3(grid_x, cnt), dim3(64 * kWaves), 0, stream, list, d_partial);
            else if (formulation == K2NN_POPCOUNT)
                hipLaunchKernelGGL(k2nn_sweep_kernel<kR>, dim3(grid_x, cnt), dim3(64 * kWaves), 0, stream, list, d_partial);
            else if (ratio && cnt == 1 && list.j[0].bias_a != 0u && list.j[0].bias_magic != 0u)     // (ratio jobs: no stamps, no probe)
                hipLaunchKernelGGL((k2nn_sweep_mx_kernel<false, true, false, true>), dim3(grid_x, cnt), dim3(64 * kMxWaves), 0, stream, list, d_partial,
                                   (uint64_t*)nullptr);
            else if (ratio)
                hipLaunchKernelGGL((k2nn_sweep_mx_kernel<false, false, false, true>), dim3(grid_x, cnt), dim3(64 * kMxWaves), 0, stream, list, d_partial,
                                   (uint64_t*)nullptr);
            else if (cnt == 1 && list.j[0].bias_a != 0u && list.j[0].bias_magic != 0u && d_stamps)
                hipLaunchKernelGGL((k2nn_sweep_mx_kernel<true, true>), dim3(grid_x, cnt), dim3(64 * kMxWaves), 0, stream, list, d_partial, d_stamps);
            else if (cnt == 1 && list.j[0].bias_a != 0u && list.j[0].bias_magic != 0u)
                hipLaunchKernelGGL((k2nn_sweep_mx_kernel<false, true>), dim3(grid_x, cnt), dim3(64 * kMxWaves), 0, stream, list, d_partial,
                                   (uint64_t*)nullptr);
            else if (d_stamps)
                hipLaunchKernelGGL((k2nn_sweep_mx_kernel<true>), dim3(grid_x, cnt), dim3(64 * kMxWaves), 0, stream, list, d_partial, d_stamps);
            else if (probe)
                hipLaunchKernelGGL((k2nn_sweep_mx_kernel<false, false, true>), dim3(grid_x, cnt), dim3(64 * kMxWaves), 0, stream, list, d_partial,
                                   (uint64_t*)nullptr);
            else
                hipLaunchKernelGGL((k2nn_sweep_mx_kernel<false>), dim3(grid_x, cnt), dim3(64 * kMxWaves), 0, stream, list, d_partial,
                                   (uint64_t*)nullptr);
            prof_mark(prof, CLC_KERNEL_K2NN_SWEEP, false, stream);
        }
        if (list.j[0].atomic_merge) {
            if (max_nq_empty)
                hipLaunchKernelGGL(k2nn_nomatch_kernel, dim3((max_nq_empty + 255) / 256, cnt), dim3(256), 0, stream, list);
        } else {
            prof_mark(prof, CLC_KERNEL_K2NN_MERGE, true, stream);
            hipLaunchKernelGGL(k2nn_merge_kernel, dim3((max_nq + kMergeQ - 1) / kMergeQ, cnt), dim3(kMergeQ * kMergeGroups),
                               0, stream, list, (const uint2*)d_partial);
            prof_mark(prof, CLC_KERNEL_K2NN_MERGE, false, stream);
        }
    }
    return hipGetLastError();
}

} // namespace clc

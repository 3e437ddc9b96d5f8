// k2nn_sweep.h -- what the popcount sweep (k2nn.hip: k2nn_sweep_kernel) and the guided sweep (k2nn_guided.hip) share: the workgroup's
// shape, the key layout and the finalize of a folded top-2 row.  Moved out of k2nn.hip as they stood; that file's comments explain them.
#ifndef CLC_K2NN_SWEEP_H
#define CLC_K2NN_SWEEP_H

#include "clc_internal.h"

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
typedef const u32x4 __attribute__((address_space(1)))* global_cu4_ptr;
typedef u32x2 __attribute__((address_space(1)))* global_u2_ptr;

// The acceptance rule (K2nnJobDev.rule) on the folded top-2: distances, or the CUDAK2NN.cu:54 sentinels 100000 / 200000 where fewer
// than two / one train rows were swept.  K2NN: CUDAK2NN.cu:75.  Ratio: the sentinel second is checked FIRST -- with one train row the
// 100000 would pass the ratio test -- then (float)d1 < r2 * (float)d2 (oracle/clc_oracle.c orc_k2nn_omp_ex, rule 1; no contraction:
// the build has -ffp-contract=off).  A compile-time parameter of the sweep kernels, not a runtime branch in them: the rule is uniform
// per launch (launch_k2nn), and any change to the finalize of k2nn_sweep_mx_kernel moves its register allocation: with a runtime branch
// here the compiler (ROCm 7, -O3) put 16 v_mov into the K2NN tile loop; with the template the K2NN instantiations keep their tile loop
// (check: hipcc -S --cuda-device-only on k2nn.hip, the tile block of k2nn_sweep_mx_kernel<false, false, false, false>).
template <bool RATIO>
__device__ __forceinline__ bool accept(const K2nnJobDev& job, const int best_i, const int best_v, const int second_v)
{
    if (best_i < 0) return false;
    if (RATIO) return second_v <= 512 && (float)best_v < job.r2 * (float)second_v;
    return second_v - best_v > (int)job.thr;
}

// {best_key, second_key} of one query -> the reference's outputs (CUDAK2NN.cu:54 sentinels, :75 acceptance)
template <bool RATIO>
__device__ __forceinline__ void emit_result(const K2nnJobDev& job, const uint32_t qi, const uint32_t bkey, const uint32_t skey)
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

} // namespace clc
#endif

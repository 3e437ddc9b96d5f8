// wg_compact.h -- the ordered compaction of one workgroup (device only), the ONE place that fixes the two rules the solves rest on:
//   * element i of the output is the i-th accepted element in ASCENDING input order (the sampler draws by position, the scale rule
//     walks consecutive features): ordered_slot below, pass after pass of kThreads elements, the caller carrying the running base;
//   * the count comes out LAST, behind a system-scope fence: after its passes a kernel runs __threadfence_system(), __syncthreads(),
//     and only then one thread stores the count / the record's ready word (release, system scope) -- the host reads pinned memory
//     on the strength of that word.  That epilogue stays in each kernel (gather.hip, inter_dev.hip): what it publishes differs.
#ifndef CLC_WG_COMPACT_H
#define CLC_WG_COMPACT_H

#include <hip/hip_runtime.h>

namespace clc {

// Position of this thread's accepted element among the accepted elements of the pass, and their number (*total, the same in every
// thread): accepted lanes below this one in the wave (ballot + mbcnt), accepted elements of the waves before it (a kThreads / 64-entry
// LDS scan, s_wave).  EVERY thread of the kThreads-wide workgroup calls it, the same number of times.
template <int kThreads> __device__ __forceinline__ uint32_t ordered_slot(const bool ok, uint32_t* s_wave, uint32_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t b = __ballot(ok);
    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (uint32_t w = 0; w < kThreads / 64; ++w) {
        const uint32_t c = s_wave[w];
        off += w < wave ? c : 0u;
        tot += c;
    }
    __syncthreads();                                     // (s_wave is written again by the next call)
    *total = tot;
    return off + before;
}

} // namespace clc

#endif

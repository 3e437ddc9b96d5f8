// k2nn_top2.h -- the running top-2 of the matrix sweep (k2nn_sweep_mx_kernel, k2nn.hip) as a network of three-input instructions, host +
// device inline and written ONCE, as map_math.h is: the kernel and the host build the tests hold it to (tests/host/k2nn_top2_lib.cpp) run
// the very same statements.
//
// Keys are the BITS of positive finite floats or of +inf ("none yet", penalised padding rows): their float order is the unsigned order of
// the bits, so the network is plain unsigned min / max nests, which the gfx950 back end selects as v_min3_u32 / v_med3_u32 / v_min_u32
// (no canonicalising v_max_f32 x, x in front of an operand, as fminf / fmaxf can drag in).  Within one chain the keys are distinct except
// for repeated +inf; the network returns the two smallest VALUES of the multiset under any ties.
//
// Count.  One key at a time costs two instructions per key (second = med3(best, second, k); best = min(best, k)): 32 for the sixteen
// accumulator registers of a chain.  Three keys reduce to their two smallest in two (min3, med3: the largest of three is never in a
// top-2), and the running pair (b, s) merges with two such pairs (l1, m1), (l2, m2) in four:
//     b' = min3(b, l1, l2)        s' = min(med3(b, l1, l2), min3(s, m1, m2))
// (the second smallest overall is the second of the three minima or the smallest of the three partners).  Sixteen keys: five triples (10),
// two merges (8), and the merge of the running pair with the fifth triple and the sixteenth key, whose partner is "none" (3):
//     b' = min3(b, l, k)          s' = min3(med3(b, l, k), s, m)
// 21 instead of 32, and the dependent chain through (b, s) is 6 instructions long instead of 32.
#ifndef CLC_K2NN_TOP2_H
#define CLC_K2NN_TOP2_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define TOP2_HD __host__ __device__ __forceinline__
#else
#define TOP2_HD static inline
#endif

namespace clc {

TOP2_HD uint32_t top2_min(const uint32_t a, const uint32_t b) { return a < b ? a : b; }
TOP2_HD uint32_t top2_max(const uint32_t a, const uint32_t b) { return a < b ? b : a; }
// (min3 pairs b with c, med3 a with b: sharing min(a, b) between the two of a triple leaves that min with two uses, and the back end then
// selects two v_min_u32 instead of one v_min3_u32)
TOP2_HD uint32_t top2_min3(const uint32_t a, const uint32_t b, const uint32_t c) { return top2_min(a, top2_min(b, c)); }
TOP2_HD uint32_t top2_med3(const uint32_t a, const uint32_t b, const uint32_t c) { return top2_max(top2_min(a, b), top2_min(top2_max(a, b), c)); }

// three keys -> their two smallest
TOP2_HD void top2_triple(const uint32_t a, const uint32_t b, const uint32_t c, uint32_t& lo, uint32_t& mid)
{
    lo = top2_min3(a, b, c);
    mid = top2_med3(a, b, c);
}

// the running pair (b <= s) with two sorted pairs (l1 <= m1), (l2 <= m2), in the two halves the sweep issues it in: the head reads the
// three minima, the tail the three partners
TOP2_HD void top2_merge3_head(const uint32_t b, const uint32_t l1, const uint32_t l2, uint32_t& nb, uint32_t& t)
{
    nb = top2_min3(b, l1, l2);
    t = top2_med3(b, l1, l2);
}
TOP2_HD void top2_merge3_tail(uint32_t& b, uint32_t& s, const uint32_t nb, const uint32_t t, const uint32_t m1, const uint32_t m2)
{
    b = nb;
    s = top2_min(t, top2_min3(s, m1, m2));
}
TOP2_HD void top2_merge3(uint32_t& b, uint32_t& s, const uint32_t l1, const uint32_t m1, const uint32_t l2, const uint32_t m2)
{
    uint32_t nb, t;
    top2_merge3_head(b, l1, l2, nb, t);
    top2_merge3_tail(b, s, nb, t, m1, m2);
}

// the running pair with one sorted pair (l <= m) and a single key k (its partner is "none"): head as above with k for l2
TOP2_HD void top2_merge_pair_key_tail(uint32_t& b, uint32_t& s, const uint32_t nb, const uint32_t t, const uint32_t m)
{
    b = nb;
    s = top2_min3(t, s, m);
}

// the step back of the running pair by one tile of 32 rows: float arithmetic on the VALUE (with distance 0 a stepped-back value lies
// below 2^23, where the bits are no longer magic + integer); +inf stays +inf
TOP2_HD uint32_t top2_step_back(const uint32_t bits)
{
    float v;
    __builtin_memcpy(&v, &bits, 4);
    v -= 32.0f;
    uint32_t r;
    __builtin_memcpy(&r, &v, 4);
    return r;
}

// The fold of sixteen keys into (b, s), cut into the eight steps the sweep issues it in (one per MFMA of the other chain; three
// instructions or fewer each).  The triples of keys 3 m .. 3 m + 2 depend on the keys alone; at most two of them, and one merge's head, wait
// in `w`.
struct Top2Wait { uint32_t l0, m0, l1, m1, nb, t; };

// (step: a constant wherever it is called, so one branch is left)
TOP2_HD void top2_fold16_step(const int step, uint32_t& b, uint32_t& s, Top2Wait& w, const uint32_t (&k)[16])
{
    if (step == 0) { top2_triple(k[0], k[1], k[2], w.l0, w.m0); w.l1 = top2_min3(k[3], k[4], k[5]); }                          // 3
    if (step == 1) { w.m1 = top2_med3(k[3], k[4], k[5]); top2_merge3_head(b, w.l0, w.l1, w.nb, w.t); }                         // 3
    if (step == 2) { top2_merge3_tail(b, s, w.nb, w.t, w.m0, w.m1); w.l0 = top2_min3(k[6], k[7], k[8]); }                      // 3
    if (step == 3) { w.m0 = top2_med3(k[6], k[7], k[8]); top2_triple(k[9], k[10], k[11], w.l1, w.m1); }                        // 3
    if (step == 4) { top2_merge3_head(b, w.l0, w.l1, w.nb, w.t); w.m0 = top2_min3(s, w.m0, w.m1); }                            // 3 (the tail's min3 here,
    if (step == 5) { b = w.nb; s = top2_min(w.t, w.m0); top2_triple(k[12], k[13], k[14], w.l0, w.m0); }                        // 3  its min there)
    if (step == 6) { top2_merge3_head(b, w.l0, k[15], w.nb, w.t); }                                                            // 2
    if (step == 7) { top2_merge_pair_key_tail(b, s, w.nb, w.t, w.m0); }                                                        // 1 (+ the step back)
}

// sixteen keys into the running pair
TOP2_HD void top2_fold16(uint32_t& best, uint32_t& second, const uint32_t (&k)[16])
{
    Top2Wait w = { 0u, 0u, 0u, 0u, 0u, 0u };
    top2_fold16_step(0, best, second, w, k);
    top2_fold16_step(1, best, second, w, k);
    top2_fold16_step(2, best, second, w, k);
    top2_fold16_step(3, best, second, w, k);
    top2_fold16_step(4, best, second, w, k);
    top2_fold16_step(5, best, second, w, k);
    top2_fold16_step(6, best, second, w, k);
    top2_fold16_step(7, best, second, w, k);
}

}  // namespace clc

#endif

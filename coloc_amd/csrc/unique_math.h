// unique_math.h -- the three statements of the one-to-one filter (include/coloc_hip.h, clc_match_unique_dev), host + device inline and
// written ONCE, as bin_math.h is: the kernels of k2nn_unique.hip and the host build the tests hold them to (tests/host/unique_lib.cpp)
// run the very same lines.
//
//   unique_is_claim   entry q of a match list is a CLAIM on train row t = match[q] iff 0 <= t < nt and best[q] <= 512
//   unique_key        (best << 22) | q: the (distance << 22) + row key of the sweeps' top-2 (k2nn_sweep.h), with the QUERY row as the index
//   unique_holder_of  the query row of a claim word, or -1 for the armed word
//
// A key is at most (512 << 22) | (2^22 - 1) = 2^31 + 2^22 - 1, so the armed word 0xFFFFFFFF is no key and the smallest key of a row --
// the smallest distance, the lowest query row among equals -- is an unsigned 32-bit minimum.  Integers only: nothing here depends on a
// floating-point flag.
#ifndef CLC_UNIQUE_MATH_H
#define CLC_UNIQUE_MATH_H

#include "guided_math.h"

namespace clc {

static constexpr uint32_t kUniqueShift = 22;                          // bits of the query row in a key
static constexpr uint32_t kUniqueRowMask = (1u << kUniqueShift) - 1u;
static constexpr uint32_t kUniqueMaxRows = 1u << kUniqueShift;        // query rows a call takes
static constexpr uint32_t kUniqueMaxDist = 512u;                      // the largest distance of two 512-bit rows
static constexpr uint32_t kUniqueFree = 0xFFFFFFFFu;                  // the armed claim word: nobody claims the row

GUIDED_HD bool unique_is_claim(const int32_t t, const uint32_t best, const int32_t nt) { return t >= 0 && t < nt && best <= kUniqueMaxDist; }
GUIDED_HD uint32_t unique_key(const uint32_t best, const uint32_t q) { return (best << kUniqueShift) | q; }
GUIDED_HD int32_t unique_holder_of(const uint32_t word) { return word == kUniqueFree ? -1 : (int32_t)(word & kUniqueRowMask); }

} // namespace clc

#endif

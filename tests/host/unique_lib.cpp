// Host build of the one-to-one filter's statements (coloc_amd/csrc/unique_math.h) as a tiny shared library for the tests
// (tests/unique_host.py): the key, the holder of a claim word, the claim test, and the filter over them in the kernels' three steps,
// compiled by plain g++ -- the lines the kernels of coloc_amd/csrc/k2nn_unique.hip run.  Test infrastructure only.
#include <stddef.h>
#include <cstdint>
#include <vector>
#include "../../coloc_amd/csrc/unique_math.h"

using namespace clc;

extern "C" {

void unique_host_keys(const uint32_t* best, const uint32_t* q, int n, uint32_t* key, int32_t* holder)
{
    for (int i = 0; i < n; ++i) { key[i] = unique_key(best[i], q[i]); holder[i] = unique_holder_of(key[i]); }
}

void unique_host_claims(const int32_t* match, const uint16_t* best, int nq, int nt, uint8_t* out)
{
    for (int q = 0; q < nq; ++q) out[q] = unique_is_claim(match[q], best[q], nt) ? 1 : 0;
}

void unique_host_filter(int32_t* match, const uint16_t* best, int nq, int nt, int32_t* owner)
{
    std::vector<uint32_t> claim((size_t)nt, kUniqueFree);                                    // arm
    for (int q = 0; q < nq; ++q)                                                             // claim
        if (unique_is_claim(match[q], best[q], nt)) {
            const uint32_t k = unique_key(best[q], (uint32_t)q);
            if (k < claim[(size_t)match[q]]) claim[(size_t)match[q]] = k;
        }
    for (int q = 0; q < nq; ++q)                                                             // resolve
        if (match[q] != -1 && !(unique_is_claim(match[q], best[q], nt) && unique_holder_of(claim[(size_t)match[q]]) == q)) match[q] = -1;
    for (int t = 0; t < nt; ++t) owner[t] = unique_holder_of(claim[(size_t)t]);
}

uint32_t unique_host_free_word() { return kUniqueFree; }
int unique_host_shift() { return (int)kUniqueShift; }
uint32_t unique_host_max_rows() { return kUniqueMaxRows; }

} // extern "C"

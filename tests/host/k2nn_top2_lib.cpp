// Host build of coloc_amd/csrc/k2nn_top2.h as a tiny shared library for the tests (tests/test_k2nn_top2_host.py): the top-2 network
// k2nn_sweep_mx_kernel runs on its accumulator registers, on the same key bits.  No GPU, no HIP headers.  Test infrastructure only.
#include <stdint.h>

#include "../../coloc_amd/csrc/k2nn_top2.h"

extern "C" {

// n cases: keys n x 16, pair n x 2 (best, second) in and out
void k2nn_top2_host_fold16(const uint32_t* keys, uint32_t* pair, int n)
{
    for (int i = 0; i < n; ++i) {
        uint32_t k[16];
        for (int j = 0; j < 16; ++j) k[j] = keys[16 * i + j];
        clc::top2_fold16(pair[2 * i], pair[2 * i + 1], k);
    }
}

// the sweep's chained use, n cases of `chains` consecutive folds: keys n x chains x 16; the pair (n x 2, in and out) steps back by one
// tile behind every fold, as in the kernel
void k2nn_top2_host_chain(const uint32_t* keys, uint32_t* pair, int n, int chains)
{
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < chains; ++c) {
            uint32_t k[16];
            for (int j = 0; j < 16; ++j) k[j] = keys[(i * chains + c) * 16 + j];
            clc::top2_fold16(pair[2 * i], pair[2 * i + 1], k);
            pair[2 * i] = clc::top2_step_back(pair[2 * i]);
            pair[2 * i + 1] = clc::top2_step_back(pair[2 * i + 1]);
        }
}

// the parts: three keys -> (lo, mid); three sorted pairs -> one
void k2nn_top2_host_triple(const uint32_t* k, uint32_t* out) { clc::top2_triple(k[0], k[1], k[2], out[0], out[1]); }
void k2nn_top2_host_merge3(const uint32_t* p, uint32_t* out)
{
    out[0] = p[0]; out[1] = p[1];
    clc::top2_merge3(out[0], out[1], p[2], p[3], p[4], p[5]);
}
uint32_t k2nn_top2_host_step_back(uint32_t bits) { return clc::top2_step_back(bits); }

}

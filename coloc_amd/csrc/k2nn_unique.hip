// k2nn_unique.hip -- the one-to-one filter (include/coloc_hip.h: clc_match_unique_dev, clc_match_unique_batch_dev) and the binned map
// match composed with it (clc_match_map_binned_unique_dev): every train row keeps the claimant with the smallest key
// (distance << 22) | query row (unique_math.h).  The pair and map sweeps composed with it are capi_match.hip's.
//
// Three enqueued operations per call, whatever the number of jobs, all on the caller's stream:
//   unique_arm_kernel      the claim words of all jobs -- ONE range of the context's d_unique -- set to 0xFFFFFFFF, on every call.  A
//                          launch like the other two, not a memset: in a captured graph a memset node left other bytes than 0xFF
//                          in the words on its second replay (tests/test_gpu_match_unique.py's replay test, one observation)
//   unique_claim_kernel    one thread per query (blockIdx.y = job): a claim folds its key into the word of its row by a 32-bit unsigned
//                          atomicMin, the ordinary vector-memory atomic at device scope; nothing else is written
//   unique_resolve_kernel  thread i answers query i (d_match[i] stays iff the word of its row names i) and train row i (d_owner[i]); the
//                          claim words are only read here, so a thread's answer does not depend on what any other thread does
// An entry's row is checked against nt before it is used as an index, in both kernels, by the one statement unique_is_claim.
#include "clc_ctx.h"
#include "k2nn_proj.h"
#include "k2nn_sweep.h"
#include "unique_math.h"

#include <algorithm>
#include <vector>

namespace clc {

static_assert(kUniqueShift == kKeyShift && kUniqueFree == kEmpty, "the filter's key is the sweeps' (distance << 22) + row key");

namespace {

constexpr int kUniqueMaxJobs = CLC_MAX_TRACK_PAIRS;
constexpr uint32_t kUniqueThreads = 256;

struct UniqueJobDev {
    int32_t* match; const uint16_t* best; int32_t* owner;             // the caller's (owner nullable)
    uint32_t* claim;                                                  // nt words of d_unique
    uint32_t nq; int32_t nt;
};
struct UniqueJobList { UniqueJobDev j[kUniqueMaxJobs]; };
static_assert(sizeof(UniqueJobList) <= 4096, "UniqueJobList is passed as a kernel argument: it must stay within the 4 KB kernarg segment");

__global__ __launch_bounds__(kUniqueThreads) void unique_arm_kernel(uint32_t* __restrict__ words, const size_t n)
{
    const size_t i = (size_t)blockIdx.x * kUniqueThreads + threadIdx.x;
    if (i < n) words[i] = kUniqueFree;
}

__global__ __launch_bounds__(kUniqueThreads) void unique_claim_kernel(const UniqueJobList jobs)
{
    const UniqueJobDev& jb = jobs.j[blockIdx.y];
    const uint32_t q = blockIdx.x * kUniqueThreads + threadIdx.x;
    if (q >= jb.nq) return;
    const int32_t t = jb.match[q];
    const uint32_t best = jb.best[q];
    if (unique_is_claim(t, best, jb.nt)) atomicMin(jb.claim + t, unique_key(best, q));       // 0 <= t < nt
}

__global__ __launch_bounds__(kUniqueThreads) void unique_resolve_kernel(const UniqueJobList jobs)
{
    const UniqueJobDev& jb = jobs.j[blockIdx.y];
    const uint32_t i = blockIdx.x * kUniqueThreads + threadIdx.x;
    if (i < jb.nq) {
        const int32_t t = jb.match[i];
        if (t != -1) {
            const bool kept = unique_is_claim(t, jb.best[i], jb.nt) && unique_holder_of(jb.claim[t]) == (int32_t)i;
            if (!kept) jb.match[i] = -1;
        }
    }
    if (jb.owner && i < (uint32_t)jb.nt) jb.owner[i] = unique_holder_of(jb.claim[i]);
}

} // namespace

int unique_check(clc_ctx* ctx, const char* who, const clc_unique_job* jobs, const int n_jobs, const bool need_best)
{
    const auto bad = [&](const char* what) { return fail(ctx, CLC_ERR_BAD_ARG, (std::string(who) + what).c_str()); };
    if (!ctx || n_jobs < 0 || n_jobs > kUniqueMaxJobs || (n_jobs > 0 && !jobs)) return bad(": null context / jobs, or a job count outside 0 .. CLC_MAX_TRACK_PAIRS");
    if (!ctx->has_mat) return fail(ctx, CLC_ERR_STATE, (std::string(who) + ": context created without matcher options").c_str());
    for (int j = 0; j < n_jobs; ++j) {
        const clc_unique_job& jb = jobs[j];
        if (jb.nq < 0 || jb.nt < 0 || (jb.nq > 0 && (!jb.d_match || (need_best && !jb.d_best)))) return bad(": negative count / null list");
        if (((uintptr_t)jb.d_match & 3u) || ((uintptr_t)jb.d_best & 1u) || ((uintptr_t)jb.d_owner & 3u)) return bad(": misaligned device pointer");
    }
    for (int j = 0; j < n_jobs; ++j)
        if ((uint32_t)jobs[j].nq > kUniqueMaxRows) return fail(ctx, CLC_ERR_CAPACITY, (std::string(who) + ": more than 2^22 query rows").c_str());
    return CLC_OK;
}

int unique_scratch(clc_ctx* ctx, const int nq, const int nt, const bool with_best, const bool with_owner, UniqueDev& dv)
{
    return carve_block(ctx, ctx->d_unique, 1, 4, true, "growing d_unique", [&](Carve& c) { dv.carve(c, (size_t)nq, (size_t)nt, with_best, with_owner); });
}

int unique_enqueue(clc_ctx* ctx, const clc_unique_job* jobs, const UniqueDev* dv, const int n_jobs, hipStream_t st)
{
    UniqueJobList list{};
    uint32_t max_nq = 0, max_rows = 0;
    uintptr_t arm_lo = 0, arm_hi = 0;                                     // the claim words of every job: one range (UniqueDev)
    int n = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const clc_unique_job& jb = jobs[j];
        if (jb.nq == 0 && (jb.nt == 0 || !jb.d_owner)) continue;          // nothing to answer
        UniqueJobDev& d = list.j[n++];
        d.match = jb.d_match; d.best = jb.d_best; d.owner = jb.d_owner; d.claim = dv[j].claim;
        d.nq = (uint32_t)jb.nq; d.nt = jb.nt;
        max_nq = std::max(max_nq, d.nq);
        max_rows = std::max(max_rows, std::max(d.nq, jb.d_owner ? (uint32_t)jb.nt : 0u));
        if (jb.nt > 0) {
            const uintptr_t lo = (uintptr_t)d.claim, hi = lo + (size_t)jb.nt * sizeof(uint32_t);
            arm_lo = arm_hi ? std::min(arm_lo, lo) : lo;
            arm_hi = std::max(arm_hi, hi);
        }
    }
    if (n == 0) return CLC_OK;
    hipError_t e = hipSuccess;
    if (arm_hi > arm_lo) {
        const size_t words = (arm_hi - arm_lo) / sizeof(uint32_t);
        hipLaunchKernelGGL(unique_arm_kernel, dim3((unsigned)((words + kUniqueThreads - 1u) / kUniqueThreads)), dim3(kUniqueThreads), 0, st, (uint32_t*)arm_lo, words);
        e = hipGetLastError();
    }
    if (e == hipSuccess && max_nq > 0) {
        hipLaunchKernelGGL(unique_claim_kernel, dim3((max_nq + kUniqueThreads - 1u) / kUniqueThreads, (unsigned)n), dim3(kUniqueThreads), 0, st, list);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(unique_resolve_kernel, dim3((max_rows + kUniqueThreads - 1u) / kUniqueThreads, (unsigned)n), dim3(kUniqueThreads), 0, st, list);
        e = hipGetLastError();
    }
    return e == hipSuccess ? CLC_OK : fail(ctx, CLC_ERR_HIP, "match_unique: launch", e);
}

namespace {

int unique_batch(clc_ctx* ctx, const clc_unique_job* jobs, const int n_jobs, void* stream)
{
    const int checked = unique_check(ctx, "match_unique", jobs, n_jobs, true);      // everything is checked before anything is enqueued
    if (checked != CLC_OK) return checked;
    if (n_jobs == 0) return CLC_OK;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<UniqueDev> dv((size_t)n_jobs);
    const int rc = carve_block(ctx, ctx->d_unique, 1, 4, true, "growing d_unique", [&](Carve& c) {
        for (int j = 0; j < n_jobs; ++j) dv[(size_t)j].carve(c, (size_t)jobs[j].nq, (size_t)jobs[j].nt, false, false);
    });
    return rc == CLC_OK ? unique_enqueue(ctx, jobs, dv.data(), n_jobs, pick(ctx, stream)) : rc;
}

} // namespace

} // namespace clc

using namespace clc;

extern "C" {

int clc_match_unique_dev(clc_ctx* ctx, const clc_unique_job* job, void* stream)
{
    if (!job) return fail(ctx, CLC_ERR_BAD_ARG, "match_unique: null job");
    return unique_batch(ctx, job, 1, stream);
}

int clc_match_unique_batch_dev(clc_ctx* ctx, const clc_unique_job* jobs, int n_jobs, void* stream)
{
    return unique_batch(ctx, jobs, n_jobs, stream);
}

int clc_match_map_binned_unique_dev(clc_ctx* ctx, const clc_map_guided_job* job, int32_t* d_owner, void* stream)
{
    if (!job) return fail(ctx, CLC_ERR_BAD_ARG, "match_map_binned_unique: null job");
    std::vector<GatherSide> sides;
    int rc = proj_checks(ctx, job, 1, sides);                          // the producer's rules, before anything is allocated
    if (rc != CLC_OK) return rc;
    clc_unique_job uj{};
    uj.d_match = job->d_match; uj.d_best = job->d_best; uj.nq = job->nq; uj.nt = ctx->map_n; uj.d_owner = d_owner;
    rc = unique_check(ctx, "match_map_binned_unique", &uj, 1, false);
    if (rc != CLC_OK) return rc;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    UniqueDev dv;
    rc = unique_scratch(ctx, uj.nq, uj.nt, !job->d_best, false, dv);
    if (rc != CLC_OK) return rc;
    clc_map_guided_job jb = *job;
    if (!jb.d_best) jb.d_best = dv.best;                                // the distances the filter reads: the caller's, or the context's scratch
    uj.d_best = jb.d_best;
    rc = clc_match_map_binned_dev(ctx, &jb, stream);
    return rc == CLC_OK ? unique_enqueue(ctx, &uj, &dv, 1, pick(ctx, stream)) : rc;
}

} // extern "C"

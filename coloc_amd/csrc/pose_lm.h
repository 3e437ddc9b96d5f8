// pose_lm.h -- the Levenberg-Marquardt pass over one pose, stated once for pnp_refine_kernel (pnp.hip) and pose_prior_kernel
// (pose_prior.hip).  Role: Localizer::refine -> PoseRefiner::refinePose (reference include/coloc/Localizer.hpp:110-177,
// include/coloc/Refiner.hpp:47-239): minimise 1/2 sum_i rho(||r_i||^2) over the 6 pose parameters [angle-axis w | t]
// (x_cam = R(w) X + t), structure and intrinsics fixed, r_i = observed - projected pixel, rho = ceres::HuberLoss(Square(4.0))
// (Refiner.hpp:122): rho(s) = s for s <= 256, 2*16*sqrt(s) - 256 beyond; then the 6x6 covariance block of the pose = (J^T W J)^-1 at
// the solution (:177-197).  Ceres itself is absent (OpenMVG third_party, empty submodule) -> unpinned; this is a Levenberg-Marquardt on
// the same cost with the same parametrisation, one workgroup of 512 threads per pose, every iteration = one pass over the points
// (residual + 2 x 6 Jacobian + 29 sums per thread, reduced in a fixed order through LDS) + a 6x6 Cholesky solve by lane 0.
// rodrigues / log_so3 / d_rodrigues_entry / solve6 / invert6_column: so3.h (host + device, so that the tests run them on the CPU too).
//
// A kernel's trip, in the order of the pieces here:
//   pose_start                                      Rt -> s.par, once
//   pose_rotation, then per point pose_residual -> [the kernel decides whether the point is used] -> pose_accumulate, pose_reduce
//                                                   ONE pass at s.par or s.try_: cost AND the normal-equation sums, so that an accepted
//                                                   trial needs no second pass (rejections are rare and only waste the Jacobian part)
//   pose_keep_sums | lm_judge                       the sums of a pass at s.par are the current ones | a trial against them
//   lm_next_step                                    lane 0's solve: the next trial in s.try_, or the end
//   pose_cov_column, pose_Rt, pose_rmse, pose_publish   the record
// The loop around the pass stays in each kernel, with ONE call site of the pass: everything here is force-inlined, and a second copy of
// the per-point body costs a dozen spilled VGPRs at the 256-register budget of a 512-thread workgroup.
// The 29th sum is the kernel's own (pnp_refine_kernel: the points used; pose_prior_kernel: three counts packed into one double).
//
// What counts as an ITERATION (RefineOut.iterations, PriorOut.iterations; LmState.it, compared with max_iter before every solve):
// every trial that was evaluated and judged, and every factorization that failed -- except the rejection or the failure that takes
// lambda above 1e10, which ends the minimisation uncounted.
//
// Fused multiply-adds in every function below that multiplies (the file default is off for the kernels compared bit for bit with the
// oracle; the refinement is held to a 50-digit reference by tolerance: tests/pose_mp.py, tests/pose_prior_mp.py); so3.h's own
// functions stay uncontracted.
#ifndef CLC_POSE_LM_H
#define CLC_POSE_LM_H

#include "clc_internal.h"
#include "so3.h"

namespace clc {

static constexpr int kPoseSums = 29;      // 21 (upper JtWJ) + 6 (JtWr) + 1 (cost) + 1 (the kernel's own)
static constexpr int kPoseThreads = 512;
static constexpr size_t kPoseRedBytes = sizeof(double) * kPoseSums * kPoseThreads;      // red[sum][thread], dynamic LDS: 116 KB
static_assert(kPoseThreads == 16 * 32 && kPoseSums * 16 <= kPoseThreads, "pose_reduce: 16 threads per sum add 32 partials each");

// The static LDS of a pose workgroup (4592 bytes).  alignas(16): where the compiler placed these arrays when each was a variable of
// its own, so the reads of s.R and s.dR keep their width.
struct PoseLds {
    alignas(16) double par[6];            // the current parameters [w | t]
    alignas(16) double try_[6];           // the trial
    alignas(16) double R[9];              // R(w) of the pass being made
    alignas(16) double dR[3][9];          // dR/dw_k of the pass being made
    alignas(16) double part[kPoseSums][16];
    alignas(16) double tot[kPoseSums];    // the sums of the pass just made
    alignas(16) double A[kPoseSums];      // the sums (JtWJ, JtWr, cost, the kernel's own) at the CURRENT parameters par
    int flag;
};
static_assert(sizeof(PoseLds) == 4592, "the pose kernels' static LDS");

struct PoseCam { double fx, sk, cx, fy, cy, huber_a, b2; };      // b2 = huber_a^2

// Levenberg-Marquardt's registers (every thread holds the same values)
struct LmState { double lambda = 1e-4, cost = 0.0; int it = 0; };

// one point at the parameters of the pass
struct PosePoint { double X0, X1, X2, xc, yc, zc, iz, xn, yn, r0, r1, sq; };

// Rt (3 x 4, row-major) -> s.par
__device__ __forceinline__ void pose_start(PoseLds& s, const int tid, const double* Rt)
{
    if (tid == 0) {
        double R0[9] = { Rt[0], Rt[1], Rt[2], Rt[4], Rt[5], Rt[6], Rt[8], Rt[9], Rt[10] };
        double w[3];
        log_so3(R0, w);
        s.par[0] = w[0]; s.par[1] = w[1]; s.par[2] = w[2]; s.par[3] = Rt[3]; s.par[4] = Rt[7]; s.par[5] = Rt[11];
    }
    __syncthreads();
}

// The prologue of a pass.  Every lane of the first wave evaluates R (same operands, same result); lane 0..8 publish it and lanes
// 0..26 each one entry of the three derivative matrices -- the serial prologue of a pass is one rotation + one entry instead of one
// rotation + 27 entries.
__device__ __forceinline__ void pose_rotation(PoseLds& s, const int tid, const double* par)
{
    if (tid < 64) {
        double Rl[9];
        rodrigues(par, Rl);
        if (tid < 9) s.R[tid] = Rl[tid];
        if (tid < 27) s.dR[tid / 9][tid % 9] = d_rodrigues_entry(par, Rl, tid / 9, tid % 9);
    }
    __syncthreads();
}

__device__ __forceinline__ PosePoint pose_residual(const PoseLds& s, const double* par, const PoseCam& c, const double* __restrict__ X,
                                                   const double* __restrict__ x, const int i)
{
#pragma clang fp contract(fast)
    PosePoint p;
    p.X0 = X[3 * i]; p.X1 = X[3 * i + 1]; p.X2 = X[3 * i + 2];
    p.xc = s.R[0] * p.X0 + s.R[1] * p.X1 + s.R[2] * p.X2 + par[3];
    p.yc = s.R[3] * p.X0 + s.R[4] * p.X1 + s.R[5] * p.X2 + par[4];
    p.zc = s.R[6] * p.X0 + s.R[7] * p.X1 + s.R[8] * p.X2 + par[5];
    p.iz = 1.0 / p.zc; p.xn = p.xc * p.iz; p.yn = p.yc * p.iz;
    p.r0 = x[2 * i] - (c.fx * p.xn + c.sk * p.yn + c.cx); p.r1 = x[2 * i + 1] - (c.fy * p.yn + c.cy);
    p.sq = p.r0 * p.r0 + p.r1 * p.r1;
    return p;
}

// a USED point into sums 0 .. 27
__device__ __forceinline__ void pose_accumulate(const PoseLds& s, const PoseCam& c, const PosePoint& p, double* acc)
{
#pragma clang fp contract(fast)
    double rho = p.sq, wgt = 1.0;                                    // rho(s), rho'(s)
    if (p.sq > c.b2) {                                               // Huber tail: rare after RANSAC, and a real branch
        const double r = sqrt(p.sq);                                 // (skipped when no lane of the wave needs it)
        rho = 2.0 * c.huber_a * r - c.b2;
        wgt = c.huber_a / r;
    }
    acc[27] += 0.5 * rho;
    // d(proj)/d(xc,yc,zc)
    const double pu0 = c.fx * p.iz, pu1 = c.sk * p.iz, pu2 = -(c.fx * p.xn + c.sk * p.yn) * p.iz;
    const double pv1 = c.fy * p.iz, pv2 = -c.fy * p.yn * p.iz;
    double Ju[6], Jv[6];      // Jacobian of the PROJECTION (residual = obs - proj -> J_r = -J)
    // the 27 derivative entries are read from LDS per point (uniform address: a broadcast read); hoisted out of the loop they take
    // 54 VGPRs and push the kernel over its 256-register budget into scratch -- the opaque offset stops that
    int dro = 0;
    asm volatile("" : "+v"(dro));
    const double (*dRp)[9] = reinterpret_cast<const double (*)[9]>(&s.dR[0][0] + dro);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double d0 = dRp[k][0] * p.X0 + dRp[k][1] * p.X1 + dRp[k][2] * p.X2;
        const double d1 = dRp[k][3] * p.X0 + dRp[k][4] * p.X1 + dRp[k][5] * p.X2;
        const double d2 = dRp[k][6] * p.X0 + dRp[k][7] * p.X1 + dRp[k][8] * p.X2;
        Ju[k] = pu0 * d0 + pu1 * d1 + pu2 * d2;
        Jv[k] = pv1 * d1 + pv2 * d2;
    }
    Ju[3] = pu0; Ju[4] = pu1; Ju[5] = pu2;
    Jv[3] = 0.0; Jv[4] = pv1; Jv[5] = pv2;
    int idx = 0;
#pragma unroll
    for (int a_ = 0; a_ < 6; ++a_) {
#pragma unroll
        for (int b_ = a_; b_ < 6; ++b_) acc[idx++] += wgt * (Ju[a_] * Ju[b_] + Jv[a_] * Jv[b_]);
    }
#pragma unroll
    for (int a_ = 0; a_ < 6; ++a_) acc[21 + a_] += wgt * (Ju[a_] * p.r0 + Jv[a_] * p.r1);   // = -J_r^T W r : descent rhs
}

// Reduction of the 29 sums over the 512 threads THROUGH LDS, transposed: every thread parks its partials in red[sum][thread]
// (conflict-free 8-byte writes), then 29 x 16 threads each add 32 of them and 29 threads add the 16 partial results -> s.tot.  The
// shuffle tree it replaces (29 values x 6 levels x 2 ds_bpermute per wave, eight waves on one LDS pipe) took 16-18 k cycles per pass,
// measured; this takes ~3 k.  A fixed order, no floating-point atomics: two runs on the same inputs give the same bits.
__device__ __forceinline__ void pose_reduce(PoseLds& s, double* red, const int tid, const double* acc)
{
#pragma unroll
    for (int i = 0; i < kPoseSums; ++i) red[i * kPoseThreads + tid] = acc[i];
    __syncthreads();
    if (tid < kPoseSums * 16) {
        const int i = tid >> 4, part = tid & 15;
        const double* src = red + i * kPoseThreads + part;
        double v = 0.0;
#pragma unroll 8
        for (int k = 0; k < kPoseThreads / 16; ++k) v += src[16 * k];
        s.part[i][part] = v;
    }
    __syncthreads();
    if (tid < kPoseSums) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) v += s.part[tid][k];
        s.tot[tid] = v;
    }
    __syncthreads();
}

// the pass just made was at s.par: its sums are the current ones
__device__ __forceinline__ void pose_keep_sums(PoseLds& s, const int tid)
{
    if (tid < kPoseSums) s.A[tid] = s.tot[tid];
    __syncthreads();
}

// The trial just evaluated (s.try_, s.tot) against the current cost: accepted -> it becomes s.par / s.A, lambda x 0.1 (floor 1e-12);
// rejected -> lambda x 10.  Returns whether the minimisation ended: an accepted step with a relative decrease below the function
// tolerance 1e-8 (Refiner.hpp:169), or lambda above 1e10 (uncounted, see ITERATION above).
__device__ __forceinline__ bool lm_judge(PoseLds& s, const int tid, LmState& lm, bool& accepted)
{
#pragma clang fp contract(fast)
    const double new_cost = s.tot[27];
    accepted = new_cost < lm.cost;
    if (accepted) {
        const double rel = (lm.cost - new_cost) / fmax(lm.cost, 1e-300);
        if (tid < 6) s.par[tid] = s.try_[tid];
        if (tid < kPoseSums) s.A[tid] = s.tot[tid];
        lm.cost = new_cost;
        lm.lambda = fmax(lm.lambda * 0.1, 1e-12);
        __syncthreads();
        ++lm.it;
        return rel < 1e-8;
    }
    lm.lambda *= 10.0;
    __syncthreads();
    if (lm.lambda > 1e10) return true;
    ++lm.it;
    return false;
}

// The next step from s.A at s.par by lane 0 -> s.try_.  A failed factorization counts as a rejected step: lambda up, try again.
// Returns whether the minimisation ended instead: max_iter reached, the gradient or the parameter tolerance met (1e-8 each, like the
// reference's settings, Refiner.hpp:169-171), or lambda above 1e10.
__device__ __forceinline__ bool lm_next_step(PoseLds& s, const int tid, LmState& lm, const int max_iter)
{
#pragma clang fp contract(fast)
    for (;;) {
        if (!(lm.it < max_iter)) return true;
        if (tid == 0) {
            double g[6], d[6];
            for (int a_ = 0; a_ < 6; ++a_) g[a_] = s.A[21 + a_];
            const bool ok = solve6(s.A, g, lm.lambda, d);
            double gn = 0, dn = 0, pn = 0;
            for (int a_ = 0; a_ < 6; ++a_) { gn = fmax(gn, fabs(g[a_])); dn += d[a_] * d[a_]; pn += s.par[a_] * s.par[a_]; }
            s.flag = !ok ? 2 : ((gn < 1e-8 * fmax(1.0, lm.cost) || sqrt(dn) < 1e-8 * (sqrt(pn) + 1e-8)) ? 1 : 0);
            for (int a_ = 0; a_ < 6; ++a_) s.try_[a_] = s.par[a_] + (ok ? d[a_] : 0.0);
        }
        __syncthreads();
        const int flag = s.flag;
        if (flag == 1) return true;
        if (flag != 2) return false;
        lm.lambda *= 10.0;
        if (lm.lambda > 1e10) return true;
        __syncthreads();
        ++lm.it;
    }
}

// column tid of the covariance (J^T W J)^-1 from s.A, by threads 0 .. 5; zero where the kernel rules it out or A is not SPD
__device__ __forceinline__ void pose_cov_column(const PoseLds& s, const int tid, const bool wanted, double* cov)
{
    if (tid < 6) {
        if (!wanted || !invert6_column(s.A, tid, cov)) for (int r = 0; r < 6; ++r) cov[6 * r + tid] = 0.0;
    }
}

// [R|t] of s.par (one thread)
__device__ __forceinline__ void pose_Rt(const PoseLds& s, double* Rt)
{
    double R[9];
    rodrigues(s.par, R);
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Rt[4 * i + j] = R[3 * i + j]; Rt[4 * i + 3] = s.par[3 + i]; }
}

__device__ __forceinline__ double pose_rmse(const double cost, const double n)
{
#pragma clang fp contract(fast)
    return n > 0.0 ? sqrt(cost / (2.0 * n)) : 0.0;
}

// The record is complete: every writer's stores to it (possibly pinned host memory) have left before `ready` is released.
__device__ __forceinline__ void pose_publish(const int tid, int32_t* ready)
{
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(ready, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Host: a pose kernel's dynamic LDS is more than the 64 KB a kernel gets by default; allowed once per kernel and device.
template <auto Kernel>
inline hipError_t pose_allow_lds()
{
    static bool attr_set[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!attr_set[dev]) {
        const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPoseRedBytes);
        if (e != hipSuccess) return e;
        attr_set[dev] = true;
    }
    return hipSuccess;
}

} // namespace clc

#endif

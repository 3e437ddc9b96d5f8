// capi_pose.hip -- pose scoring and the fixed-threshold robust solvers behind the C ABI (include/coloc_hip.h): residuals / scores of
// caller-supplied hypotheses, P3P and five-point RANSAC with a given threshold, the single-pose refinement.  The data-parallel core of
// SfM_Localizer::Localize (reference include/coloc/Localizer.hpp:82-93), RobustMatcher::filterEssential (RobustMatcher.hpp:153-186) and
// PoseRefiner::refinePose (Refiner.hpp:47-239); the a-contrario rule the reference actually runs is in pose_batch.hip.
#include "clc_ctx.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace clc;

extern "C" {

/* ---- PnP ------------------------------------------------------------------------------------ */

static int pnp_upload(clc_ctx* ctx, const double* h_Rt, int H, const double* h_X, const double* h_x, int N,
                      const double* h_K, size_t extra, double** dRt, double** dX, double** dx, double** dK, double** dExtra)
{
    PnpScoreDev dv;
    const int rc = ensure_pnp(ctx, [&](Carve& c) { dv.carve(c, (size_t)H, (size_t)N, extra); });
    if (rc != CLC_OK) return rc;
    *dRt = dv.Rt; *dX = dv.X; *dx = dv.x; *dK = dv.K; *dExtra = dv.extra;
    CLC_HIP(ctx, hipMemcpyAsync(*dRt, h_Rt, sizeof(double) * 12 * H, hipMemcpyHostToDevice, ctx->stream));
    if (N > 0) {
        CLC_HIP(ctx, hipMemcpyAsync(*dX, h_X, sizeof(double) * 3 * N, hipMemcpyHostToDevice, ctx->stream));
        CLC_HIP(ctx, hipMemcpyAsync(*dx, h_x, sizeof(double) * 2 * N, hipMemcpyHostToDevice, ctx->stream));
    }
    CLC_HIP(ctx, hipMemcpyAsync(*dK, h_K, sizeof(double) * 9, hipMemcpyHostToDevice, ctx->stream));
    return CLC_OK;
}

int clc_pnp_residuals(clc_ctx* ctx, const double* h_Rt, int H, const double* h_X, const double* h_x, int N,
                      const double* h_K, double* h_err)
{
    if (!ctx || H < 0 || N < 0 || !h_K || (H > 0 && !h_Rt) || (N > 0 && (!h_X || !h_x)) || (H > 0 && N > 0 && !h_err))
        return fail(ctx, CLC_ERR_BAD_ARG, "pnp_residuals: bad argument");
    if (H == 0 || N == 0) return CLC_OK;
    if (H > 65535) return fail(ctx, CLC_ERR_CAPACITY, "pnp_residuals: more than 65535 hypotheses per call");
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    double *dRt, *dX, *dx, *dK, *dE;
    const int rc = pnp_upload(ctx, h_Rt, H, h_X, h_x, N, h_K, (size_t)H * N, &dRt, &dX, &dx, &dK, &dE);
    if (rc != CLC_OK) return rc;
    CLC_HIP(ctx, launch_pnp_residuals(dRt, H, dX, dx, N, dK, dE, ctx->stream, &ctx->prof));
    CLC_HIP(ctx, hipMemcpyAsync(h_err, dE, sizeof(double) * (size_t)H * N, hipMemcpyDeviceToHost, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CLC_OK;
}

int clc_pnp_score(clc_ctx* ctx, const double* h_Rt, int H, const double* h_X, const double* h_x, int N,
                  const double* h_K, double thr2, int32_t* h_count, double* h_cost)
{
    if (!ctx || H < 0 || N < 0 || !h_K || (H > 0 && !h_Rt) || (N > 0 && (!h_X || !h_x)))
        return fail(ctx, CLC_ERR_BAD_ARG, "pnp_score: bad argument");
    if (H == 0) return CLC_OK;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    double *dRt, *dX, *dx, *dK, *dE;
    const int rc = pnp_upload(ctx, h_Rt, H, h_X, h_x, N, h_K, (size_t)2 * H, &dRt, &dX, &dx, &dK, &dE);
    if (rc != CLC_OK) return rc;
    double* d_cost = dE;
    int32_t* d_count = (int32_t*)(dE + H);
    CLC_HIP(ctx, launch_pnp_score(dRt, H, dX, dx, N, dK, thr2, d_count, d_cost, ctx->stream, &ctx->prof));
    if (h_cost) CLC_HIP(ctx, hipMemcpyAsync(h_cost, d_cost, sizeof(double) * H, hipMemcpyDeviceToHost, ctx->stream));
    if (h_count) CLC_HIP(ctx, hipMemcpyAsync(h_count, d_count, sizeof(int32_t) * H, hipMemcpyDeviceToHost, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CLC_OK;
}

static int epipolar_impl(clc_ctx* ctx, const double* h_F, int H, const double* h_x1, const double* h_x2, int N, double thr2,
                         double* h_err, int32_t* h_count, double* h_cost)
{
    if (!ctx || H < 0 || N < 0 || (H > 0 && !h_F) || (N > 0 && (!h_x1 || !h_x2))) return fail(ctx, CLC_ERR_BAD_ARG, "epipolar: bad argument");
    if (H == 0 || (N == 0 && h_err)) return CLC_OK;
    if (H > 65535) return fail(ctx, CLC_ERR_CAPACITY, "epipolar: more than 65535 hypotheses per call");
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    const size_t out = h_err ? (size_t)H * N : (size_t)2 * H;
    EpipolarDev dv;
    const int rc = ensure_pnp(ctx, [&](Carve& c) { dv.carve(c, (size_t)H, (size_t)N, out); });
    if (rc != CLC_OK) return rc;
    double *dF = dv.F, *d1 = dv.x1, *d2 = dv.x2, *dO = dv.out;
    CLC_HIP(ctx, hipMemcpyAsync(dF, h_F, sizeof(double) * 9 * H, hipMemcpyHostToDevice, ctx->stream));
    if (N > 0) {
        CLC_HIP(ctx, hipMemcpyAsync(d1, h_x1, sizeof(double) * 2 * N, hipMemcpyHostToDevice, ctx->stream));
        CLC_HIP(ctx, hipMemcpyAsync(d2, h_x2, sizeof(double) * 2 * N, hipMemcpyHostToDevice, ctx->stream));
    }
    if (h_err) {
        CLC_HIP(ctx, launch_epipolar(dF, H, d1, d2, N, thr2, dO, nullptr, nullptr, ctx->stream, &ctx->prof));
        CLC_HIP(ctx, hipMemcpyAsync(h_err, dO, sizeof(double) * (size_t)H * N, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        int32_t* dC = (int32_t*)(dO + H);
        CLC_HIP(ctx, launch_epipolar(dF, H, d1, d2, N, thr2, nullptr, dC, dO, ctx->stream, &ctx->prof));
        if (h_cost) CLC_HIP(ctx, hipMemcpyAsync(h_cost, dO, sizeof(double) * H, hipMemcpyDeviceToHost, ctx->stream));
        if (h_count) CLC_HIP(ctx, hipMemcpyAsync(h_count, dC, sizeof(int32_t) * H, hipMemcpyDeviceToHost, ctx->stream));
    }
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CLC_OK;
}

// S minimal samples of `k` distinct indices in [0, N) from a xorshift64* stream
static void draw_samples(uint64_t seed, int S, int N, std::vector<int32_t>& out, int k = 3)
{
    out.resize((size_t)k * S);
    uint64_t st = seed ? seed : 0x9E3779B97F4A7C15ull;
    auto next = [&]() { st ^= st >> 12; st ^= st << 25; st ^= st >> 27; return st * 0x2545F4914F6CDD1Dull; };   // xorshift64*
    for (int s = 0; s < S; ++s) {
        for (int j = 0; j < k; ++j) {
            int32_t v;
            bool again;
            do {
                v = (int32_t)(next() % (uint64_t)N);
                again = false;
                for (int m = 0; m < j && N > j; ++m) again = again || out[(size_t)k * s + m] == v;
            } while (again);
            out[(size_t)k * s + j] = v;
        }
    }
}

static int pnp_ransac_impl(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K,
                           const int32_t* h_samples, int S, uint64_t seed, double thr2, double* h_Rt, uint8_t* h_mask,
                           int* n_inliers, double* cost, double* h_all_Rt, double refine_huber = -1.0, double* h_cov = nullptr,
                           double* rmse = nullptr)
{
    if (!ctx || N < 0 || S < 0 || !h_K || (N > 0 && (!h_X || !h_x))) return fail(ctx, CLC_ERR_BAD_ARG, "pnp_ransac: bad argument");
    if (!pose_K_ok(h_K)) return fail(ctx, CLC_ERR_BAD_ARG, "pnp_ransac: K must be { fx, skew, cx; 0, fy, cy; 0, 0, 1 }");
    if (n_inliers) *n_inliers = 0;
    if (N < 3 || S == 0) { if (h_mask && N > 0) memset(h_mask, 0, (size_t)N); return CLC_OK; }
    if (S > 16384) return fail(ctx, CLC_ERR_CAPACITY, "pnp_ransac: more than 16384 samples per call");
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> drawn;
    if (!h_samples) { draw_samples(seed, S, N, drawn); h_samples = drawn.data(); }
    // RansacDev / RansacPin: [ X 3N | x 2N | K 16 | samples ] in, 4 slots of [R|t] per sample, [ result | refine record | mask ] out
    const bool refine = refine_huber > 0.0;
    const RansacDims dims{ (size_t)N, (size_t)S, 5, 1, 3, 4, 12, sizeof(PnpResult), refine ? sizeof(RefineOut) : 0 };
    RansacDev dv; RansacPin pin;
    int rc = ensure_pnp(ctx, [&](Carve& c) { dv.carve(c, dims); });
    if (rc == CLC_OK) rc = ensure_pinned(ctx, [&](Carve& c) { pin.carve(c, dims, false); });
    if (rc != CLC_OK) return rc;
    double *dX = dv.in.pts, *dx = dX + (size_t)3 * N, *dK = dv.in.K, *dRt = dv.models;
    uint8_t* dMask = dv.out.mask;
    // Inputs go into the pinned buffer and stay there: the first launch reads them over PCIe and stages them into
    // device memory itself, the last launch writes record + mask back into the pinned buffer.  No copy commands: a
    // pose solve is three (four with refinement) kernel launches and one stream synchronisation.
    memcpy(pin.in.pts, h_X, sizeof(double) * 3 * N);
    memcpy(pin.in.pts + (size_t)3 * N, h_x, sizeof(double) * 2 * N);
    memcpy(pin.in.K, h_K, sizeof(double) * 9);
    memcpy(pin.in.samples, h_samples, sizeof(int32_t) * 3 * S);
    PnpHostStage hs;
    hs.src = pin.in.pts;
    hs.n_doubles = (int)(pin.in.bytes / sizeof(double));
    hs.h_mask = pin.out.mask;
    hs.h_result = pin.out.result;
    CLC_HIP(ctx, launch_pnp_ransac(dX, dx, N, dK, dv.in.samples, S, thr2, dRt, dv.count, dv.cost, dMask, dv.out.result, ctx->stream, &ctx->prof, &hs));
    if (refine)
        CLC_HIP(ctx, launch_pnp_refine((const double*)dv.out.result /* PnpResult.Rt */, dX, dx, dMask, N, dK, refine_huber, 50, dv.out.ref, ctx->stream,
                                       &ctx->prof, &((const PnpResult*)dv.out.result)->h, pin.out.ref));
    if (h_all_Rt) CLC_HIP(ctx, hipMemcpyAsync(h_all_Rt, dRt, sizeof(double) * 48 * S, hipMemcpyDeviceToHost, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const PnpResult& r = *(const PnpResult*)pin.out.result;
    if (h_Rt) memcpy(h_Rt, r.Rt, sizeof r.Rt);
    if (h_mask) memcpy(h_mask, pin.out.mask, (size_t)N);
    if (n_inliers) *n_inliers = r.h >= 0 ? r.count : 0;
    if (cost) *cost = r.cost;
    if (refine) {
        const RefineOut& f = *(const RefineOut*)pin.out.ref;
        if (h_Rt) memcpy(h_Rt, f.Rt, sizeof f.Rt);
        if (h_cov) memcpy(h_cov, f.cov, sizeof f.cov);
        if (rmse) *rmse = f.rmse;
    }
    return CLC_OK;
}

int clc_epipolar_residuals(clc_ctx* ctx, const double* h_F, int H, const double* h_x1, const double* h_x2, int N, double* h_err)
{
    if (H > 0 && N > 0 && !h_err) return fail(ctx, CLC_ERR_BAD_ARG, "epipolar_residuals: null output");
    return epipolar_impl(ctx, h_F, H, h_x1, h_x2, N, 0.0, h_err, nullptr, nullptr);
}

int clc_epipolar_score(clc_ctx* ctx, const double* h_F, int H, const double* h_x1, const double* h_x2, int N, double thr2,
                       int32_t* h_count, double* h_cost)
{
    return epipolar_impl(ctx, h_F, H, h_x1, h_x2, N, thr2, nullptr, h_count, h_cost);
}

static int essential_impl(clc_ctx* ctx, const double* h_x1, const double* h_x2, int N, const double* h_K1, const double* h_K2,
                          const int32_t* h_samples, int S, uint64_t seed, double thr2, double* h_E, double* h_F, uint8_t* h_mask,
                          int* n_inliers, double* h_all_E)
{
    if (!ctx || N < 0 || S < 0 || !h_K1 || !h_K2 || (N > 0 && (!h_x1 || !h_x2))) return fail(ctx, CLC_ERR_BAD_ARG, "essential_ransac: bad argument");
    if (n_inliers) *n_inliers = 0;
    if (N < 5 || S == 0) { if (h_mask && N > 0) memset(h_mask, 0, (size_t)N); return CLC_OK; }
    if (S > 6000) return fail(ctx, CLC_ERR_CAPACITY, "essential_ransac: more than 6000 samples per call");
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> drawn;
    if (!h_samples) { draw_samples(seed, S, N, drawn, 5); h_samples = drawn.data(); }
    // RansacDev / RansacPin: [ x1 2N | x2 2N | K1 16 | K2 16 | samples ] in (one copy), 10 slots of { F, E } per sample,
    // [ result | mask ] out (one copy, over the inputs in the pinned block)
    const RansacDims dims{ (size_t)N, (size_t)S, 4, 2, 5, 10, 18, sizeof(EpiResult), 0 };
    RansacDev dv; RansacPin pin;
    int rc = ensure_pnp(ctx, [&](Carve& c) { dv.carve(c, dims); });
    if (rc == CLC_OK) rc = ensure_pinned(ctx, [&](Carve& c) { pin.carve(c, dims, true); });
    if (rc != CLC_OK) return rc;
    double *d1 = dv.in.pts, *d2 = d1 + (size_t)2 * N, *dFE = dv.models;
    memcpy(pin.in.pts, h_x1, sizeof(double) * 2 * N);
    memcpy(pin.in.pts + (size_t)2 * N, h_x2, sizeof(double) * 2 * N);
    memcpy(pin.in.K, h_K1, sizeof(double) * 9);
    memcpy(pin.in.K + 16, h_K2, sizeof(double) * 9);
    memcpy(pin.in.samples, h_samples, sizeof(int32_t) * 5 * S);
    CLC_HIP(ctx, hipMemcpyAsync(d1, pin.in.pts, pin.in.bytes, hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, launch_essential_ransac(d1, d2, N, dv.in.K, dv.in.K + 16, dv.in.samples, S, thr2, dFE, dv.count, dv.cost, dv.out.mask, dv.out.result, ctx->stream,
                                         &ctx->prof));
    CLC_HIP(ctx, hipMemcpyAsync(pin.out.result, dv.out.result, pin.out.bytes, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<double> fe;
    if (h_all_E) { fe.resize((size_t)180 * S); CLC_HIP(ctx, hipMemcpyAsync(fe.data(), dFE, sizeof(double) * 180 * S, hipMemcpyDeviceToHost, ctx->stream)); }
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const EpiResult& r = *(const EpiResult*)pin.out.result;
    if (h_E) memcpy(h_E, r.E, sizeof r.E);
    if (h_F) memcpy(h_F, r.F, sizeof r.F);
    if (h_mask) memcpy(h_mask, pin.out.mask, (size_t)N);
    if (n_inliers) *n_inliers = r.h >= 0 ? r.count : 0;
    if (h_all_E)
        for (size_t k = 0; k < (size_t)10 * S; ++k) memcpy(h_all_E + 9 * k, fe.data() + 18 * k + 9, sizeof(double) * 9);
    return CLC_OK;
}

int clc_essential_ransac(clc_ctx* ctx, const double* h_x1, const double* h_x2, int N, const double* h_K1, const double* h_K2,
                         const int32_t* h_samples, int S, uint64_t seed, double thr2, double* h_E, double* h_F,
                         uint8_t* h_inlier_mask, int* n_inliers)
{
    return essential_impl(ctx, h_x1, h_x2, N, h_K1, h_K2, h_samples, S, seed, thr2, h_E, h_F, h_inlier_mask, n_inliers, nullptr);
}

int clc_essential_fivepoint(clc_ctx* ctx, const double* h_x1, const double* h_x2, int N, const double* h_K1, const double* h_K2,
                            const int32_t* h_samples, int S, double* h_E_out)
{
    if (!h_samples || !h_E_out) return fail(ctx, CLC_ERR_BAD_ARG, "essential_fivepoint: bad argument");
    return essential_impl(ctx, h_x1, h_x2, N, h_K1, h_K2, h_samples, S, 0, 1.0, nullptr, nullptr, nullptr, nullptr, h_E_out);
}

int clc_pnp_ransac(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, const int32_t* h_samples,
                   int S, uint64_t seed, double thr2, double* h_Rt, uint8_t* h_inlier_mask, int* n_inliers, double* cost)
{
    return pnp_ransac_impl(ctx, h_X, h_x, N, h_K, h_samples, S, seed, thr2, h_Rt, h_inlier_mask, n_inliers, cost, nullptr);
}

int clc_pnp_refine(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, const uint8_t* h_inlier_mask,
                   const double* h_Rt_in, double huber_a, int max_iter, double* h_Rt_out, double* h_cov, double* rmse, int* iterations)
{
    if (!ctx || N < 0 || !h_K || !h_Rt_in || (N > 0 && (!h_X || !h_x))) return fail(ctx, CLC_ERR_BAD_ARG, "pnp_refine: bad argument");
    if (N < 3) return fail(ctx, CLC_ERR_BAD_ARG, "pnp_refine: needs at least 3 correspondences");
    if (!pose_K_ok(h_K)) return fail(ctx, CLC_ERR_BAD_ARG, "pnp_refine: K must be { fx, skew, cx; 0, fy, cy; 0, 0, 1 }");
    if (!(huber_a > 0.0)) huber_a = 16.0;          // ceres::HuberLoss(Square(4.0)), Refiner.hpp:122
    if (max_iter <= 0) max_iter = 50;
    CLC_HIP(ctx, hipSetDevice(ctx->device));
    // RefineDev / RefinePin: [ X 3N | x 2N | K 16 | Rt_in 12 | mask (N bytes) ] in (one copy), the record out (over the inputs in the pinned block)
    RefineDev dv; RefinePin pin;
    int rc = ensure_pnp(ctx, [&](Carve& c) { dv.carve(c, (size_t)N, true, sizeof(RefineOut)); });
    if (rc == CLC_OK) rc = ensure_pinned(ctx, [&](Carve& c) { pin.carve(c, (size_t)N, true, sizeof(RefineOut), true); });
    if (rc != CLC_OK) return rc;
    memcpy(pin.in.X, h_X, sizeof(double) * 3 * N);
    memcpy(pin.in.x, h_x, sizeof(double) * 2 * N);
    memcpy(pin.in.K, h_K, sizeof(double) * 9);
    memcpy(pin.in.Rt, h_Rt_in, sizeof(double) * 12);
    if (h_inlier_mask) memcpy(pin.in.mask, h_inlier_mask, (size_t)N);
    CLC_HIP(ctx, hipMemcpyAsync(dv.in.X, pin.in.X, pin.in.bytes, hipMemcpyHostToDevice, ctx->stream));
    CLC_HIP(ctx, launch_pnp_refine(dv.in.Rt, dv.in.X, dv.in.x, h_inlier_mask ? dv.in.mask : nullptr, N, dv.in.K, huber_a, max_iter, dv.out, ctx->stream, &ctx->prof));
    CLC_HIP(ctx, hipMemcpyAsync(pin.out, dv.out, sizeof(RefineOut), hipMemcpyDeviceToHost, ctx->stream));
    CLC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const RefineOut& r = *pin.out;
    if (h_Rt_out) memcpy(h_Rt_out, r.Rt, sizeof r.Rt);
    if (h_cov) memcpy(h_cov, r.cov, sizeof r.cov);
    if (rmse) *rmse = r.rmse;
    if (iterations) *iterations = r.iterations;
    return CLC_OK;
}

int clc_pnp_localize(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, const int32_t* h_samples,
                     int S, uint64_t seed, double thr2, double huber_a, double* h_Rt, double* h_cov, uint8_t* h_inlier_mask,
                     int* n_inliers, double* rmse)
{
    if (h_Rt) memset(h_Rt, 0, sizeof(double) * 12);
    if (h_cov) memset(h_cov, 0, sizeof(double) * 36);
    if (rmse) *rmse = 0.0;
    return pnp_ransac_impl(ctx, h_X, h_x, N, h_K, h_samples, S, seed, thr2, h_Rt, h_inlier_mask, n_inliers, nullptr, nullptr,
                           huber_a > 0.0 ? huber_a : 16.0, h_cov, rmse);
}

int clc_pnp_p3p(clc_ctx* ctx, const double* h_X, const double* h_x, int N, const double* h_K, const int32_t* h_samples, int S,
                double* h_Rt_out)
{
    if (!h_samples || !h_Rt_out) return fail(ctx, CLC_ERR_BAD_ARG, "pnp_p3p: bad argument");
    return pnp_ransac_impl(ctx, h_X, h_x, N, h_K, h_samples, S, 0, 1.0, nullptr, nullptr, nullptr, nullptr, h_Rt_out);
}

} // extern "C"

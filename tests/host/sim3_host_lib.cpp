// sim3_host_lib.cpp -- the host build of coloc_amd/csrc/sim3_math.h + clc_acr.h (g++ -ffp-contract=off) and, on top of it, the SEQUENTIAL
// statement of clc_sim3_acransac: the published a-contrario loop (one model after the other, a full sort per model) with the product's
// solver, residual, sampler and NFA term, a total order on (residual bits, index), then the acceptance rule and the refit.  The GPU tests
// compare the device with this bit for bit; tests/test_sim3_host.py holds it to a 50-digit reference.  Shares no code with the kernels
// beyond the two headers.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../coloc_amd/csrc/clc_acr.h"
#include "../../coloc_amd/csrc/sim3_math.h"
#include "../../coloc_amd/csrc/map_math.h"

using namespace clc;

namespace {

// log10 C(n, k) and log10 C(k, m) as OpenMVG tabulates them (float log10 table, float accumulation), the log10 being the product's
void tables(int n, int m, std::vector<float>& cn, std::vector<float>& ck)
{
    std::vector<float> lg((size_t)n + 2, 0.0f), prefix((size_t)n + 1, 0.0f);
    for (int k = 1; k <= n + 1; ++k) lg[k] = (float)clc_acr_log10((double)k);
    for (int i = 1; i <= n; ++i) prefix[i] = prefix[i - 1] + (lg[n - i + 1] - lg[i]);
    cn.assign((size_t)n + 1, 0.0f); ck.assign((size_t)n + 1, 0.0f);
    for (int k = 1; k < n; ++k) cn[k] = prefix[(n - k < k) ? n - k : k];
    for (int nn = 0; nn <= n; ++nn) {
        int kk = m;
        float r = 0.0f;
        if (!(kk >= nn || kk == 0)) {
            if (nn - kk < kk) kk = nn - kk;
            for (int i = 1; i <= kk; ++i) r += lg[nn - i + 1] - lg[i];
        }
        ck[nn] = r;
    }
}

void identity(double* s, double* R, double* t, double* A)
{
    *s = 1.0;
    for (int q = 0; q < 9; ++q) R[q] = q % 4 == 0 ? 1.0 : 0.0;
    for (int q = 0; q < 3; ++q) t[q] = 0.0;
    for (int q = 0; q < 12; ++q) A[q] = q % 5 == 0 ? 1.0 : 0.0;
}

} // namespace

extern "C" {

int sim3_host_minimal(const double* x9, const double* y9, double* A) { return sim3_minimal(x9, x9 + 3, x9 + 6, y9, y9 + 3, y9 + 6, A) ? 1 : 0; }
void sim3_host_residuals(const double* A, const double* x, const double* y, int n, double* out)
{
    for (int i = 0; i < n; ++i) out[i] = sim3_residual(A, x + 3 * i, y + 3 * i);
}
void sim3_host_from_model(const double* A, double* s, double* R, double* t) { sim3_from_model(A, s, R, t); }
int sim3_host_refit(const double* x, const double* y, const int32_t* list, int n, double* s, double* R, double* t, double* A)
{
    return sim3_refit(x, y, list, n, s, R, t, A) ? 1 : 0;
}
void sim3_host_apply_points(const double* A, const double* X, int n, double* out) { for (int i = 0; i < n; ++i) sim3_apply_point(A, X + 3 * i, out + 3 * i); }
void sim3_host_apply_pose(double s, const double* R, const double* t, double* Rt) { sim3_apply_pose(s, R, t, Rt); }
// the scale-only rule: X' = X * s, one multiplication per component; the pose through rescale_pose (map_math.h)
void sim3_host_scale_points(double s, const double* X, int n, double* out) { for (int i = 0; i < 3 * n; ++i) out[i] = X[i] * s; }
void sim3_host_scale_pose(double s, double* Rt) { rescale_pose(Rt, s); }
double sim3_host_box_volume(const double* y, int n)
{
    double bx[6];
    for (int q = 0; q < 3; ++q) {
        bx[q] = bx[3 + q] = y[q];
        for (int i = 1; i < n; ++i) { const double v = y[3 * i + q]; bx[q] = v < bx[q] ? v : bx[q]; bx[3 + q] = v > bx[3 + q] ? v : bx[3 + q]; }
    }
    return sim3_box_volume(bx);
}
double sim3_host_logalpha0(double V) { return clc_acr_log10(sim3_alpha0(V)); }

// The sequential statement.  Outputs as clc_sim3_acransac's; inliers: ascending residual.  Returns found (0 / 1).
int sim3_host_acransac(const double* x, const double* y, int n, int max_iteration, uint64_t seed, double precision, double* s, double* R,
                       double* t, double* A, uint8_t* mask, int32_t* inliers, int* n_inliers, double* error_max, double* min_nfa_out,
                       int* iterations, int* valid, int* refit)
{
    const int m = 3, M = 1;
    identity(s, R, t, A);
    *n_inliers = 0; *error_max = 0.0; *min_nfa_out = INFINITY; *iterations = 0; *valid = -1; *refit = 0;
    for (int i = 0; i < n; ++i) mask[i] = 0;
    if (n <= m || max_iteration == 0) return 0;
    const double V = sim3_host_box_volume(y, n);
    if (!sim3_volume_ok(V)) return 0;
    const double logalpha0 = clc_acr_log10(sim3_alpha0(V)), mult = 1.5, loge0 = clc_acr_log10((double)M * (double)(n - m));
    const double max_threshold = std::isinf(precision) ? INFINITY : precision * (1.0 * 1.0);
    std::vector<float> cn, ck;
    tables(n, m, cn, ck);
    std::vector<std::pair<uint64_t, uint32_t>> se((size_t)n);
    std::vector<uint32_t> index((size_t)n), inl;
    for (int i = 0; i < n; ++i) index[i] = (uint32_t)i;
    double min_nfa = INFINITY, emax = INFINITY, model[12];
    int reserve = max_iteration / 10, n_iter = max_iteration - reserve, best_iter = -1, iter = 0;
    bool ac_mode = std::isinf(precision);
    for (; iter < n_iter; ++iter) {
        uint32_t pos[3];
        clc_acr_sample(seed, (uint32_t)iter, (uint32_t)index.size(), m, pos);
        const uint32_t i0 = index[pos[0]], i1 = index[pos[1]], i2 = index[pos[2]];
        double cand[12];
        sim3_minimal(x + 3 * i0, x + 3 * i1, x + 3 * i2, y + 3 * i0, y + 3 * i1, y + 3 * i2, cand);
        bool better = false;
        if (cand[0] == cand[0]) {
            int cnt = 0;
            for (int i = 0; i < n; ++i) {
                const double r = sim3_residual(cand, x + 3 * i, y + 3 * i);
                cnt += r <= max_threshold ? 1 : 0;
                se[i] = { clc_acr_bits(r), (uint32_t)i };
            }
            if (!ac_mode && (double)cnt > 2.5 * (double)m) ac_mode = true;
            if (ac_mode) {
                std::sort(se.begin(), se.end());
                double best = INFINITY, bek = 0.0;
                int bk = m;
                for (int kk = m + 1; kk <= n; ++kk) {
                    const double r = clc_acr_from_bits(se[kk - 1].first);
                    if (!(r <= max_threshold)) continue;
                    const double v = clc_acr_nfa(loge0, logalpha0, mult, r, kk, m, cn[kk], ck[kk]);
                    if (v < best) { best = v; bk = kk; bek = r; }
                }
                if (best < min_nfa) {
                    better = true; min_nfa = best; emax = bek; best_iter = iter;
                    inl.resize((size_t)bk);
                    for (int i = 0; i < bk; ++i) inl[i] = se[i].second;
                    memcpy(model, cand, sizeof model);
                }
            }
        }
        if ((better && min_nfa < 0) || (iter + 1 == n_iter && reserve)) {
            if (inl.empty()) { n_iter++; reserve--; }
            else {
                index = inl;
                if (reserve) { n_iter = iter + 1 + reserve; reserve = 0; }
            }
        }
    }
    *iterations = iter;
    *min_nfa_out = min_nfa;
    const bool ok = min_nfa < 0.0 && !inl.empty();
    if (!ok || !sim3_accepted(best_iter, (int)inl.size())) return 0;
    *valid = best_iter;
    *n_inliers = (int)inl.size();
    *error_max = sqrt(emax) / 1.0;
    std::vector<int32_t> asc;
    for (size_t i = 0; i < inl.size(); ++i) { inliers[i] = (int32_t)inl[i]; mask[inl[i]] = 1; }
    for (int i = 0; i < n; ++i) if (mask[i]) asc.push_back(i);
    memcpy(A, model, sizeof model);
    sim3_from_model(A, s, R, t);
    *refit = sim3_refit(x, y, asc.data(), (int)asc.size(), s, R, t, A) ? 1 : 0;
    return 1;
}

} // extern "C"

// Host build of the bundle adjustment's statements (coloc_amd/csrc/ba_math.h) as a tiny shared library for the tests (tests/ba_host.py,
// tests/test_ba_host.py): what the kernels of map_ba.hip run per point and per entry, compiled by g++ without contraction, with the
// kernels' order of summation -- the points that carry an observation in ascending index, in chunks of kBaChunk, the chunks in order.
// libm's sincos / atan2 stand in for the device's, so results agree with the device to rounding, not bit for bit.  The
// Levenberg-Marquardt loop itself is tests/ba_host.py's.  Test infrastructure only.
#include <cmath>
#include <cstring>
#include <vector>
#include "../../coloc_amd/csrc/ba_math.h"

using namespace clc;

extern "C" {

int ba_host_sizeof_cams() { return (int)sizeof(BaCams); }
int ba_host_chunk() { return kBaChunk; }

void ba_host_from_Rt(const double* Rt, double* par) { ba_camera_from_Rt(Rt, par); }

// K: n_cams x 3 { focal, ppx, ppy }, par: n_cams x 6
void ba_host_cams_set(void* out, int n_cams, uint32_t mask, const double* K, const double* par)
{
    BaCams& cams = *(BaCams*)out;
    memset(&cams, 0, sizeof cams);
    cams.n_cams = n_cams;
    for (int c = 0; c < kBaCams; ++c) cams.slot[c] = -1;
    for (int c = 0; c < n_cams; ++c) {
        if (!((mask >> c) & 1u)) continue;
        cams.slot[c] = cams.n_slots++;
        for (int i = 0; i < 3; ++i) cams.K[c][i] = K[3 * c + i];
        for (int i = 0; i < 6; ++i) cams.par[c][i] = par[6 * c + i];
        ba_camera_update(cams, c);
    }
}

void ba_host_to_Rt(const void* in, int c, double* Rt) { const BaCams& cams = *(const BaCams*)in; ba_camera_to_Rt(cams.R[c], cams.par[c], Rt); }

int ba_host_invert3(const double* V, double lambda, double* inv) { return ba_invert3(V, lambda, inv) ? 1 : 0; }

// 1/2 sum rho; n_obs / n_pts: the observations and the points that count
double ba_host_cost(const void* in, int n_points, const double* X, const uint32_t* obs, const double* x, double a, int* n_obs, int* n_pts)
{
    const BaCams& cams = *(const BaCams*)in;
    double total = 0.0, chunk = 0.0;
    int k = 0, no = 0;
    for (int t = 0; t < n_points; ++t) {
        const uint32_t bits = ba_obs_bits(cams, obs[t]);
        if (!bits) continue;
        chunk += ba_point_cost(cams, bits, X + 3 * (size_t)t, x + 2 * (size_t)cams.n_cams * t, a);
        no += __builtin_popcount(bits);
        if (++k % kBaChunk == 0) { total += chunk; chunk = 0.0; }
    }
    if (k % kBaChunk) total += chunk;
    if (n_obs) *n_obs = no;
    if (n_pts) *n_pts = k;
    return total;
}

// One damped step at the iterate (cams, X): dc (6 per slot), dX (3 per point, zeros where a point does not count), the largest gradient
// component, |step|^2 and |parameters|^2 in the kernels' order.  0: a factorisation failed.
int ba_host_step(const void* in, int n_points, const double* X, const uint32_t* obs, const double* x, double a, double lambda, double* dc, double* dX,
                 double* gmax, double* dn, double* pn)
{
    const BaCams& cams = *(const BaCams*)in;
    const int n = 6 * cams.n_slots, E = ba_entries(n), sums = ba_tri(n) + 3 * n;
    int32_t cam_of_slot[kBaCams] = {};
    for (int c = 0; c < cams.n_cams; ++c) if (cams.slot[c] >= 0) cam_of_slot[cams.slot[c]] = c;
    std::vector<int> idx;
    for (int t = 0; t < n_points; ++t) if (ba_obs_bits(cams, obs[t])) idx.push_back(t);
    const size_t np = idx.size();
    std::vector<double> rec(np * cams.n_cams * kBaRec, 0.0), pt(np * kBaPoint, 0.0), sys(E, 0.0), part(E, 0.0);
    double gm = 0.0;
    bool ok = true;
    for (size_t k0 = 0; k0 < np; k0 += kBaChunk) {
        const size_t k1 = std::min(np, k0 + (size_t)kBaChunk);
        for (size_t k = k0; k < k1; ++k) {
            const int t = idx[k];
            double g1;
            ok = ba_point_build(cams, ba_obs_bits(cams, obs[t]), X + 3 * (size_t)t, x + 2 * (size_t)cams.n_cams * t, a, lambda,
                                &rec[k * cams.n_cams * kBaRec], &pt[k * kBaPoint], &g1) && ok;
            gm = fmax(gm, g1);
        }
        for (int e = 0; e < sums; ++e) {
            const BaEntry en = ba_entry(n, e, cam_of_slot);
            double acc = 0.0;
            for (size_t k = k0; k < k1; ++k)
                acc += ba_entry_term(en, ba_obs_bits(cams, obs[idx[k]]), &rec[k * cams.n_cams * kBaRec], &pt[k * kBaPoint]);
            part[e] = acc;
        }
        for (int e = 0; e < sums; ++e) sys[e] += part[e];
    }
    for (int a_ = 0; a_ < n; ++a_) gm = fmax(gm, fabs(sys[ba_tri(n) + 2 * n + a_]));
    *gmax = gm;
    memset(dX, 0, sizeof(double) * 3 * (size_t)n_points);
    if (!ok) return 0;
    std::vector<double> S((size_t)kBaDim * kBaDim, 0.0);
    if (!ba_system_solve(sys.data(), n, lambda, S.data(), dc)) return 0;
    double d2 = 0.0, p2 = 0.0;
    for (int c = 0; c < cams.n_cams; ++c) {
        if (cams.slot[c] < 0) continue;
        for (int i = 0; i < 6; ++i) { d2 += dc[6 * cams.slot[c] + i] * dc[6 * cams.slot[c] + i]; p2 += cams.par[c][i] * cams.par[c][i]; }
    }
    double dsum = 0.0, psum = 0.0;
    for (size_t k0 = 0; k0 < np; k0 += kBaChunk) {
        double dchunk = 0.0, pchunk = 0.0;
        for (size_t k = k0; k < std::min(np, k0 + (size_t)kBaChunk); ++k) {
            const int t = idx[k];
            ba_point_delta(cams, ba_obs_bits(cams, obs[t]), &rec[k * cams.n_cams * kBaRec], &pt[k * kBaPoint], dc, dX + 3 * (size_t)t);
            const double* d = dX + 3 * (size_t)t; const double* P = X + 3 * (size_t)t;
            dchunk += (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            pchunk += (P[0] * P[0] + P[1] * P[1]) + P[2] * P[2];
        }
        dsum += dchunk; psum += pchunk;
    }
    *dn = d2 + dsum; *pn = p2 + psum;
    return 1;
}

}

// sim3_asan_main.cpp -- a stand-alone program (its own main, nothing loaded into Python, no GPU) that drives coloc_amd/csrc/sim3_math.h
// and the host-side conversions of HIPRobustMatcher::matchMapsSimilarity (coloc_amd/host/HIPRobustMatcher.hpp) over their edge cases.
// tests/test_sim3_asan.py builds it with -fsanitize=address,undefined and runs it: every buffer below has exactly the size the code
// is documented to touch, so an access past it, a signed overflow or a misaligned access ends the run.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "HIPRobustMatcher.hpp"
#include "../../coloc_amd/csrc/sim3_math.h"

using namespace clc;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static double rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24) * 20.0 - 10.0; }

int main()
{
    unsigned seed = 12345u;
    // the minimal solver: heap blocks of exactly 3 doubles per point and 12 per model
    for (int it = 0; it < 200; ++it) {
        std::unique_ptr<double[]> p[6];
        for (auto& q : p) { q.reset(new double[3]); for (int c = 0; c < 3; ++c) q[c] = rnd(seed); }
        if (it % 10 == 1) for (int c = 0; c < 3; ++c) p[1][c] = p[0][c];                              // coincident
        if (it % 10 == 2) for (int c = 0; c < 3; ++c) p[5][c] = p[3][c] + 2.0 * (p[4][c] - p[3][c]);   // collinear in the old cloud
        std::unique_ptr<double[]> A(new double[12]);
        const bool ok = sim3_minimal(p[0].get(), p[1].get(), p[2].get(), p[3].get(), p[4].get(), p[5].get(), A.get());
        CHECK(ok == (A[0] == A[0]));
        if (it % 10 == 1 || it % 10 == 2) CHECK(!ok);
        if (!ok) continue;
        double s, R[9], t[3];
        sim3_from_model(A.get(), &s, R, t);
        CHECK(s > 0.0 && sim3_finite(s));
        // the sample's centroid is carried onto the old one: the residuals of the three points are bounded by the triangles' mismatch
        for (int k = 0; k < 3; ++k) CHECK(sim3_finite(sim3_residual(A.get(), p[k].get(), p[3 + k].get())));
    }
    // the refit over lists of every size around the partial sums, with and without an index list
    for (int n : { 1, 2, 3, 4, 127, 128, 129, 256, 257, 1000 }) {
        std::vector<double> x(3 * (size_t)n), y(3 * (size_t)n);
        const double c = std::cos(0.3), sn = std::sin(0.3);
        for (int i = 0; i < n; ++i) {
            for (int q = 0; q < 3; ++q) x[3 * i + q] = rnd(seed);
            y[3 * i] = 2.5 * (c * x[3 * i] - sn * x[3 * i + 1]) + 1.0;
            y[3 * i + 1] = 2.5 * (sn * x[3 * i] + c * x[3 * i + 1]) - 2.0;
            y[3 * i + 2] = 2.5 * x[3 * i + 2] + 3.0;
        }
        double s = 0.0, R[9], t[3], A[12];
        const bool ok = sim3_refit(x.data(), y.data(), nullptr, n, &s, R, t, A);
        CHECK(ok == (n >= 3));                                                                     // one or two points span no plane
        if (ok) CHECK(std::fabs(s - 2.5) < 1e-9 && std::fabs(t[2] - 3.0) < 1e-8);
        // every other point, through a list of exactly that many entries
        std::vector<int32_t> list;
        for (int i = 0; i < n; i += 2) list.push_back(i);
        const bool ok2 = sim3_refit(x.data(), y.data(), list.data(), (int)list.size(), &s, R, t, A);
        CHECK(ok2 == (list.size() >= 3));
        if (ok2) {
            std::vector<double> out(3);
            sim3_apply_point(A, x.data(), out.data());
            CHECK(std::fabs(out[0] - y[0]) < 1e-8 && std::fabs(out[2] - y[2]) < 1e-8);
            double Rt[12] = { 1, 0, 0, 0.5, 0, 1, 0, -0.5, 0, 0, 1, 2.0 };
            sim3_apply_pose(s, R, t, Rt);
            CHECK(sim3_finite(Rt[3]) && sim3_finite(Rt[11]));
        }
    }
    {   // a collinear cloud: refused, the outputs untouched
        std::vector<double> x(30), y(30);
        for (int i = 0; i < 10; ++i) for (int q = 0; q < 3; ++q) { x[3 * i + q] = i * (q + 1.0); y[3 * i + q] = 2.0 * i * (q + 1.0); }
        double s = -7.0, R[9], t[3], A[12];
        CHECK(!sim3_refit(x.data(), y.data(), nullptr, 10, &s, R, t, A) && s == -7.0);
    }
    {   // the box and the acceptance rule
        const double box[6] = { 0, 0, 0, 1, 2, 3 }, flat[6] = { 0, 0, 0, 1, 0, 3 };
        CHECK(sim3_box_volume(box) == 6.0 && sim3_volume_ok(6.0) && !sim3_volume_ok(sim3_box_volume(flat)) && !sim3_volume_ok(INFINITY));
        CHECK(!sim3_accepted(0, 7) && sim3_accepted(0, 8) && !sim3_accepted(-1, 100));
    }
    {   // matchMapsSimilarity's conversions: matches that name no landmark are left out; masks and lists of the exact sizes
        using openMVG::matching::IndMatch;
        std::vector<openMVG::Vec3> oldX, newX;
        for (int i = 0; i < 5; ++i) oldX.emplace_back(1.0 * i, 2.0 * i, 3.0 * i);
        for (int i = 0; i < 4; ++i) newX.emplace_back(-1.0 * i, 0.5 * i, 7.0);
        std::vector<IndMatch> common = { IndMatch(0, 3), IndMatch(4, 0), IndMatch(5, 1), IndMatch(2, 4), IndMatch(3, 3) };
        std::vector<double> xn, xo;
        std::vector<size_t> kept;
        coloc::hipgeom::sim3_pairs(oldX, newX, common, xn, xo, kept);
        CHECK(kept.size() == 3 && xn.size() == 9 && xo.size() == 9 && kept[2] == 4);
        CHECK(xo[3] == 4.0 && xo[5] == 12.0 && xn[3] == 0.0 && xn[5] == 7.0);
        std::vector<uint8_t> mask = { 1, 0, 1 };
        const std::vector<IndMatch> in = coloc::hipgeom::sim3_inlier_features(common, kept, mask);
        CHECK(in.size() == 2 && in[0] == IndMatch(0, 3) && in[1] == IndMatch(3, 3));
        mask.resize(1);                                                                            // a shorter mask reads no further
        CHECK(coloc::hipgeom::sim3_inlier_features(common, kept, mask).size() == 1);
        common.clear();
        coloc::hipgeom::sim3_pairs(oldX, newX, common, xn, xo, kept);
        CHECK(kept.empty() && xn.empty() && coloc::hipgeom::sim3_inlier_features(common, kept, mask).empty());
    }
    if (failures) return 1;
    std::puts("sim3_asan_main: ok");
    return 0;
}

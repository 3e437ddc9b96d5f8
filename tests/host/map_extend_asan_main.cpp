// map_extend_asan_main.cpp -- a stand-alone program (its own main, nothing loaded into Python, no GPU) that drives
// coloc_amd/csrc/extend_math.h and grow_point (map_math.h) over their edge cases.  tests/test_map_extend_asan.py builds it with
// -fsanitize=address,undefined and runs it: every buffer below is a heap block of exactly the size the code is documented to touch, so an
// access past it, a signed overflow or a misaligned access ends the run.
#include <cmath>
#include <cstdio>
#include <memory>

#include "../../coloc_amd/csrc/extend_math.h"

using namespace clc;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static double rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (double)(1u << 24) * 2.0 - 1.0; }

static void yaw_pose(double a, const double* C, double* Rt)
{
    const double c = std::cos(a), s = std::sin(a);
    const double R[9] = { c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c };
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) Rt[4 * r + q] = R[3 * r + q];
        Rt[4 * r + 3] = -((R[3 * r] * C[0] + R[3 * r + 1] * C[1]) + R[3 * r + 2] * C[2]);
    }
}

int main()
{
    unsigned seed = 2024u;
    for (int it = 0; it < 500; ++it) {
        std::unique_ptr<double[]> cam_a(new double[3]), cam_b(new double[3]), Rt_a(new double[12]), Rt_b(new double[12]), F(new double[9]);
        std::unique_ptr<double[]> P_a(new double[12]), P_b(new double[12]), xa(new double[2]), xb(new double[2]), X(new double[3]);
        cam_a[0] = 512.0 + 100.0 * rnd(seed); cam_a[1] = 320.0; cam_a[2] = 240.0;
        cam_b[0] = 512.0 + 100.0 * rnd(seed); cam_b[1] = 300.0 + 20.0 * rnd(seed); cam_b[2] = 250.0;
        const double Ca[3] = { rnd(seed), rnd(seed), rnd(seed) };
        // every tenth pair shares its centre, every seventh its whole pose
        const double Cb[3] = { it % 10 == 0 ? Ca[0] : Ca[0] + 0.6, Ca[1], Ca[2] };
        const double ya = 0.1 * rnd(seed), yb = it % 7 == 0 && it % 10 == 0 ? ya : ya + 0.03;
        yaw_pose(ya, Ca, Rt_a.get());
        yaw_pose(yb, Cb, Rt_b.get());
        fundamental_from_poses(cam_a.get(), Rt_a.get(), cam_b.get(), Rt_b.get(), F.get());
        for (int i = 0; i < 9; ++i) CHECK(std::isfinite(F[i]));
        // a world point in front of both cameras, its two pixels, the epipolar residual and the point back
        const double W[3] = { Ca[0] + 2.0 * rnd(seed), Ca[1] + 2.0 * rnd(seed), Ca[2] + 5.0 + 30.0 * std::fabs(rnd(seed)) };
        projective_equivalent(cam_a[0], cam_a[1], cam_a[2], Rt_a.get(), P_a.get());
        projective_equivalent(cam_b[0], cam_b[1], cam_b[2], Rt_b.get(), P_b.get());
        double ha[3], hb[3];
        for (int r = 0; r < 3; ++r) {
            ha[r] = P_a[4 * r] * W[0] + P_a[4 * r + 1] * W[1] + P_a[4 * r + 2] * W[2] + P_a[4 * r + 3];
            hb[r] = P_b[4 * r] * W[0] + P_b[4 * r + 1] * W[1] + P_b[4 * r + 2] * W[2] + P_b[4 * r + 3];
        }
        xa[0] = ha[0] / ha[2]; xa[1] = ha[1] / ha[2]; xb[0] = hb[0] / hb[2]; xb[1] = hb[1] / hb[2];
        const double l[3] = { F[0] * xa[0] + F[1] * xa[1] + F[2], F[3] * xa[0] + F[4] * xa[1] + F[5], F[6] * xa[0] + F[7] * xa[1] + F[8] };
        double nF = 0.0;
        for (int i = 0; i < 9; ++i) nF += F[i] * F[i];
        CHECK(std::fabs(xb[0] * l[0] + xb[1] * l[1] + l[2]) <= 1e-9 * std::sqrt(nF) * (1.0 + xa[0] * xa[0] + xa[1] * xa[1]) * (1.0 + xb[0] * xb[0] + xb[1] * xb[1]));
        std::unique_ptr<float[]> L(new float[3]);
        const bool line = guided_line(F.get(), xa[0], xa[1], L.get());
        if (it % 10 == 0) CHECK(!line || std::sqrt(nF) < 1e-12);                 // one centre: no line, up to the rounding of t
        const bool ok = grow_point(cam_a.get(), cam_b.get(), P_a.get(), P_b.get(), Rt_a.get(), Rt_b.get(), xa.get(), xb.get(), X.get());
        if (ok) for (int r = 0; r < 3; ++r) CHECK(std::fabs(X[r] - W[r]) <= 1e-6 * (1.0 + std::fabs(W[r])));
        if (it % 10 == 0) CHECK(!ok);                                            // parallel rays: under 2 degrees
    }
    // the mask's boundaries
    CHECK(extend_keeps(-1, -1, 0u, 0) && !extend_keeps(-1, -1, 1u, 0) && extend_keeps(-1, -1, 512u, kExtendMaxDistance));
    CHECK(!extend_keeps(0, -1, 0u, 64) && !extend_keeps(-1, 0, 0u, 64) && !extend_keeps(-1, -1, 65535u, kExtendMaxDistance));
    CHECK(!extend_keeps(2147483647, -1, 0u, 64) && extend_keeps(-2147483647 - 1, -2147483647 - 1, 64u, 64));
    if (failures) return 1;
    std::printf("map_extend_asan_main: ok\n");
    return 0;
}

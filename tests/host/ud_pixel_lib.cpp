// Host build of Pinhole_Intrinsic_Radial_K3::get_ud_pixel (coloc_amd/host/coloc_hip_geometry.hpp) for tests/test_track_abi.py: the member
// HIPLocalizer::setupTracks calls, against which tests/track_host.py's numpy restatement is held bit for bit.
#include "../../coloc_amd/host/coloc_hip_geometry.hpp"

extern "C" void ud_pixel_host(const double* cam /* focal, ppx, ppy, k1, k2, k3 */, const double* p, int n, double* out)
{
    const openMVG::cameras::Pinhole_Intrinsic_Radial_K3 c(0, 0, cam[0], cam[1], cam[2], cam[3], cam[4], cam[5]);
    for (int i = 0; i < n; ++i) {
        const openMVG::Vec2 u = c.get_ud_pixel(openMVG::Vec2(p[2 * i], p[2 * i + 1]));
        out[2 * i] = u[0];
        out[2 * i + 1] = u[1];
    }
}

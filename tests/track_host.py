"""Localizer::setupTracks in numpy float64 (reference include/coloc/Localizer.hpp:59-75), the yardstick of the device track kernel.

Written from the reference's loop and from Pinhole_Intrinsic_Radial_K3::get_ud_pixel (coloc_amd/host/coloc_hip_geometry.hpp:97-135); shares
no code with coloc_amd/csrc/gather.hip.  Every operation is an IEEE + - x / sqrt on float32 / float64 arrays in the reference's order, so
results are compared bit for bit.
"""
import math

import numpy as np

DISTORTIONS = [(0.0, 0.0, 0.0), (-0.28, 0.07, 0.0), (0.1, -0.02, 0.003)]


def level_scales(levels=8):
    """static_cast<float>(std::pow(1.2f, level)): pow(float, integer) is evaluated in double (GPUDetector.hpp:173)."""
    base = float(np.float32(1.2))
    return np.array([np.float32(math.pow(base, float(l))) for l in range(levels)], dtype=np.float32)


def feature_positions(kps):
    """(n, 2) float32: scale * (float)x, scale * (float)y (GPUDetector.hpp:172-179)."""
    s = level_scales(256 if len(kps) and int(kps["scale"].max()) >= 8 else 8)[kps["scale"]]
    out = np.empty((len(kps), 2), dtype=np.float32)
    out[:, 0] = s * kps["x"].astype(np.float32)
    out[:, 1] = s * kps["y"].astype(np.float32)
    return out


def _disto(r2, k):
    t = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
    return r2 * t * t


def _bisection_radius_solve(r2, k, epsilon=1e-10):
    """elementwise bisection_radius_solve: every element walks its own loops (masks), same operations in the same order"""
    lower = r2.copy()
    upper = r2.copy()
    while True:
        act = _disto(lower, k) > r2
        if not act.any():
            break
        lower[act] = lower[act] / 1.05
    while True:
        act = _disto(upper, k) < r2
        if not act.any():
            break
        upper[act] = upper[act] * 1.05
    while True:
        act = epsilon < upper - lower
        if not act.any():
            break
        mid = .5 * (lower + upper)
        hi = _disto(mid, k) > r2
        up = act & hi
        lo = act & ~hi
        upper[up] = mid[up]
        lower[lo] = mid[lo]
    return .5 * (lower + upper)


def get_ud_pixel(p, cam):
    """p (n, 2) float64 distorted pixels, cam = (focal, ppx, ppy, k1, k2, k3) -> (n, 2) undistorted pixels."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    f, ppx, ppy = (np.float64(v) for v in cam[:3])
    k = [np.float64(v) for v in cam[3:6]]
    c0 = (p[:, 0] - ppx) / f
    c1 = (p[:, 1] - ppy) / f
    r2 = c0 * c0 + c1 * c1
    radius = np.ones_like(r2)
    nz = r2 != 0.0
    if nz.any():
        r2n = r2[nz]
        radius[nz] = np.sqrt(_bisection_radius_solve(r2n, k) / r2n)
    out = np.empty_like(p)
    out[:, 0] = f * (radius * c0) + ppx
    out[:, 1] = f * (radius * c1) + ppy
    return out


def build_tracks(match, map_X, cam, kps=None, feat=None, count=None):
    """matchFeaturesWithMap's accepted queries in ascending order (GPUMatcher.hpp:263-266) through setupTracks.

    match (nq,) int32: map row or anything outside [0, len(map_X)) for "no match"; count: rows q >= count are ignored.
    Returns (track_query, track_map, X (N, 3), x (N, 2))."""
    match = np.asarray(match, dtype=np.int32)
    map_X = np.asarray(map_X, dtype=np.float64).reshape(-1, 3)
    nq = len(match) if count is None else min(len(match), int(count))
    m = match[:nq]
    q = np.nonzero((m >= 0) & (m < len(map_X)))[0].astype(np.int32)
    tm = m[q].astype(np.int32)
    if kps is not None:
        pos = feature_positions(kps[q])
    else:
        pos = np.asarray(feat, dtype=np.float32)[q, :2]
    x = get_ud_pixel(pos.astype(np.float64), cam)
    return q, tm, map_X[tm].copy(), x

"""The gather of RobustMatcher::computeRelativePose in numpy float64 (reference include/coloc/RobustMatcher.hpp:372-424, the loop at
:393-398), the yardstick of the device pair kernel.

Written from the reference's loop: for every putative match of the pair, in the order GPUMatcher::computeMatches emits them
(IndMatch(i, h_matches[i]) for ascending i, GPUMatcher.hpp:215-220), the two feature positions, each undistorted through its own camera's
Pinhole_Intrinsic_Radial_K3::get_ud_pixel.  Built on tests/track_host.py's feature_positions / get_ud_pixel; shares no code with
coloc_amd/csrc/gather.hip.  Results are compared bit for bit.
"""
import numpy as np

import track_host


def _positions(rows, kps, feat):
    """float32 feature positions of the given rows: level-local keypoints scaled, or a block of positions (first two columns)"""
    if (kps is None) == (feat is None):
        raise ValueError("exactly one of kps / feat per camera")
    if kps is not None:
        return track_host.feature_positions(kps[rows])
    return np.asarray(feat, dtype=np.float32)[rows, :2]


def build_pairs(match, nt, camA, camB, kpsA=None, featA=None, kpsB=None, featB=None, countA=None, countB=None):
    """match (nq,) int32: query row of camera A -> train row of camera B, anything outside [0, min(nt, countB)) for "no match"; rows
    q >= countA are ignored.  cam* = (focal, ppx, ppy, k1, k2, k3).  Returns (pair_q, pair_t, x1 (N, 2), x2 (N, 2)) in ascending q."""
    match = np.asarray(match, dtype=np.int32)
    nq = len(match) if countA is None else min(len(match), int(countA))
    nt = int(nt) if countB is None else min(int(nt), int(countB))
    m = match[:nq]
    q = np.nonzero((m >= 0) & (m < nt))[0].astype(np.int32)
    t = m[q].astype(np.int32)
    x1 = track_host.get_ud_pixel(_positions(q, kpsA, featA).astype(np.float64), camA)
    x2 = track_host.get_ud_pixel(_positions(t, kpsB, featB).astype(np.float64), camB)
    return q, t, x1, x2

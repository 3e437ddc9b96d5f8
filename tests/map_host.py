"""The map's tracks and seed landmarks as a plain Python / numpy statement, the yardstick of coloc_amd/csrc/map_build.hip
(include/coloc_hip.h: clc_tracks_build_dev, clc_map_build_dev): a dict union-find over the nodes (camera, row), the filter, the id order,
the seed gather and the acceptance.  Shares no code with the kernels.  The fp64 arithmetic of one landmark is NOT restated here: it is the
host build of coloc_amd/csrc/map_math.h (tests/host/map_math_lib.cpp), which the device is compared with bit for bit, and which
tests/test_map_host.py holds to numpy's SVD."""
import ctypes as C
import os
import subprocess

import numpy as np

import track_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = []


def lib():
    if not _LIB:
        out = os.path.join(ROOT, "tests", "host", "libmap_math_host.so")
        src = os.path.join(ROOT, "tests", "host", "map_math_lib.cpp")
        hdr = os.path.join(ROOT, "coloc_amd", "csrc", "map_math.h")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        _LIB.append(C.CDLL(out))
    return _LIB[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))


def projection(cam, Rt):
    """P = K [R|t], K = { focal, 0, ppx; 0, focal, ppy; 0, 0, 1 } (plain numpy: for the tests' own references)"""
    K = np.array([[cam[0], 0.0, cam[1]], [0.0, cam[0], cam[2]], [0.0, 0.0, 1.0]])
    return K @ np.asarray(Rt, dtype=np.float64).reshape(3, 4)


def design(P1, x1, P2, x2):
    D = np.zeros(16)
    lib().map_math_host_design(_p(_f64(P1, 12)), _p(_f64(x1, 2)), _p(_f64(P2, 12)), _p(_f64(x2, 2)), _p(D))
    return D.reshape(4, 4)


def triangulate(P1, P2, x1, x2):
    """the host DLT of n correspondences -> (X (n, 3), ok (n,) bool)"""
    x1, x2 = _f64(x1, (-1, 2)), _f64(x2, (-1, 2))
    X, ok = np.zeros((len(x1), 3)), np.zeros(len(x1), dtype=np.uint8)
    lib().map_math_host_triangulate(_p(_f64(P1, 12)), _p(_f64(P2, 12)), _p(x1), _p(x2), C.c_int(len(x1)), _p(X), _p(ok))
    return X, ok.astype(bool)


def seed_points(cam_i, cam_j, Rt_i, Rt_j, x_i, x_j):
    """the seed kernel's statement on n pairs of undistorted pixels -> (X (n, 3), accepted (n,) bool)"""
    x_i, x_j = _f64(x_i, (-1, 2)), _f64(x_j, (-1, 2))
    X, ok = np.zeros((len(x_i), 3)), np.zeros(len(x_i), dtype=np.uint8)
    lib().map_math_host_seed_points(_p(_f64(cam_i[:3], 3)), _p(_f64(cam_j[:3], 3)), _p(_f64(Rt_i, 12)), _p(_f64(Rt_j, 12)), _p(x_i), _p(x_j),
                                    C.c_int(len(x_i)), _p(X), _p(ok))
    return X, ok.astype(bool)


def accepted(Rt_i, Rt_j, X):
    return bool(lib().map_math_host_accepted(_p(_f64(Rt_i, 12)), _p(_f64(Rt_j, 12)), _p(_f64(X, 3))))


def pose_center(R, t):
    Cc = np.zeros(3)
    lib().map_math_host_pose_center(_p(_f64(R, 9)), _p(_f64(t, 3)), _p(Cc))
    return Cc


def seed_poses(Ro, Co, Rrel, Crel, scale):
    Rt_i, Rt_j = np.zeros(12), np.zeros(12)
    lib().map_math_host_seed_poses(_p(_f64(Ro, 9)), _p(_f64(Co, 3)), _p(_f64(Rrel, 9)), _p(_f64(Crel, 3)), C.c_double(scale), _p(Rt_i), _p(Rt_j))
    return Rt_i.reshape(3, 4), Rt_j.reshape(3, 4)


# ---- the tracks --------------------------------------------------------------------------------------------------------------------

def pair_edges(pair):
    """the (q, t) edges a pair names: dict(cam_a, cam_b, q, t [, count, index]) -- the first min(len, count) entries of q / t, or those
    the index list picks (an index outside the lists names no edge)"""
    q, t = np.asarray(pair["q"], dtype=np.int64), np.asarray(pair["t"], dtype=np.int64)
    if pair.get("index") is not None:
        idx = np.asarray(pair["index"], dtype=np.int64)
        n = len(idx) if pair.get("count") is None else max(min(len(idx), int(pair["count"])), 0)
        idx = idx[:n]
        idx = idx[(idx >= 0) & (idx < len(q))]
        return q[idx], t[idx]
    n = len(q) if pair.get("count") is None else max(min(len(q), int(pair["count"])), 0)
    return q[:n], t[:n]


def build_tracks(rows, pairs):
    """-> track_feat (n_tracks, n_cams) int32, row or -1.  A dict union-find over (camera, row); a component with two rows of one
    camera is dropped whole; the survivors in ascending order of their smallest (camera, row)."""
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for p in pairs:
        a, b = int(p["cam_a"]), int(p["cam_b"])
        assert 0 <= a < b < len(rows)
        for q, t in zip(*pair_edges(p)):
            if not (0 <= q < rows[a] and 0 <= t < rows[b]):
                continue
            u, v = (a, int(q)), (b, int(t))
            parent.setdefault(u, u)
            parent.setdefault(v, v)
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[ru] = rv
    comps = {}
    for node in parent:
        comps.setdefault(find(node), []).append(node)
    kept = []
    for nodes in comps.values():
        cams = [c for c, _ in nodes]
        if len(nodes) >= 2 and len(set(cams)) == len(cams):
            kept.append(sorted(nodes))
    kept.sort(key=lambda nodes: nodes[0])
    table = np.full((len(kept), len(rows)), -1, dtype=np.int32)
    for k, nodes in enumerate(kept):
        for c, r in nodes:
            table[k, c] = r
    return table


def positions(cam_spec):
    """dict(kps= | feat=) -> (n, 2) float32 feature positions"""
    if cam_spec.get("kps") is not None:
        return track_host.feature_positions(cam_spec["kps"])
    return np.asarray(cam_spec["feat"], dtype=np.float32)[:, :2]


def build_map(rows, pairs, cams, seed_pair, Rt_a, Rt_b):
    """-> dict(track_feat, map_track, map_row, X): the tracks, then for every track with both seed cameras, in id order, get_ud_pixel of
    the two rows, the host build of map_math.h, and the accepted points.  cams[c] = dict(cam=(focal, ppx, ppy, k1, k2, k3), kps= | feat=)."""
    table = build_tracks(rows, pairs)
    a, b = int(pairs[seed_pair]["cam_a"]), int(pairs[seed_pair]["cam_b"])
    ids = np.nonzero((table[:, a] >= 0) & (table[:, b] >= 0))[0].astype(np.int32) if len(table) else np.zeros(0, dtype=np.int32)
    ra, rb = table[ids, a], table[ids, b]
    xa = track_host.get_ud_pixel(positions(cams[a])[ra].astype(np.float64), cams[a]["cam"])
    xb = track_host.get_ud_pixel(positions(cams[b])[rb].astype(np.float64), cams[b]["cam"])
    X, ok = seed_points(cams[a]["cam"], cams[b]["cam"], Rt_a, Rt_b, xa, xb)
    return dict(track_feat=table, map_track=ids[ok], map_row=ra[ok].astype(np.int32), X=X[ok].copy(), seed_tracks=ids, seed_X=X, seed_ok=ok)

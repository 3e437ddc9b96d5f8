"""The map extension on the host: THE statement clc_map_extend_dev is held to (include/coloc_hip.h), composed of the statements the
steps already have, and the scenes the tests share.

  F           the g++ build of coloc_amd/csrc/extend_math.h (tests/host/map_extend_lib.cpp): not restated here
  guided      tests/guided_host.py::statement under that F
  mask        three numpy comparisons (held to extend_keeps of the g++ build in tests/test_map_extend_host.py)
  one-to-one  tests/unique_host.py::unique
  point       tests/track_host.py::get_ud_pixel, then grow_point of coloc_amd/csrc/map_math.h in the g++ build
  append      a Python loop in ascending q

Everything is IEEE arithmetic in a fixed order or integer work, so the device results are compared bit for bit.  A view is a dict:
desc (n, 64) uint8, feat (n, 2) float32 or kps (detector keypoints), cam (focal, ppx, ppy, k1, k2, k3), Rt (3, 4), track (n,) int32 or
None, count (the device-side row count) or None."""
import ctypes as C
import os
import subprocess

import numpy as np

import guided_host as gh
import track_host
import unique_host as uh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = []
MAX_DISTANCE = 512
W, H = 640, 480
CAM = (512.0, 320.0, 240.0, 0.0, 0.0, 0.0)
CAM_K1 = (512.0, 320.0, 240.0, -0.05, 0.0, 0.0)
BAND, THRESHOLD, CAP = 2.0, 40, 64                      # the main case's parameters
CLASSES = ("guided", "over_cap", "masked_a", "masked_b", "lost_claim", "refused", "added")


def lib():
    if not _LIB:
        out = os.path.join(ROOT, "tests", "host", "libmap_extend_host.so")
        src = os.path.join(ROOT, "tests", "host", "map_extend_lib.cpp")
        hdrs = [os.path.join(ROOT, "coloc_amd", "csrc", h) for h in ("extend_math.h", "map_math.h", "guided_math.h", "unique_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        L = C.CDLL(out)
        assert L.map_extend_host_max_distance() == MAX_DISTANCE
        _LIB.append(L)
    return _LIB[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))


def fundamental(cam_a, Rt_a, cam_b, Rt_b):
    """(3, 3): fundamental_from_poses of the g++ build"""
    F = np.zeros(9)
    lib().map_extend_host_fundamental(_p(_f64(cam_a[:3], 3)), _p(_f64(Rt_a, 12)), _p(_f64(cam_b[:3], 3)), _p(_f64(Rt_b, 12)), _p(F))
    return F.reshape(3, 3)


def cxx_keeps(track_a, track_b, best, max_distance):
    ta, tb = np.ascontiguousarray(track_a, dtype=np.int32), np.ascontiguousarray(track_b, dtype=np.int32)
    best = np.ascontiguousarray(best, dtype=np.uint32)
    out = np.zeros(len(ta), dtype=np.uint8)
    lib().map_extend_host_keeps(_p(ta), _p(tb), _p(best), len(ta), int(max_distance), _p(out))
    return out.astype(bool)


def points(cam_a, cam_b, Rt_a, Rt_b, x_a, x_b):
    """grow_point of every pair of undistorted pixels: (ok (n,) bool, X (n, 3))"""
    x_a, x_b = _f64(x_a, (-1, 2)), _f64(x_b, (-1, 2))
    ok, X = np.zeros(len(x_a), dtype=np.uint8), np.zeros((len(x_a), 3))
    if len(x_a):
        lib().map_extend_host_points(_p(_f64(cam_a[:3], 3)), _p(_f64(cam_b[:3], 3)), _p(_f64(Rt_a, 12)), _p(_f64(Rt_b, 12)), _p(x_a), _p(x_b),
                                     len(x_a), _p(ok), _p(X))
    return ok.astype(bool), X


def _positions(v, rows):
    kps, feat = v.get("kps"), v.get("feat")
    pos = track_host.feature_positions(kps[rows]) if kps is not None else np.asarray(feat, dtype=np.float32)[rows, :2]
    return track_host.get_ud_pixel(pos.astype(np.float64), v["cam"])


def statement(a, b, band, threshold, max_distance, map_n, maxkp, update_tracks=True):
    """One job on a map of map_n rows in a context of capacity maxkp.  Returns every intermediate list: F, guided / best (the guided
    match), masked, unique (the one-to-one list), ok / X_all (grow_point per query; False / 0 where the entry is -1), accepted (the
    unbounded result: every accepted q ascending), new_q, new_t, X, n_guided, n_added, n_dropped, track_a / track_b (as the call leaves
    them; None where the view has none), classes (dict over CLASSES; the six behind `guided` partition it)."""
    na, nb = len(a["desc"]), len(b["desc"])
    F = fundamental(a["cam"], a["Rt"], b["cam"], b["Rt"])
    g = gh.statement(a["desc"], b["desc"], F, band, threshold, a["cam"], b["cam"], kps_a=a.get("kps"), feat_a=a.get("feat"),
                     kps_b=b.get("kps"), feat_b=b.get("feat"), count_a=a.get("count"), count_b=b.get("count"))
    guided, best = g["match"], g["best"]
    ta = np.asarray(a["track"], dtype=np.int32) if a.get("track") is not None else np.full(na, -1, dtype=np.int32)
    tb = np.asarray(b["track"], dtype=np.int32) if b.get("track") is not None else np.full(nb, -1, dtype=np.int32)
    hit = guided >= 0
    t_of = np.where(hit, guided, 0)
    by_a = hit & (ta >= 0)
    by_b = hit & ~by_a & (tb[t_of] >= 0 if nb else np.zeros(na, dtype=bool))
    by_cap = hit & ~by_a & ~by_b & (best.astype(np.int64) > max_distance)
    masked = np.where(hit & ~by_a & ~by_b & ~by_cap, guided, -1).astype(np.int32)
    unique, _ = uh.unique(masked, best, nb)
    lost = (masked >= 0) & (unique < 0)
    q = np.nonzero(unique >= 0)[0]
    ok, X_all = np.zeros(na, dtype=bool), np.zeros((na, 3))
    if len(q):
        okq, Xq = points(a["cam"], b["cam"], a["Rt"], b["Rt"], _positions(a, q), _positions(b, unique[q]))
        ok[q], X_all[q] = okq, Xq
    accepted = np.nonzero(ok)[0].astype(np.int32)
    room = max(int(maxkp) - int(map_n), 0)
    new_q = accepted[:room]
    new_t = unique[new_q].astype(np.int32)
    track_a = ta.copy() if a.get("track") is not None else None
    track_b = tb.copy() if b.get("track") is not None else None
    if update_tracks:
        rows = map_n + np.arange(len(new_q), dtype=np.int32)
        if track_a is not None:
            track_a[new_q] = rows
        if track_b is not None:
            track_b[new_t] = rows
    classes = dict(guided=int(hit.sum()), over_cap=int(by_cap.sum()), masked_a=int(by_a.sum()), masked_b=int(by_b.sum()),
                   lost_claim=int(lost.sum()), refused=int(len(q) - ok.sum()), added=int(ok.sum()))
    return dict(F=F, guided=guided, best=best, masked=masked, unique=unique, ok=ok, X_all=X_all, accepted=accepted, new_q=new_q, new_t=new_t,
                X=X_all[new_q].copy(), n_guided=int(hit.sum()), n_added=len(new_q), n_dropped=len(accepted) - len(new_q), track_a=track_a,
                track_b=track_b, classes=classes)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def pose(yaw, C_):
    """[R|t] of a camera at centre C_ turned by `yaw` about y; t = -R C, each row ((R0 C0 + R1 C1) + R2 C2) negated"""
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    t = np.array([-((R[i, 0] * C_[0] + R[i, 1] * C_[1]) + R[i, 2] * C_[2]) for i in range(3)])
    return np.column_stack([R, t])


def _project(cam, Rt, X):
    """distorted pixels of world points (Pinhole_Intrinsic_Radial_K3: the distortion acts on the normalised point) and their depths"""
    Xc = X @ Rt[:, :3].T + Rt[:, 3]
    c = Xc[:, :2] / Xc[:, 2:3]
    r2 = (c * c).sum(1)
    k1, k2, k3 = cam[3:6]
    c = c * (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3)))[:, None]
    return c * cam[0] + np.array([cam[1], cam[2]]), Xc[:, 2]


def _flip(rng, row, n_bits):
    out = row.copy()
    for bit in rng.choice(512, size=n_bits, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


TRACK_EVERY = (4, 10, 7)                                 # view k: every TRACK_EVERY[k]-th common row is a landmark already


def make_views(rows, seed, cams=None, map_n=40, noise=0.3, doubles=True):
    """len(rows) views of one scene, view k 0.6 k along x with a yaw of 0.03 k, rows[k] rows each.  The common points (three quarters of
    the smallest view; all of it below four rows) lie 3 - 40 deep in front of view 0 and project into every image, so both sides of the 2
    degree rule occur; every view sees them with `noise` pixels of noise and a descriptor 0 - 11 bits from the scene's, in an order of
    its own.  Every TRACK_EVERY[k]-th common row of view k is tracked (distinct map rows below map_n).  In view 0 a tenth of the common
    rows appear TWICE, a quarter pixel apart (doubles), where it has rows to spare.  The other rows of a view are random descriptors at
    random positions.  Returns (views, info): info[k]["common"][i] = the row of common point i in view k."""
    rng = np.random.RandomState(seed)
    n_views = len(rows)
    cams = cams or [CAM] * n_views
    Rts = [pose(0.03 * k, (0.6 * k, 0.0, 0.0)) for k in range(n_views)]
    least = min(rows)
    n_common = least if least < 4 else (3 * least) // 4
    X = np.zeros((0, 3))
    while len(X) < n_common:                             # points in front of view 0 that every view holds well inside its image
        m = 2 * (n_common - len(X)) + 8
        px = np.column_stack([rng.uniform(30, W - 30, m), rng.uniform(30, H - 30, m)])
        d = rng.uniform(3.0, 40.0, m)
        cand = np.column_stack([(px[:, 0] - CAM[1]) / CAM[0] * d, (px[:, 1] - CAM[2]) / CAM[0] * d, d])
        keep = np.ones(m, dtype=bool)
        for k in range(n_views):
            p, z = _project(cams[k], Rts[k], cand)
            keep &= (z > 1.0) & (p[:, 0] > 20) & (p[:, 0] < W - 20) & (p[:, 1] > 20) & (p[:, 1] < H - 20)
        X = np.vstack([X, cand[keep]])[:n_common]
    base = rng.randint(0, 256, (n_common, 64)).astype(np.uint8)
    views, info = [], []
    for k in range(n_views):
        n = rows[k]
        p, _ = _project(cams[k], Rts[k], X)
        pos = p + rng.normal(0.0, noise, p.shape) if n_common else p
        desc = np.array([_flip(rng, r, rng.randint(0, 12)) for r in base], dtype=np.uint8).reshape(-1, 64)
        n_dup = min(n_common // 10, n - n_common) if (doubles and k == 0) else 0
        dup_of = rng.choice(n_common, n_dup, replace=False) if n_dup else np.zeros(0, dtype=np.int64)
        pos = np.vstack([pos, pos[dup_of] + np.array([0.25, 0.0])])
        desc = np.vstack([desc, np.array([_flip(rng, desc[i], rng.randint(0, 4)) for i in dup_of], dtype=np.uint8).reshape(-1, 64)])
        n_extra = n - n_common - n_dup
        pos = np.vstack([pos, np.column_stack([rng.uniform(20, W - 20, n_extra), rng.uniform(20, H - 20, n_extra)])])
        desc = np.vstack([desc, rng.randint(0, 256, (n_extra, 64)).astype(np.uint8)])
        track = np.full(n, -1, dtype=np.int32)
        step = TRACK_EVERY[k % len(TRACK_EVERY)]
        tracked = np.arange(0, n_common, step)
        if map_n > 0 and len(tracked):
            track[tracked] = rng.choice(map_n, len(tracked), replace=len(tracked) > map_n)
        order = rng.permutation(n)                         # new row r holds old row order[r]
        where = np.empty(n, dtype=np.int64)
        where[order] = np.arange(n)
        views.append(dict(desc=np.ascontiguousarray(desc[order]), feat=np.ascontiguousarray(pos[order].astype(np.float32)), cam=tuple(cams[k]),
                          Rt=Rts[k], track=np.ascontiguousarray(track[order]), count=None))
        info.append(dict(common=where[:n_common], doubles=where[n_common:n_common + n_dup], X=X))
    return views, info


def make_map(map_n, seed):
    """an old map: random descriptor rows and points"""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (map_n, 64)).astype(np.uint8), rng.uniform(-5.0, 5.0, (map_n, 3)) + np.array([0.0, 0.0, 20.0])


def main_case():
    """the committed main case: 300 common + 100 other rows a view, band 2, threshold 40, cap 64, a map of 40 rows"""
    views, info = make_views([400, 400], seed=7)
    return views, info, dict(band=BAND, threshold=THRESHOLD, max_distance=CAP, map_n=40)


def with_kps(view):
    """the same view with its positions as detector keypoints of level 0: pixel centres, so the positions move by up to half a pixel"""
    from coloc_amd import KP_DTYPE
    kps = np.zeros(len(view["feat"]), dtype=KP_DTYPE)
    kps["x"], kps["y"] = np.rint(view["feat"][:, 0]).astype(np.int32), np.rint(view["feat"][:, 1]).astype(np.int32)
    out = dict(view)
    out["kps"], out["feat"] = kps, None
    return out

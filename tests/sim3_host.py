"""ctypes access to the host build of the 3-D similarity (tests/host/sim3_host_lib.cpp over coloc_amd/csrc/sim3_math.h and clc_acr.h) and
to the sequential statement of clc_sim3_acransac it holds: the yardstick the device is compared with bit for bit.  Built on demand, like
tests/acr_host.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = []


def lib():
    if not _LIB:
        out = os.path.join(ROOT, "tests", "host", "libsim3_host.so")
        src = os.path.join(ROOT, "tests", "host", "sim3_host_lib.cpp")
        hdrs = [os.path.join(ROOT, "coloc_amd", "csrc", h) for h in ("sim3_math.h", "clc_acr.h", "map_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        L = C.CDLL(out)
        L.sim3_host_box_volume.restype = C.c_double
        L.sim3_host_logalpha0.restype = C.c_double
        L.sim3_host_logalpha0.argtypes = [C.c_double]
        _LIB.append(L)
    return _LIB[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pts(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)


def minimal(x3, y3):
    """three correspondences (3, 3) each -> A (12,), NaN-filled for a degenerate sample"""
    x3, y3 = _pts(x3), _pts(y3)
    A = np.zeros(12)
    lib().sim3_host_minimal(_p(x3), _p(y3), _p(A))
    return A


def minimal_of_samples(x, y, samples):
    x, y = _pts(x), _pts(y)
    return np.stack([minimal(x[list(s)], y[list(s)]) for s in np.asarray(samples).reshape(-1, 3)]) if len(samples) else np.zeros((0, 12))


def residuals(A, x, y):
    x, y = _pts(x), _pts(y)
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(12)
    out = np.zeros(len(x))
    lib().sim3_host_residuals(_p(A), _p(x), _p(y), C.c_int(len(x)), _p(out))
    return out


def from_model(A):
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(12)
    s, R, t = C.c_double(), np.zeros(9), np.zeros(3)
    lib().sim3_host_from_model(_p(A), C.byref(s), _p(R), _p(t))
    return s.value, R.reshape(3, 3), t


def refit(x, y, inliers=None):
    """Umeyama over the inliers in ascending index (None: all) -> (ok, s, R, t, A); refused: ok False, the rest None"""
    x, y = _pts(x), _pts(y)
    lst = np.arange(len(x), dtype=np.int32) if inliers is None else np.sort(np.asarray(inliers, dtype=np.int32))
    s, R, t, A = C.c_double(), np.zeros(9), np.zeros(3), np.zeros(12)
    ok = lib().sim3_host_refit(_p(x), _p(y), _p(lst), C.c_int(len(lst)), C.byref(s), _p(R), _p(t), _p(A))
    return (True, s.value, R.reshape(3, 3), t, A.reshape(3, 4)) if ok else (False, None, None, None, None)


def apply_points(A, X):
    X = _pts(X)
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(12)
    out = np.zeros_like(X)
    lib().sim3_host_apply_points(_p(A), _p(X), C.c_int(len(X)), _p(out))
    return out


def apply_pose(s, R, t, Rt):
    Rt = np.ascontiguousarray(Rt, dtype=np.float64).reshape(12).copy()
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    lib().sim3_host_apply_pose(C.c_double(s), _p(R), _p(t), _p(Rt))
    return Rt.reshape(3, 4)


def scale_points(s, X):
    X = _pts(X)
    out = np.zeros_like(X)
    lib().sim3_host_scale_points(C.c_double(s), _p(X), C.c_int(len(X)), _p(out))
    return out


def scale_pose(s, Rt):
    Rt = np.ascontiguousarray(Rt, dtype=np.float64).reshape(12).copy()
    lib().sim3_host_scale_pose(C.c_double(s), _p(Rt))
    return Rt.reshape(3, 4)


def box_volume(y):
    y = _pts(y)
    return float(lib().sim3_host_box_volume(_p(y), C.c_int(len(y))))


def acransac(x_new, x_old, max_iteration=256, seed=1, precision=float("inf")):
    """The sequential statement of clc_sim3_acransac: the dict Context.sim3_acransac returns."""
    x, y = _pts(x_new), _pts(x_old)
    n = len(x)
    assert len(y) == n
    R, t, A = np.zeros(9), np.zeros(3), np.zeros(12)
    mask, inl = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.int32)
    s, emax, nfa = C.c_double(), C.c_double(), C.c_double()
    ni, its, valid, rf = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    lib().sim3_host_acransac(_p(x), _p(y), C.c_int(n), C.c_int(int(max_iteration)), C.c_uint64(int(seed)), C.c_double(float(precision)),
                             C.byref(s), _p(R), _p(t), _p(A), _p(mask), _p(inl), C.byref(ni), C.byref(emax), C.byref(nfa), C.byref(its),
                             C.byref(valid), C.byref(rf))
    return dict(found=valid.value >= 0, s=s.value, R=R.reshape(3, 3), t=t, A=A.reshape(3, 4), mask=mask[:n].astype(bool),
                inliers=inl[:ni.value].copy(), n_inliers=ni.value, error_max=emax.value, min_nfa=nfa.value, iterations=its.value,
                valid=valid.value, refit=rf.value)


APPLY_SCALE, APPLY_FULL = 0, 1
SIM_OK, SIM_NO_MODEL = 0, 1


def transform_points(res, X, apply):
    """the new map's points under a solve's result: unchanged without a model, X * s (APPLY_SCALE) or s R X + t (APPLY_FULL)"""
    X = _pts(X)
    if not res["found"]:
        return X.copy()
    return apply_points(res["A"], X) if apply == APPLY_FULL else scale_points(res["s"], X)


def transform_pose(res, Rt, apply):
    if not res["found"]:
        return np.ascontiguousarray(Rt, dtype=np.float64).reshape(3, 4).copy()
    return apply_pose(res["s"], res["R"], res["t"], Rt) if apply == APPLY_FULL else scale_pose(res["s"], Rt)


def map_align_sim(old_X, new_X, match, apply=APPLY_SCALE, max_iteration=256, seed=1, precision=float("inf")):
    """The whole step of clc_map_align_sim_dev as a host statement: the common list of a match array in ascending old row (an index outside
    the new map is no match), the sequential statement of the solve on X_new | X_old of the common features, the transform of every new
    point.  -> the solve's dict + match (cleaned), cq, ct, n_common, inlier (flags per common feature), status, X."""
    old_X, new_X = _pts(old_X), _pts(new_X)
    match = np.asarray(match, dtype=np.int64)
    cq = np.nonzero((match >= 0) & (match < len(new_X)))[0]
    ct = match[cq]
    res = acransac(new_X[ct], old_X[cq], max_iteration, seed, precision)
    res.update(match=np.where((match >= 0) & (match < len(new_X)), match, -1).astype(np.int32), cq=cq.astype(np.int32), ct=ct.astype(np.int32),
               n_common=len(cq), inlier=res["mask"], status=SIM_OK if res["found"] else SIM_NO_MODEL, X=transform_points(res, new_X, apply))
    return res

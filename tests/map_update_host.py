"""The map update's tail as a host statement, the yardstick of coloc_amd/csrc/map_update.hip (include/coloc_hip.h: clc_map_align_dev,
clc_map_update_batch_dev): the common list from a match array in plain numpy -- ascending old row, an index outside the new map is no
match -- and the fp64 / fp32 arithmetic of the scale rule, the rescale and rescale_pose from the host build of inter_math.h + map_math.h
(tests/host/map_update_lib.cpp), which the device is compared with bit for bit and which tests/test_map_update_host.py holds to an
independent Python restatement.  Shares no code with the kernel."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NO_SCALE = 0, 1
_LIB = []


def lib():
    if not _LIB:
        out = os.path.join(ROOT, "tests", "host", "libmap_update_host.so")
        src = os.path.join(ROOT, "tests", "host", "map_update_lib.cpp")
        hdrs = [os.path.join(ROOT, "coloc_amd", "csrc", h) for h in ("map_math.h", "inter_math.h")] + [os.path.join(ROOT, "include", "coloc_hip.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        _LIB.append(C.CDLL(out))
    return _LIB[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def common_list(match, n_new):
    """match[q] = new row of old row q or -1 -> (cq, ct) int32, ascending old row; an index outside [0, n_new) is no match"""
    match = np.asarray(match, dtype=np.int64)
    cq = np.nonzero((match >= 0) & (match < n_new))[0]
    return cq.astype(np.int32), match[cq].astype(np.int32)


def clean_match(match, n_new):
    """the match array as the call reports it: -1 where the index names no new row"""
    match = np.asarray(match, dtype=np.int32)
    return np.where((match >= 0) & (match < n_new), match, -1).astype(np.int32)


def scale_of(old_X, new_X, cq, ct):
    """-> (scale, n_terms, status) of a common list"""
    old_X = np.ascontiguousarray(old_X, dtype=np.float64).reshape(-1, 3)
    new_X = np.ascontiguousarray(new_X, dtype=np.float64).reshape(-1, 3)
    cq, ct = np.ascontiguousarray(cq, dtype=np.int32), np.ascontiguousarray(ct, dtype=np.int32)
    assert len(cq) == len(ct) and (len(cq) == 0 or (cq.max() < len(old_X) and ct.max() < len(new_X) and cq.min() >= 0 and ct.min() >= 0))
    scale, n_terms = C.c_double(0.0), C.c_int(0)
    f = lib().map_update_host_scale
    f.restype = C.c_int
    status = f(_p(old_X), _p(new_X), _p(cq), _p(ct), C.c_int(len(cq)), C.byref(scale), C.byref(n_terms))
    return scale.value, n_terms.value, status


def rescale_points(X, scale):
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    out = np.zeros_like(X)
    lib().map_update_host_rescale_points(_p(X), C.c_int(len(X)), C.c_double(scale), _p(out))
    return out


def rescale_pose(Rt, scale):
    Rt = np.ascontiguousarray(Rt, dtype=np.float64).reshape(12).copy()
    lib().map_update_host_rescale_pose(_p(Rt), C.c_double(scale))
    return Rt.reshape(3, 4)


def align(old_X, new_X, match):
    """the whole step: -> dict(match, cq, ct, n_common, n_terms, scale, status, X)"""
    new_X = np.ascontiguousarray(new_X, dtype=np.float64).reshape(-1, 3)
    cq, ct = common_list(match, len(new_X))
    scale, n_terms, status = scale_of(old_X, new_X, cq, ct)
    return dict(match=clean_match(match, len(new_X)), cq=cq, ct=ct, n_common=len(cq), n_terms=n_terms, scale=scale, status=status,
                X=rescale_points(new_X, scale))

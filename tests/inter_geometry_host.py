"""ctypes access to the host build of the inter-camera geometry (tests/host/inter_geometry_lib.cpp over coloc_amd/csrc/inter_geometry.cpp
and inter_math.h).  root: the checkout to build from (tools/make_inter_geometry_golden.py points it at the parent commit's)."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIBS = {}


def lib(root=ROOT):
    if root not in _LIBS:
        out = os.path.join(root, "tests", "host", "libinter_geometry_host.so")
        srcs = [os.path.join(root, "tests", "host", "inter_geometry_lib.cpp"), os.path.join(root, "coloc_amd", "csrc", "inter_geometry.cpp")]
        deps = srcs + [os.path.join(root, "coloc_amd", "csrc", h) for h in ("inter_math.h", "inter_geometry.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps if os.path.exists(d)):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(root, "include")] + srcs + ["-o", out])
        _LIBS[root] = C.CDLL(out)
    return _LIBS[root]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def relative(x1, x2, K, E, inliers, root=ROOT):
    """inter_relative: dict(stage, n_front, corr, Xt, x2f, R, t); the arrays hold n_front points (none unless stage == 0)"""
    ni = len(inliers)
    Xt, x2f, corr, R, t = np.zeros(3 * ni), np.zeros(2 * ni), np.zeros(ni, np.int32), np.zeros(9), np.zeros(3)
    nf = C.c_int(0)
    stage = lib(root).inter_geometry_host_relative(_p(x1), _p(x2), C.c_int(len(x1)), _p(K), _p(K), _p(E), _p(inliers), C.c_int(ni), _p(Xt), _p(x2f),
                                                   _p(corr), _p(R), _p(t), C.byref(nf))
    m = nf.value if stage == 0 else 0
    return dict(stage=stage, n_front=nf.value, corr=corr[:m].copy(), Xt=Xt[:3 * m].copy(), x2f=x2f[:2 * m].copy(), R=R, t=t)


def scale_pose(front, common, map_X, Rt_source, root=ROOT):
    """inter_scale_pose: dict(stage, n_common, scale, Rt, Xw)"""
    nf = len(front["corr"])
    common, map_X, Rt_source = np.ascontiguousarray(common, np.int32), np.ascontiguousarray(map_X), np.ascontiguousarray(Rt_source)
    Rt, Xw = np.zeros(12), np.zeros(3 * nf)
    nc, scale = C.c_int(0), C.c_double(0.0)
    stage = lib(root).inter_geometry_host_scale_pose(_p(front["Xt"]), C.c_int(nf), _p(front["R"]), _p(front["t"]), _p(common), C.c_int(len(common)),
                                                     _p(map_X), C.c_int(len(map_X)), _p(Rt_source), C.byref(nc), C.byref(scale), _p(Rt), _p(Xw))
    return dict(stage=stage, n_common=nc.value, scale=np.float64(scale.value), Rt=Rt, Xw=Xw)


def run_cases(root=ROOT):
    """every case of tests/inter_scenes.py through the library built from `root`: a flat dict of arrays, the fixture's layout"""
    import inter_scenes as S
    out, fronts = {}, {}
    for name in S.FRONT_CASES:
        i = S.front_inputs(name)
        f = relative(i["x1"], i["x2"], i["K"], i["E"], i["inliers"], root)
        fronts[name] = (i, f)
        out["front/%s/inliers" % name] = i["inliers"]
        for k in ("stage", "n_front", "corr", "Xt", "x2f", "R", "t"):
            out["front/%s/%s" % (name, k)] = np.asarray(f[k])
    for name, (fname, form, _) in S.SCALE_CASES.items():
        i, f = fronts[fname]
        p = i["pair"]
        com = S.common_pairs(form, f["corr"], p["map_index"], len(p["map_X"]))
        s = scale_pose(f, com, p["map_X"], p["Rt_source"], root)
        out["scale/%s/common" % name] = com
        for k in ("stage", "n_common", "scale", "Rt", "Xw"):
            out["scale/%s/%s" % (name, k)] = np.asarray(s[k])
    return out


def fixture_form(out):
    """the fixture's layout: every array of more than 200 entries as the SHA-256 of its type, shape and bytes -- 32 bytes that hold it bit
    for bit --, the smaller ones (all of the n = 60 cases, every R, t, Rt and scale) in full, where a difference can be located"""
    def sha(a):
        a = np.ascontiguousarray(a)
        return np.frombuffer(hashlib.sha256(("%s %s " % (a.dtype.str, a.shape)).encode() + a.tobytes()).digest(), np.uint8)
    return {k: sha(v) if np.size(v) > 200 else np.asarray(v) for k, v in out.items()}

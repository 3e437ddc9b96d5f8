"""The map grown past the seed pair as a plain Python / numpy statement, the yardstick of coloc_amd/csrc/map_grow.hip (include/coloc_hip.h:
clc_map_build_grow_dev): per-track landmarks and observation masks in dicts, the resection order, the resection lists, the grow of every
resected camera's tracks and the grown map's rows.  Shares no code with the kernels.  It stands on tests/map_host.py for the tracks and the
seed; the fp64 arithmetic of ONE point is not restated: it is the g++ build of coloc_amd/csrc/map_math.h (tests/host/map_grow_lib.cpp).  The
poses of the resected cameras are an INPUT (a callable): the a-contrario solve has its own references."""
import ctypes as C
import os
import subprocess

import numpy as np

import map_host
import track_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = []
GROW_OK, GROW_NO_TRACKS, GROW_NO_POSE, GROW_CAPACITY = 0, 1, 2, 3
MAX_CORR = 16384


def lib():
    if not _LIB:
        out = os.path.join(ROOT, "tests", "host", "libmap_grow_host.so")
        src = os.path.join(ROOT, "tests", "host", "map_grow_lib.cpp")
        hdr = os.path.join(ROOT, "coloc_amd", "csrc", "map_math.h")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        L = C.CDLL(out)
        L.map_grow_host_cos_2deg.restype = C.c_double
        _LIB.append(L)
    return _LIB[0]


_p, _f64 = map_host._p, map_host._f64


def ray(cam, Rt, x_ud):
    r = np.zeros(3)
    lib().map_grow_host_ray(_p(_f64(cam[:3], 3)), _p(_f64(Rt, 12)), _p(_f64(x_ud, 2)), _p(r))
    return r


def angle_over_2deg(r_i, r_j):
    r_i, r_j = _f64(r_i, (-1, 3)), _f64(r_j, (-1, 3))
    over = np.zeros(len(r_i), dtype=np.uint8)
    lib().map_grow_host_angle(_p(r_i), _p(r_j), C.c_int(len(r_i)), _p(over))
    return over.astype(bool)


def grow_point(cam_i, cam_j, Rt_i, Rt_j, x_i, x_j):
    """-> (accepted, X)"""
    X = np.zeros(3)
    ok = lib().map_grow_host_point(_p(_f64(cam_i[:3], 3)), _p(_f64(cam_j[:3], 3)), _p(_f64(Rt_i, 12)), _p(_f64(Rt_j, 12)), _p(_f64(x_i, 2)),
                                   _p(_f64(x_j, 2)), _p(X))
    return bool(ok), X


def observation_ok(Rt, X):
    return bool(lib().map_grow_host_observation_ok(_p(_f64(Rt, 12)), _p(_f64(X, 3))))


def resect_list(table, X, obs, ud, I):
    """camera I's resection list on a state: the tracks that hold I and have a landmark, in ascending id"""
    ts = [t for t in range(len(table)) if table[t, I] >= 0 and obs.get(t, 0)]
    rows = table[ts, I].astype(np.int32) if ts else np.zeros(0, dtype=np.int32)
    return dict(track=np.array(ts, dtype=np.int32), row=rows, X=np.array([X[t] for t in ts]).reshape(-1, 3), x=ud[I][rows].reshape(-1, 2))


def grow_map(rows, pairs, cams, seed_pair, Rt_a, Rt_b, pose_of):
    """pose_of(camera, its resection list) -> [R|t] (3 x 4), or None where the resection failed.  -> dict: the seed build's entries, the
    per-track state (X, obs: dicts by track id), lists[camera] (at the camera's turn), status[camera], order (the resection order), poses,
    and the grown map: map_track, map_cam, map_row, map_obs, map_X, n_seed_rows, n_added."""
    base = map_host.build_map(rows, pairs, cams, seed_pair, Rt_a, Rt_b)
    table = base["track_feat"]
    n_cams = len(rows)
    a, b = int(pairs[seed_pair]["cam_a"]), int(pairs[seed_pair]["cam_b"])
    ud = [track_host.get_ud_pixel(map_host.positions(c).astype(np.float64), c["cam"]) for c in cams]
    X, obs = {}, {}
    for t, x in zip(base["map_track"].tolist(), base["X"]):
        X[t], obs[t] = x.copy(), (1 << a) | (1 << b)
    valid = {a: np.asarray(Rt_a, dtype=np.float64).reshape(3, 4), b: np.asarray(Rt_b, dtype=np.float64).reshape(3, 4)}
    status, lists, order = {a: GROW_OK, b: GROW_OK}, {}, [c for c in range(n_cams) if c not in (a, b)]
    for I in order:
        lst = resect_list(table, X, obs, ud, I)
        lists[I] = lst
        if len(lst["track"]) == 0:
            status[I] = GROW_NO_TRACKS
            continue
        if len(lst["track"]) > MAX_CORR:
            status[I] = GROW_CAPACITY
            continue
        Rt = pose_of(I, lst)
        if Rt is None:
            status[I] = GROW_NO_POSE
            continue
        status[I] = GROW_OK
        valid[I] = np.asarray(Rt, dtype=np.float64).reshape(3, 4)
        for t in np.nonzero(table[:, I] >= 0)[0].tolist():
            if obs.get(t, 0):
                cand, Xt = [I], X[t]
            else:
                cand, Xt = [], None
                for J in sorted(valid):
                    if J == I or table[t, J] < 0:
                        continue
                    if Xt is None:
                        ok, Xn = grow_point(cams[I]["cam"], cams[J]["cam"], valid[I], valid[J], ud[I][table[t, I]], ud[J][table[t, J]])
                        if ok:
                            Xt = Xn
                            cand.append(I)
                    cand.append(J)
                if Xt is None:
                    continue
            mask = obs.get(t, 0)
            for J in cand:
                if observation_ok(valid[J], Xt):
                    mask |= 1 << J
            if mask:
                X[t], obs[t] = Xt, mask
    ts = sorted(t for t in obs if obs[t])
    cam = [(obs[t] & -obs[t]).bit_length() - 1 for t in ts]
    out = dict(base)
    out.update(state_X=X, state_obs=obs, ud=ud, lists=lists, status=[status[c] for c in range(n_cams)], order=order, poses=valid,
               map_track=np.array(ts, dtype=np.int32), map_cam=np.array(cam, dtype=np.int32),
               map_row=np.array([table[t, c] for t, c in zip(ts, cam)], dtype=np.int32), map_obs=np.array([obs[t] for t in ts], dtype=np.uint8),
               map_X=np.array([X[t] for t in ts]).reshape(-1, 3), n_seed_rows=len(base["map_track"]), n_added=len(ts) - len(base["map_track"]))
    return out

"""The map's bundle adjustment on the host: the scenes the tests share, and the Levenberg-Marquardt loop of coloc_amd/csrc/map_ba.hip in
numpy over the g++ build of coloc_amd/csrc/ba_math.h (tests/host/ba_lib.cpp) -- the per-point and per-entry arithmetic is not restated,
the loop (pnp_refine_kernel's damping schedule and stopping rules) is.

  scene(name)       'A' 3 cameras x 12 points, 'B' 3 x 70, 'C' 8 x 300 (one camera outside cam_mask), fixed seeds: points in
                    [-5, 5]^2 x [4, 20], cameras on a small arc, f = 1000, pp (640, 360), 0.5 px noise, single-observation points,
                    observations displaced by about 39 px (the Huber tail), a start perturbed by 0.01 rad / 0.05 / 0.1
  solve(...)        the loop; what clc_ba_dev reports, from the host statement
  mp_problem / mp_params      the same problem and an iterate for the 50-digit reference (tests/ba_mp.py)
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
BA_OK, BA_MAX_ITERATIONS, BA_STALLED, BA_BAD_START, BA_EMPTY = 0, 1, 2, 3, 4


def lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "tests", "host", "libba_host.so")
        src = os.path.join(ROOT, "tests", "host", "ba_lib.cpp")
        hdrs = [os.path.join(ROOT, "coloc_amd", "csrc", h) for h in ("ba_math.h", "so3.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        _LIB = C.CDLL(out)
        _LIB.ba_host_cost.restype = C.c_double
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
SCENES = {          # seed, cameras, points, missing share, single-observation points, tail observations, camera outside the mask
    "A": (27, 3, 12, 0.0, 1, 1, None),
    "B": (30, 3, 70, 0.3, 2, 3, None),
    "C": (37, 8, 300, 0.4, 3, 5, 5),
}


def _rot_y(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def _exp(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + math.sin(th) / th * W + (1 - math.cos(th)) / th ** 2 * W @ W


def project(K, Rt, X):
    Xc = Rt[:, :3] @ X + Rt[:, 3]
    return np.array([K[0] * Xc[0] / Xc[2] + K[1], K[0] * Xc[1] / Xc[2] + K[2]])


def scene(name, noise=0.5, perturb=True):
    """dict: K (n, 3), mask, obs (uint32), x (points, n, 2), Rt_true / Rt0 (n, 3, 4), X_true / X0, tails [(t, c)], singles [t]"""
    seed, n_cams, n_pts, missing, n_single, n_tail, out_cam = SCENES[name]
    rng = np.random.RandomState(seed)
    X = np.column_stack([rng.uniform(-5, 5, n_pts), rng.uniform(-5, 5, n_pts), rng.uniform(4, 20, n_pts)])
    K = np.tile(np.array([1000.0, 640.0, 360.0]), (n_cams, 1))
    Rt = np.zeros((n_cams, 3, 4))
    for c in range(n_cams):
        th = (c - 0.5 * (n_cams - 1)) * 0.15
        R = _rot_y(-0.5 * th) @ _exp(0.02 * rng.standard_normal(3))
        Cc = np.array([4.0 * math.sin(th), 0.1 * rng.standard_normal(), 4.0 * (1 - math.cos(th))])
        Rt[c, :, :3] = R
        Rt[c, :, 3] = -R @ Cc
    mask = ((1 << n_cams) - 1) & ~(0 if out_cam is None else 1 << out_cam)
    masked = [c for c in range(n_cams) if (mask >> c) & 1]
    see = rng.uniform(size=(n_pts, n_cams)) >= missing
    singles = list(range(1, 1 + 2 * n_single, 2))
    for t in range(n_pts):
        if t in singles:
            see[t, :] = False
            see[t, masked[t % len(masked)]] = True
        else:
            while sum(see[t, c] for c in masked) < 2:
                see[t, masked[rng.randint(len(masked))]] = True
    if out_cam is not None:                     # two points that only the camera outside the mask sees
        for t in (n_pts - 1, n_pts - 4):
            see[t, :] = False
            see[t, out_cam] = True
    x = np.zeros((n_pts, n_cams, 2))
    for t in range(n_pts):
        for c in range(n_cams):
            x[t, c] = project(K[c], Rt[c], X[t]) + noise * rng.standard_normal(2)
    tails = []
    for t in range(n_pts):
        if len(tails) < n_tail and t % 5 == 0 and sum(see[t, c] for c in masked) >= 3:
            c = [c for c in masked if see[t, c]][len(tails) % 3]
            x[t, c] += np.array([28.0, -27.0]) if noise > 0 else 0.0
            tails.append((t, c))
    assert len(tails) == n_tail, "scene %s: too few points with three observations" % name
    obs = np.array([sum(1 << c for c in range(n_cams) if see[t, c]) for t in range(n_pts)], dtype=np.uint32)
    Rt0, X0 = Rt.copy(), X.copy()
    if perturb:
        for c in range(n_cams):
            Rt0[c, :, :3] = Rt[c, :, :3] @ _exp(0.01 * rng.standard_normal(3))
            Rt0[c, :, 3] = Rt[c, :, 3] + 0.05 * rng.standard_normal(3)
        X0 = X + 0.1 * rng.standard_normal(X.shape)
    return dict(name=name, K=K, mask=mask, obs=obs, x=x, Rt_true=Rt, X_true=X, Rt0=Rt0, X0=X0, tails=tails, singles=singles, out_cam=out_cam)


# ---- the host statement ---------------------------------------------------------------------------------------------------------------
class Cams:
    def __init__(self, K, mask, par):
        self.buf = np.zeros(lib().ba_host_sizeof_cams() // 8 + 1)
        self.K = np.ascontiguousarray(K, dtype=np.float64)
        self.mask = int(mask)
        self.set(par)

    def set(self, par):
        self.par = np.ascontiguousarray(par, dtype=np.float64)
        lib().ba_host_cams_set(_p(self.buf), C.c_int(len(self.K)), C.c_uint32(self.mask), _p(self.K), _p(self.par))

    def Rt(self, c):
        out = np.zeros(12)
        lib().ba_host_to_Rt(_p(self.buf), C.c_int(c), _p(out))
        return out.reshape(3, 4)


def params_from_Rt(Rt):
    par = np.zeros((len(Rt), 6))
    for c in range(len(Rt)):
        row = np.zeros(6)
        lib().ba_host_from_Rt(_p(np.ascontiguousarray(Rt[c], dtype=np.float64).reshape(12)), _p(row))
        par[c] = row
    return par


def cost(cams, X, obs, x, a):
    no, npt = C.c_int(0), C.c_int(0)
    v = lib().ba_host_cost(_p(cams.buf), C.c_int(len(obs)), _p(X), _p(obs), _p(x), C.c_double(a), C.byref(no), C.byref(npt))
    return v, no.value, npt.value


def solve(K, mask, obs, x, Rt0, X0, max_iterations=0, huber_a=0.0, function_tolerance=1e-8):
    """The loop of map_ba.hip.  -> dict(status, iterations, cost_initial, cost_final, rmse, n_obs, n_points, n_cams, Rt, X, lambda_)"""
    a = huber_a if huber_a > 0 else 16.0
    max_it = max_iterations if max_iterations > 0 else 500
    obs = np.ascontiguousarray(obs, dtype=np.uint32)
    x = np.ascontiguousarray(x, dtype=np.float64)
    X = np.ascontiguousarray(X0, dtype=np.float64).copy()
    Rt = np.array(Rt0, dtype=np.float64).copy()
    n = len(K)
    cams = Cams(K, mask, params_from_Rt(Rt))
    c0, n_obs, n_pts = cost(cams, X, obs, x, a)
    res = dict(iterations=0, cost_initial=c0, cost_final=c0, n_obs=n_obs, n_points=n_pts, n_cams=bin(mask & ((1 << n) - 1)).count("1"), Rt=Rt, X=X,
               rmse=0.0, lambda_=1e-4)
    if n_obs == 0:
        res.update(status=BA_EMPTY, cost_initial=0.0, cost_final=0.0)
        return res
    if not math.isfinite(c0):
        res.update(status=BA_BAD_START)
        return res
    lam, cur, it, status, accepted = 1e-4, c0, 0, None, 0
    slots = [c for c in range(n) if (mask >> c) & 1]
    while status is None:
        if not it < max_it:
            status = BA_MAX_ITERATIONS
            break
        dc, dX = np.zeros(48), np.zeros_like(X)
        gmax, dn, pn = C.c_double(0), C.c_double(0), C.c_double(0)
        ok = lib().ba_host_step(_p(cams.buf), C.c_int(len(obs)), _p(X), _p(obs), _p(x), C.c_double(a), C.c_double(lam), _p(dc), _p(dX),
                                C.byref(gmax), C.byref(dn), C.byref(pn))
        if gmax.value < 1e-8 * max(1.0, cur):
            status = BA_OK
            break
        if not ok:
            lam *= 10.0
            if lam > 1e10:
                status = BA_STALLED
            else:
                it += 1
            continue
        if math.sqrt(dn.value) < 1e-8 * (math.sqrt(pn.value) + 1e-8):
            status = BA_OK
            break
        par_try = cams.par.copy()
        for s, c in enumerate(slots):
            par_try[c] = cams.par[c] + dc[6 * s:6 * s + 6]
        X_try = X + dX
        trial = Cams(K, mask, par_try)
        new, _, _ = cost(trial, X_try, obs, x, a)
        if new < cur:
            rel = (cur - new) / max(cur, 1e-300)
            cams, X, cur = trial, X_try, new
            lam = max(lam * 0.1, 1e-12)
            it += 1
            accepted += 1
            if rel < function_tolerance:
                status = BA_OK
        else:
            lam *= 10.0
            if lam > 1e10:
                status = BA_STALLED
            else:
                it += 1
    if accepted:
        for c in slots:
            Rt[c] = cams.Rt(c)
    res.update(status=status, iterations=it, cost_final=cur, rmse=math.sqrt(cur / (2.0 * n_obs)), Rt=Rt, X=X, lambda_=lam)
    return res


def solve_scene(s, **kw):
    return solve(s["K"], s["mask"], s["obs"], s["x"], s["Rt0"], s["X0"], **kw)


# ---- the 50-digit side ----------------------------------------------------------------------------------------------------------------
def mp_problem(s, huber_a=16.0):
    return dict(K=s["K"].tolist(), mask=int(s["mask"]), obs=[int(v) for v in s["obs"]], x=s["x"].tolist(), a=huber_a)


def mp_params(prob, Rt, X):
    """float64 [R|t] and points -> the reference's parameter vector (the rotation's logarithm at 50 digits)"""
    import ba_mp
    import pose_mp as pm
    pars = {}
    for c in ba_mp.cams_of(prob):
        R = np.asarray(Rt[c])[:, :3]
        pars[c] = list(pm.log_so3(R.tolist())) + pm.vec(np.asarray(Rt[c])[:, 3].tolist())
    return ba_mp.pack(prob, pars, {t: np.asarray(X[t]).tolist() for t in ba_mp.points_of(prob)})

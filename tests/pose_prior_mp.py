"""50-digit reference of the pose-from-the-prediction rule (include/coloc_hip.h, THE RULE of clc_track_prior_dev), on top of
tests/pose_mp.py (imported, not edited): each round's minimiser is pose_mp.newton_polish over the round's mask, started at the round's
p_k, and classify runs at 50 digits.

  track_state(p, ...)   (zc, sq) of every track at p, as mpf
  classify(state, g2)   in iff zc > 0 and sq <= g2
  solve(...)            the rounds: masks m_0 .. (m_0 = zc > 0 under the prior, m_{k+1} = classify(p_{k+1})), the (zc, sq) every
                        classification looked at -- for the input condition of tests/test_pose_prior_reference.py --, rounds_run,
                        converged, result, the final parameters, mask and minimum cost
A pass over 600 points takes about half a second, so solve() is cached per case by its caller (tests/pose_prior_cases.py).
"""
import numpy as np
from mpmath import mp, mpf

import pose_mp as pm

OK, FEW = 0, 1


def track_state(p, X, x, K):
    p = pm.vec(p)
    Km = pm.mat3(K)
    R = pm.exp_so3(p[:3])
    out = []
    for Xi, xi in zip(X, x):
        Xi, xi = pm.vec(Xi), pm.vec(xi)
        zc = pm.cam_point(R, p[3:], Xi)[2]
        out.append((zc, pm.sq_err(Km, R, p[3:], Xi, xi) if zc != 0 else mpf("inf")))
    return out


def classify(state, g2):
    return np.array([bool(zc > 0 and sq <= g2) for zc, sq in state], dtype=bool)


def solve(X, x, K, Rt_prior, gate, huber_a=16.0, rounds=0, min_inliers=0):
    Rt_prior = np.asarray(Rt_prior, dtype=np.float64).reshape(3, 4)
    a = huber_a if huber_a > 0 else 16.0
    rounds = rounds or 4
    need = max(min_inliers if min_inliers > 0 else 8, 4)
    g2 = mpf(gate) * mpf(gate)
    p = pm.log_so3(Rt_prior[:, :3]) + pm.vec(Rt_prior[:, 3])
    st = track_state(p, X, x, K)
    m = np.array([bool(zc > 0) for zc, _ in st], dtype=bool)
    masks, states, rounds_run, converged = [m.copy()], [st], 0, 0      # states[k]: what produced masks[k]
    for _ in range(rounds):
        if m.sum() < 4:
            break
        p, _ = pm.newton_polish(p, X, x, K, a, mask=m)
        rounds_run += 1
        st = track_state(p, X, x, K)
        m_next = classify(st, g2)
        masks.append(m_next.copy())
        states.append(st)
        same = np.array_equal(m_next, m)
        m = m_next
        if same:
            converged = 1
            break
    mask = classify(st, g2)                                             # of the last p, over ALL tracks
    n_in = int(mask.sum())
    return dict(p=p, mask=mask, masks=masks, states=states, n_inliers=n_in, rounds_run=rounds_run, converged=converged,
                result=OK if n_in >= need else FEW, g2=g2, huber_a=a)


def band_violations(ref, lo=mpf("0.95"), hi=mpf("1.05"), z_min=mpf(10) ** -6):
    """The tracks that lie in the band at some reference round: (round, track, sq / g2, zc).  Round 0's classification has no residual
    gate, so only |zc| counts there."""
    bad = []
    g2 = ref["g2"]
    for k, st in enumerate(ref["states"]):
        for i, (zc, sq) in enumerate(st):
            if abs(zc) < z_min or (k > 0 and lo * g2 <= sq <= hi * g2):
                bad.append((k, i, float(sq / g2), float(zc)))
    if ref["rounds_run"] == 0:                                          # the final mask is classify(prior): gated
        for i, (zc, sq) in enumerate(ref["states"][0]):
            if lo * g2 <= sq <= hi * g2:
                bad.append((0, i, float(sq / g2), float(zc)))
    return bad

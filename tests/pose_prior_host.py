"""The pose-from-the-prediction rule (include/coloc_hip.h, THE RULE of clc_track_prior_dev) in plain float64 numpy: the statement the
50-digit reference tests/pose_prior_mp.py is compared with on the CPU (tests/test_pose_prior_reference.py).  It shares no code with
coloc_amd/csrc/pose_prior.hip: rotations and their derivatives are the yardsticks of tests/test_so3_host.py, the 6 x 6 solve is a Cholesky
written out here.  The device states the Levenberg-Marquardt rules restated below once, in coloc_amd/csrc/pose_lm.h (lm_judge,
lm_next_step and what counts as an iteration), for clc_pnp_refine and clc_pnp_refine_prior alike; this file stays an independent model.

  sums(p, ..., used)      zc, sq of EVERY track at p; A = sum w J^T J, g = sum w J^T r, cost = 1/2 sum rho over the tracks of `used`
  classify(zc, sq, g2)    in iff zc > 0 and sq <= g2 (NaN: out)
  levenberg(p, ..., used) the Levenberg-Marquardt of clc_pnp_refine from p over `used`: lambda from 1e-4, x 0.1 (floor 1e-12) on an
                          accepted step, x 10 on a rejected one or a failed solve, stop above 1e10, function / gradient / parameter
                          tests at 1e-8, at most max_iter steps
  solve(...)              the rounds
"""
import numpy as np

from test_so3_host import np_exp, np_log, np_dexp

OK, FEW = 0, 1


def sums(p, X, x, K, a, used):
    w, t = p[:3], p[3:]
    R, dR = np_exp(w), np_dexp(w)
    Xc = X @ R.T + t
    with np.errstate(divide="ignore", invalid="ignore"):
        iz = 1.0 / Xc[:, 2]
        xn, yn = Xc[:, 0] * iz, Xc[:, 1] * iz
        r = np.stack([x[:, 0] - (K[0, 0] * xn + K[0, 1] * yn + K[0, 2]), x[:, 1] - (K[1, 1] * yn + K[1, 2])], 1)
        sq = (r ** 2).sum(1)
    zc = Xc[:, 2]
    u = np.flatnonzero(used)
    if len(u) == 0:
        return zc, sq, np.zeros((6, 6)), np.zeros(6), 0.0
    Xu, ru, squ, izu, xnu, ynu = X[u], r[u], sq[u], iz[u], xn[u], yn[u]
    tail = squ > a * a
    root = np.sqrt(np.where(tail, squ, 1.0))
    rho = np.where(tail, 2.0 * a * root - a * a, squ)
    wgt = np.where(tail, a / root, 1.0)
    P = np.zeros((len(u), 2, 3))
    P[:, 0, 0] = K[0, 0] * izu; P[:, 0, 1] = K[0, 1] * izu; P[:, 0, 2] = -(K[0, 0] * xnu + K[0, 1] * ynu) * izu
    P[:, 1, 1] = K[1, 1] * izu; P[:, 1, 2] = -K[1, 1] * ynu * izu
    D = np.concatenate([np.einsum("kij,nj->nik", dR, Xu), np.broadcast_to(np.eye(3), (len(u), 3, 3))], 2)
    J = np.einsum("nab,nbk->nak", P, D)
    A = np.einsum("n,nai,naj->ij", wgt, J, J)
    g = np.einsum("n,nai,na->i", wgt, J, ru)
    return zc, sq, A, g, 0.5 * rho.sum()


def classify(zc, sq, g2):
    with np.errstate(invalid="ignore"):
        return (zc > 0.0) & (sq <= g2)


def solve6(A, g, lam):
    """(A + lam diag(max(A_ii, 1e-12))) d = g by Cholesky; None where a pivot is not above 64 ulp of its diagonal entry."""
    M = A.copy()
    for i in range(6):
        M[i, i] = A[i, i] + lam * max(A[i, i], 1e-12)
    L = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            s = M[i, j] - L[i, :j] @ L[j, :j]
            if i == j:
                if not (s > 0.0 and s > 64 * 2.0 ** -53 * M[i, i]):
                    return None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y = np.linalg.solve(L, g)
    return np.linalg.solve(L.T, y)


def levenberg(p, X, x, K, a, used, max_iter):
    """Returns (p, iterations, zc, sq, A, g, cost) with the sums at the returned p."""
    zc, sq, A, g, cost = sums(p, X, x, K, a, used)
    lam, it = 1e-4, 0
    while it < max_iter:
        d = solve6(A, g, lam)
        if d is None:
            lam *= 10.0
            if lam > 1e10:
                break
            it += 1
            continue
        if np.abs(g).max() < 1e-8 * max(1.0, cost) or np.linalg.norm(d) < 1e-8 * (np.linalg.norm(p) + 1e-8):
            break
        q = p + d
        zc_q, sq_q, A_q, g_q, cost_q = sums(q, X, x, K, a, used)
        if cost_q < cost:
            rel = (cost - cost_q) / max(cost, 1e-300)
            p, zc, sq, A, g, cost = q, zc_q, sq_q, A_q, g_q, cost_q
            lam = max(lam * 0.1, 1e-12)
            it += 1
            if rel < 1e-8:
                break
        else:
            lam *= 10.0
            if lam > 1e10:
                break
            it += 1
    return p, it, zc, sq, A, g, cost


def solve(X, x, K, Rt_prior, gate, huber_a=16.0, rounds=0, max_iter=0, min_inliers=0):
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    Rt_prior = np.asarray(Rt_prior, dtype=np.float64).reshape(3, 4)
    a = huber_a if huber_a > 0 else 16.0
    rounds = rounds or 4
    max_iter = max_iter or 50
    need = max(min_inliers if min_inliers > 0 else 8, 4)
    g2 = gate * gate
    p = np.concatenate([np_log(Rt_prior[:, :3]), Rt_prior[:, 3]])
    p0 = p.copy()
    zc, sq, _, _, _ = sums(p, X, x, K, a, np.zeros(len(X), bool))
    with np.errstate(invalid="ignore"):
        m = zc > 0.0
    masks, its, rounds_run, converged = [m.copy()], 0, 0, 0
    for _ in range(rounds):
        if m.sum() < 4:
            break
        p, it, zc, sq, _, _, _ = levenberg(p, X, x, K, a, m, max_iter)
        its += it
        rounds_run += 1
        m_next = classify(zc, sq, g2)
        masks.append(m_next.copy())
        same = np.array_equal(m_next, m)
        m = m_next
        if same:
            converged = 1
            break
    zc, sq, A, _, cost = sums(p, X, x, K, a, np.ones(len(X), bool))
    mask = classify(zc, sq, g2)
    _, _, A, _, cost = sums(p, X, x, K, a, mask)
    n_in = int(mask.sum())
    result = OK if n_in >= need else FEW
    moved = not np.array_equal(p, p0)
    Rt = np.concatenate([np_exp(p[:3]), p[3:, None]], 1) if moved else Rt_prior.copy()
    cov = np.zeros((6, 6))
    if result == OK and solve6(A, np.zeros(6), 0.0) is not None:
        cov = np.linalg.inv(A)
    return dict(Rt=Rt, p=p, cov=cov, mask=mask, masks=masks, n_inliers=n_in, rmse=float(np.sqrt(cost / (2 * n_in))) if n_in else 0.0,
                iterations=its, rounds_run=rounds_run, converged=converged, result=result)

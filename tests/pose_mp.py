"""50-digit reference of the single-pose refinement (mpmath, mp.dps = 50): the operation coloc_amd/csrc/pnp.hip's pnp_refine_kernel and
the scoring kernels compute, stated plainly and without any of the product's formulas.

  exp_so3 / log_so3      rotation <-> angle-axis (logarithm: angle from atan2(|a| / 2, (tr - 1) / 2), axis from the symmetric part near pi)
  project / residual / sq_err      pixel projection with the FULL 3 x 3 K (u / w, v / w), obs - proj, its squared norm
  huber_cost             1/2 sum rho(||r||^2), rho(s) = s for s <= a^2, 2 a sqrt(s) - a^2 beyond (pnp.hip, ceres::HuberLoss(a^2))
  normal_equations       A = sum w_i J_i^T J_i, g = sum w_i J_i^T r_i (descent right-hand side), cost; J the 2 x 6 Jacobian of the
                         PROJECTION in [angle-axis | t], w = 1 inside, a / ||r|| in the tail
  newton_polish          Gauss-Newton steps d = A^-1 g at 50 digits until ||d||_inf < 1e-30: the reference minimiser

Derivatives are central differences at 50 digits (step 1e-20: truncation 1e-40 relative): of the rotation matrix with respect to
the angle-axis vector and of the pixel with respect to the camera-frame point, combined by the chain rule -- no closed-form rotation
derivative (the product's is Gallego & Yezzi's; the reference must not share it).  jacobian_direct differences the whole projection
instead; the tests hold the two to each other.  Plain lists of mpf, no vectorisation: a pass over 600 points takes about half a second.
"""
from mpmath import mp, mpf

mp.dps = 50
H_STEP = mpf(10) ** -20


def vec(a):
    return [mpf(float(v)) if not isinstance(v, mpf) else v for v in a]


def mat3(a):
    """3 x 3 nested list of mpf from a numpy array / nested list / flat 9."""
    flat = [v for row in a for v in (row if hasattr(row, "__len__") else [row])]
    flat = vec(flat)
    return [flat[0:3], flat[3:6], flat[6:9]]


def _skew(w):
    return [[mpf(0), -w[2], w[1]], [w[2], mpf(0), -w[0]], [-w[1], w[0], mpf(0)]]


def _matmul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def exp_so3(w):
    """R = I + sin(th)/th [w]x + 2 sin^2(th/2)/th^2 [w]x^2."""
    w = vec(w)
    th = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    eye = [[mpf(int(i == j)) for j in range(3)] for i in range(3)]
    if th == 0:
        return eye
    W = _skew(w)
    W2 = _matmul(W, W)
    a = mp.sin(th) / th
    b = 2 * mp.sin(th / 2) ** 2 / (th * th)
    return [[eye[i][j] + a * W[i][j] + b * W2[i][j] for j in range(3)] for i in range(3)]


def log_so3(R):
    R = mat3(R)
    a = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    s = mp.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) / 2
    c = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    th = mp.atan2(s, c)
    if c > 0:
        if s == 0:
            return [v / 2 for v in a]
        return [th * v / (2 * s) for v in a]
    # axis from the symmetric part (R + R^T) / 2 = c I + (1 - c) k k^T: k_p^2 from the largest diagonal entry, the others by division
    S = [[(R[i][j] + R[j][i]) / 2 for j in range(3)] for i in range(3)]
    p = max(range(3), key=lambda i: S[i][i])
    kp = mp.sqrt((S[p][p] - c) / (1 - c))
    k = [kp if j == p else S[p][j] / ((1 - c) * kp) for j in range(3)]
    if k[0] * a[0] + k[1] * a[1] + k[2] * a[2] < 0:
        k = [-v for v in k]
    return [th * v for v in k]


def cam_point(R, t, X):
    return [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]


def pixel(K, Xc):
    """(u / w, v / w, w) of K Xc with the full K."""
    u = K[0][0] * Xc[0] + K[0][1] * Xc[1] + K[0][2] * Xc[2]
    v = K[1][0] * Xc[0] + K[1][1] * Xc[1] + K[1][2] * Xc[2]
    w = K[2][0] * Xc[0] + K[2][1] * Xc[1] + K[2][2] * Xc[2]
    return u / w, v / w, w


def project(K, R, t, X):
    u, v, _ = pixel(K, cam_point(R, t, X))
    return [u, v]


def residual(K, R, t, X, x):
    u, v = project(K, R, t, X)
    return [x[0] - u, x[1] - v]


def sq_err(K, R, t, X, x):
    r = residual(K, R, t, X, x)
    return r[0] * r[0] + r[1] * r[1]


def rho(s, a):
    return s if s <= a * a else 2 * a * mp.sqrt(s) - a * a


def _prep(X, x, K, mask):
    idx = [i for i in range(len(X)) if mask is None or mask[i]]
    return [vec(X[i]) for i in idx], [vec(x[i]) for i in idx], mat3(K)


def huber_cost(p, X, x, K, a=16.0, mask=None):
    p = vec(p); a = mpf(a)
    Xs, xs, Km = _prep(X, x, K, mask)
    R = exp_so3(p[:3])
    return sum((rho(sq_err(Km, R, p[3:], Xi, xi), a) for Xi, xi in zip(Xs, xs)), mpf(0)) / 2


def jacobian_direct(p, Xi, K):
    """2 x 6 Jacobian of one point's projection: central differences of the whole map p -> pixel."""
    p = vec(p); Xi = vec(Xi); Km = mat3(K)
    J = [[None] * 6, [None] * 6]
    for k in range(6):
        pp = list(p); pm = list(p)
        pp[k] += H_STEP; pm[k] -= H_STEP
        up = project(Km, exp_so3(pp[:3]), pp[3:], Xi)
        um = project(Km, exp_so3(pm[:3]), pm[3:], Xi)
        J[0][k] = (up[0] - um[0]) / (2 * H_STEP)
        J[1][k] = (up[1] - um[1]) / (2 * H_STEP)
    return J


def d_exp_so3(w):
    """[k][i][j] = dR_ij / dw_k by central differences."""
    w = vec(w)
    out = []
    for k in range(3):
        wp = list(w); wm = list(w)
        wp[k] += H_STEP; wm[k] -= H_STEP
        Rp, Rm = exp_so3(wp), exp_so3(wm)
        out.append([[(Rp[i][j] - Rm[i][j]) / (2 * H_STEP) for j in range(3)] for i in range(3)])
    return out


def normal_equations(p, X, x, K, a=16.0, mask=None):
    """(A 6 x 6 mp.matrix, g 6 x 1 mp.matrix, cost) at parameters p over the masked correspondences."""
    p = vec(p); a = mpf(a)
    Xs, xs, Km = _prep(X, x, K, mask)
    R = exp_so3(p[:3]); t = p[3:]
    dR = d_exp_so3(p[:3])
    A = [[mpf(0)] * 6 for _ in range(6)]
    g = [mpf(0)] * 6
    cost = mpf(0)
    two_h = 2 * H_STEP
    for Xi, xi in zip(Xs, xs):
        Xc = cam_point(R, t, Xi)
        u, v, _ = pixel(Km, Xc)
        r0, r1 = xi[0] - u, xi[1] - v
        s = r0 * r0 + r1 * r1
        cost += rho(s, a)
        wgt = mpf(1) if s <= a * a else a / mp.sqrt(s)
        # d(pixel)/d(Xc): central differences, 2 x 3
        P = [[None] * 3, [None] * 3]
        for m in range(3):
            cp = list(Xc); cm = list(Xc)
            cp[m] += H_STEP; cm[m] -= H_STEP
            up, vp, _ = pixel(Km, cp)
            um, vm, _ = pixel(Km, cm)
            P[0][m] = (up - um) / two_h
            P[1][m] = (vp - vm) / two_h
        Ju = [None] * 6; Jv = [None] * 6
        for k in range(3):
            d = [dR[k][i][0] * Xi[0] + dR[k][i][1] * Xi[1] + dR[k][i][2] * Xi[2] for i in range(3)]
            Ju[k] = P[0][0] * d[0] + P[0][1] * d[1] + P[0][2] * d[2]
            Jv[k] = P[1][0] * d[0] + P[1][1] * d[1] + P[1][2] * d[2]
            Ju[3 + k] = P[0][k]; Jv[3 + k] = P[1][k]
        for i in range(6):
            wu, wv = wgt * Ju[i], wgt * Jv[i]
            g[i] += wu * r0 + wv * r1
            Ai = A[i]
            for j in range(i, 6):
                Ai[j] += wu * Ju[j] + wv * Jv[j]
    for i in range(6):
        for j in range(i):
            A[i][j] = A[j][i]
    return mp.matrix(A), mp.matrix(g), cost / 2


def newton_step(p, X, x, K, a=16.0, mask=None):
    """(d = A^-1 g, A, g, cost)."""
    A, g, cost = normal_equations(p, X, x, K, a, mask)
    return mp.lu_solve(A, g), A, g, cost


def newton_polish(p, X, x, K, a=16.0, mask=None, tol=mpf(10) ** -30, max_steps=80):
    """Gauss-Newton from a float64 start to ||A^-1 g||_inf < tol.  Returns (p, steps); raises if it does not get there."""
    p = vec(p)
    for it in range(max_steps):
        d, _, _, _ = newton_step(p, X, x, K, a, mask)
        if max(abs(d[i]) for i in range(6)) < tol:
            return p, it
        p = [p[i] + d[i] for i in range(6)]
    raise RuntimeError("newton_polish: no convergence in %d steps" % max_steps)


def to_float(v):
    import numpy as np
    if isinstance(v, mp.matrix):
        return np.array([[float(v[i, j]) for j in range(v.cols)] for i in range(v.rows)])
    if isinstance(v, list) and v and isinstance(v[0], list):
        return np.array([[float(e) for e in row] for row in v])
    return np.array([float(e) for e in v])

"""50-digit reference of the map's bundle adjustment (mpmath, mp.dps = 50; built on tests/pose_mp.py): the operation
coloc_amd/csrc/ba_math.h and the kernels of coloc_amd/csrc/map_ba.hip compute, stated plainly and without any of the product's formulas.

A problem is a dict: K (n_cams x 3: focal, ppx, ppy), mask (bit c: camera c is adjusted), obs (n_points masks), x (n_points x n_cams x
2 undistorted pixels), a (Huber).  Parameters p = [angle-axis | t] of every MASKED camera in ascending order, then X of every point that
carries an observation of a masked camera in ascending order (pack / unpack).

  cost / residuals       1/2 sum rho(|r|^2), r = x - (f hnormalized(R X + t) + pp); per observation (r, weight)
  jacobian_rows          the projection's 2 x n Jacobian rows per observation by central differences (step 1e-20) of the WHOLE map
                         parameters -> pixel: no closed-form derivative of anything
  normal_equations       A = sum w J^T J, g = sum w J^T r (descent right-hand side), cost
  gauge_directions       the seven directions the cost does not see (three translations, three rotations, scale), as tangent vectors at p,
                         by central differences of the group action itself
  null_directions        those and, per point seen by ONE camera, its viewing ray (A is singular there too: rank 2 of 3)
  polish                 Newton from a float64 start until the step is < 1e-30: the reference minimiser.  The step is taken in the
                         complement of the gauge directions (a bordered system, eliminated through the landmarks' Schur complement at 50
                         digits) with the cost's own Hessian by differences; (A + mu I) d = g with the Gauss-Newton A converges too,
                         but on these scenes -- a narrow baseline and a 39 px residual -- at one bit a step.
"""
from mpmath import mp, mpf

import pose_mp as pm

mp.dps = 50
H = pm.H_STEP


def _extra(fn):
    """runs fn at 75 digits: a central difference at step 1e-20 loses 20 digits to rounding, and what it returns is to carry 50"""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with mp.workdps(75):
            return fn(*a, **kw)
    return wrapped


def cams_of(prob):
    return [c for c in range(len(prob["K"])) if (prob["mask"] >> c) & 1]


def bits_of(prob, t):
    b = int(prob["obs"][t])
    return [c for c in cams_of(prob) if (b >> c) & 1]


def points_of(prob):
    return [t for t in range(len(prob["obs"])) if bits_of(prob, t)]


def pack(prob, pars, X):
    """pars[c] (6) per camera index, X[t] (3) per point -> p"""
    p = []
    for c in cams_of(prob):
        p += pm.vec(pars[c])
    for t in points_of(prob):
        p += pm.vec(X[t])
    return p


def unpack(prob, p):
    """-> ({camera: 6}, {point: 3})"""
    cams, pts = cams_of(prob), points_of(prob)
    pars = {c: p[6 * i:6 * i + 6] for i, c in enumerate(cams)}
    X = {t: p[6 * len(cams) + 3 * k:6 * len(cams) + 3 * k + 3] for k, t in enumerate(pts)}
    return pars, X


def observations(prob):
    """[(t, c)] in ascending point, then camera"""
    return [(t, c) for t in points_of(prob) for c in bits_of(prob, t)]


def project(Kc, par, X):
    """pixel and depth"""
    Xc = pm.cam_point(pm.exp_so3(par[:3]), par[3:], X)
    return [Kc[0] * Xc[0] / Xc[2] + Kc[1], Kc[0] * Xc[1] / Xc[2] + Kc[2]], Xc[2]


def _K(prob):
    return [pm.vec(k) for k in prob["K"]]


def residuals(prob, p):
    """[(t, c, r0, r1, weight, depth)]"""
    pars, X = unpack(prob, pm.vec(p))
    K = _K(prob)
    a = mpf(prob["a"])
    out = []
    for t, c in observations(prob):
        u, z = project(K[c], pars[c], X[t])
        xo = pm.vec(prob["x"][t][c])
        r0, r1 = xo[0] - u[0], xo[1] - u[1]
        s = r0 * r0 + r1 * r1
        out.append((t, c, r0, r1, mpf(1) if s <= a * a else a / mp.sqrt(s), z))
    return out


def cost(prob, p):
    """1/2 sum rho; +inf where a depth is not positive"""
    a = mpf(prob["a"])
    total = mpf(0)
    for _, _, r0, r1, _, z in residuals(prob, p):
        if z <= 0:
            return mp.inf
        total += pm.rho(r0 * r0 + r1 * r1, a)
    return total / 2


@_extra
def jacobian_rows(prob, p):
    """[(t, c, {index: du}, {index: dv})]: the nonzero columns of each observation's rows, central differences of the projection"""
    p = pm.vec(p)
    cams, pts = cams_of(prob), points_of(prob)
    K = _K(prob)
    ci = {c: i for i, c in enumerate(cams)}
    pi = {t: k for k, t in enumerate(pts)}
    pars, X = unpack(prob, p)
    # the rotations of every camera at its parameters displaced by +-H, formed once (exp_so3 is the expensive part of the map)
    rot = {}
    for c in cams:
        rot[(c, 0, 0)] = (pm.exp_so3(pars[c][:3]), list(pars[c][3:]))
        for m in range(6):
            for sgn in (1, -1):
                q = list(pars[c])
                q[m] += sgn * H
                rot[(c, m, sgn)] = (pm.exp_so3(q[:3]), q[3:]) if m < 3 else (rot[(c, 0, 0)][0], q[3:])

    def pix(Kc, Rt, Xt):
        Xc = pm.cam_point(Rt[0], Rt[1], Xt)
        return Kc[0] * Xc[0] / Xc[2] + Kc[1], Kc[0] * Xc[1] / Xc[2] + Kc[2]

    rows = []
    for t, c in observations(prob):
        cols = list(range(6 * ci[c], 6 * ci[c] + 6)) + list(range(6 * len(cams) + 3 * pi[t], 6 * len(cams) + 3 * pi[t] + 3))
        du, dv = {}, {}
        for m, col in enumerate(cols):
            if m < 6:
                up, um = pix(K[c], rot[(c, m, 1)], X[t]), pix(K[c], rot[(c, m, -1)], X[t])
            else:
                Xp = list(X[t]); Xm = list(X[t])
                Xp[m - 6] += H; Xm[m - 6] -= H
                up, um = pix(K[c], rot[(c, 0, 0)], Xp), pix(K[c], rot[(c, 0, 0)], Xm)
            du[col] = (up[0] - um[0]) / (2 * H)
            dv[col] = (up[1] - um[1]) / (2 * H)
        rows.append((t, c, du, dv))
    return rows


@_extra
def normal_equations(prob, p):
    """(A n x n nested list, g list, cost)"""
    p = pm.vec(p)
    n = len(p)
    A = [[mpf(0)] * n for _ in range(n)]
    g = [mpf(0)] * n
    res = residuals(prob, p)
    a = mpf(prob["a"])
    total = mpf(0)
    for (t, c, du, dv), (_, _, r0, r1, w, _) in zip(jacobian_rows(prob, p), res):
        total += pm.rho(r0 * r0 + r1 * r1, a)
        cols = list(du)
        for i in cols:
            g[i] += w * (du[i] * r0 + dv[i] * r1)
            for j in cols:
                A[i][j] += w * (du[i] * du[j] + dv[i] * dv[j])
    return A, g, total / 2


def _act(prob, p, kind, k, eps):
    """the similarity's action on p: kind 't' translate along axis k, 'r' rotate about axis k, 's' scale, each by eps"""
    pars, X = unpack(prob, p)
    if kind == "r":
        w = [mpf(0)] * 3
        w[k] = eps
        Q = pm.exp_so3(w)                                      # X' = Q X, R' = R Q^T, t' = t
    out_pars, out_X = {}, {}
    for c, par in pars.items():
        R = pm.exp_so3(par[:3])
        t = list(par[3:])
        if kind == "t":                                        # X' = X + eps e_k, t' = t - eps R e_k
            t = [t[i] - eps * R[i][k] for i in range(3)]
        elif kind == "r":
            R = [[sum(R[i][m] * Q[j][m] for m in range(3)) for j in range(3)] for i in range(3)]
        else:                                                  # X' = (1 + eps) X, t' = (1 + eps) t
            t = [(1 + eps) * v for v in t]
        out_pars[c] = list(pm.log_so3(R)) + t
    for t_, Xt in X.items():
        if kind == "t":
            Xn = list(Xt)
            Xn[k] += eps
        elif kind == "r":
            Xn = [sum(Q[i][m] * Xt[m] for m in range(3)) for i in range(3)]
        else:
            Xn = [(1 + eps) * v for v in Xt]
        out_X[t_] = Xn
    return pack(prob, out_pars, out_X)


@_extra
def gauge_directions(prob, p):
    """seven tangent vectors at p"""
    p = pm.vec(p)
    out = []
    for kind, ks in (("t", range(3)), ("r", range(3)), ("s", [0])):
        for k in ks:
            pp, pm_ = _act(prob, p, kind, k, H), _act(prob, p, kind, k, -H)
            out.append([(u - v) / (2 * H) for u, v in zip(pp, pm_)])
    return out


@_extra
def null_directions(prob, p):
    p = pm.vec(p)
    dirs = gauge_directions(prob, p)
    cams, pts = cams_of(prob), points_of(prob)
    pars, X = unpack(prob, p)
    for k, t in enumerate(pts):
        b = bits_of(prob, t)
        if len(b) != 1:
            continue
        par = pars[b[0]]
        R = pm.exp_so3(par[:3])
        C = [-sum(R[m][i] * par[3 + m] for m in range(3)) for i in range(3)]      # -R^T t
        d = [mpf(0)] * len(p)
        for i in range(3):
            d[6 * len(cams) + 3 * k + i] = X[t][i] - C[i]
        dirs.append(d)
    return dirs


def _orthonormal(dirs):
    basis = []
    for d in dirs:
        v = list(d)
        for _ in range(2):
            for b in basis:
                s = sum(x * y for x, y in zip(v, b))
                v = [x - s * y for x, y in zip(v, b)]
        nrm = mp.sqrt(sum(x * x for x in v))
        basis.append([x / nrm for x in v])
    return basis


H2 = mpf(10) ** -12          # second differences: truncation 1e-24, rounding 1e-26 relative


def _rotation_derivatives(w):
    """(R, dR[k], d2R[i][j]) of exp_so3 at w by central first (H) and second (H2) differences"""
    w = pm.vec(w)

    def at(shift):
        return pm.exp_so3([w[i] + shift[i] for i in range(3)])

    def e(k, s):
        return [s if i == k else mpf(0) for i in range(3)]
    R = at([mpf(0)] * 3)
    dR = pm.d_exp_so3(w)
    d2R = [[None] * 3 for _ in range(3)]
    for i in range(3):
        Rp, Rm = at(e(i, H2)), at(e(i, -H2))
        d2R[i][i] = [[(Rp[r][q] - 2 * R[r][q] + Rm[r][q]) / (H2 * H2) for q in range(3)] for r in range(3)]
        for j in range(i + 1, 3):
            quad = [at([u + v for u, v in zip(e(i, si * H2), e(j, sj * H2))]) for si, sj in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
            d2R[i][j] = d2R[j][i] = [[(quad[0][r][q] - quad[1][r][q] - quad[2][r][q] + quad[3][r][q]) / (4 * H2 * H2) for q in range(3)] for r in range(3)]
    return R, dR, d2R


def _term_hessian(Kc, par, X, xo, a, rot):
    """9 x 9 Hessian of ONE observation's cost term 1/2 rho(|x - pixel(R(w) X + t)|^2) in (w, t, X): the term is phi(Xc), Xc = R(w) X + t,
    so it is J^T (grad^2 phi) J + sum_m (d phi / d Xc_m) grad^2 Xc_m -- phi's derivatives by differences of phi itself, Xc's from the
    differenced rotation."""
    R, dR, d2R = rot
    Xc = pm.cam_point(R, par[3:], X)

    def phi(v):
        r0, r1 = xo[0] - (Kc[0] * v[0] / v[2] + Kc[1]), xo[1] - (Kc[0] * v[1] / v[2] + Kc[2])
        return pm.rho(r0 * r0 + r1 * r1, a) / 2

    def sh(i, s, j=None, sj=None):
        v = list(Xc)
        v[i] += s
        if j is not None:
            v[j] += sj
        return v
    f0 = phi(Xc)
    gphi = [(phi(sh(i, H)) - phi(sh(i, -H))) / (2 * H) for i in range(3)]
    Hphi = [[None] * 3 for _ in range(3)]
    for i in range(3):
        Hphi[i][i] = (phi(sh(i, H2)) - 2 * f0 + phi(sh(i, -H2))) / (H2 * H2)
        for j in range(i + 1, 3):
            Hphi[i][j] = Hphi[j][i] = (phi(sh(i, H2, j, H2)) - phi(sh(i, H2, j, -H2)) - phi(sh(i, -H2, j, H2)) + phi(sh(i, -H2, j, -H2))) / (4 * H2 * H2)
    # J: 3 x 9, columns w_k: dR_k X, t_k: e_k, X_a: R[:, a]
    J = [[None] * 9 for _ in range(3)]
    for m in range(3):
        for k in range(3):
            J[m][k] = dR[k][m][0] * X[0] + dR[k][m][1] * X[1] + dR[k][m][2] * X[2]
            J[m][3 + k] = mpf(int(m == k))
            J[m][6 + k] = R[m][k]
    M = [[Hphi[m][0] * J[0][j] + Hphi[m][1] * J[1][j] + Hphi[m][2] * J[2][j] for j in range(9)] for m in range(3)]
    Hl = [[J[0][i] * M[0][j] + J[1][i] * M[1][j] + J[2][i] * M[2][j] for j in range(9)] for i in range(9)]
    for m in range(3):
        for i in range(3):
            for j in range(3):
                Hl[i][j] += gphi[m] * (d2R[i][j][m][0] * X[0] + d2R[i][j][m][1] * X[1] + d2R[i][j][m][2] * X[2])
                Hl[i][6 + j] += gphi[m] * dR[i][m][j]
                Hl[6 + j][i] += gphi[m] * dR[i][m][j]
    return Hl


@_extra
def newton_step(prob, p):
    """(d, g, cost): the Newton step  min 1/2 d^T H d - g^T d  over the d orthogonal to the seven gauge directions, through the Schur
    complement on the points (every point of prob needs two observations: polish sees to that).  H is the cost's own Hessian, term by
    term (_term_hessian): Gauss-Newton's w J^T J leaves out the curvature of the projection, which at a 39 px residual on a narrow
    baseline is most of a point's depth curvature -- it then gains one bit a step."""
    p = pm.vec(p)
    cams, pts = cams_of(prob), points_of(prob)
    nc = 6 * len(cams)
    n = len(p)
    U = [[mpf(0)] * nc for _ in range(nc)]
    V = [[[mpf(0)] * 3 for _ in range(3)] for _ in pts]
    W = {}
    g = [mpf(0)] * n
    pi = {t: k for k, t in enumerate(pts)}
    res = residuals(prob, p)
    a = mpf(prob["a"])
    total = mpf(0)
    pars, Xs = unpack(prob, p)
    K = _K(prob)
    second = {c: _rotation_derivatives(pars[c][:3]) for c in cams}
    for (t, c, du, dv), (_, _, r0, r1, w, _) in zip(jacobian_rows(prob, p), res):
        s = r0 * r0 + r1 * r1
        total += pm.rho(s, a)
        cols = list(du)
        cc, pc = cols[:6], cols[6:]
        for i in cols:
            g[i] += w * (du[i] * r0 + dv[i] * r1)
        Hl = _term_hessian(K[c], pars[c], Xs[t], pm.vec(prob["x"][t][c]), a, second[c])
        for i in range(6):
            for j in range(6):
                U[cc[i]][cc[j]] += Hl[i][j]
        k = pi[t]
        for i in range(3):
            for j in range(3):
                V[k][i][j] += Hl[6 + i][6 + j]
        W[(k, cc[0])] = [[Hl[i][6 + j] for j in range(3)] for i in range(6)]
    # the bordered system [[H, N], [N^T, 0]] [d; nu] = [g; 0]: the border's seven rows are one more block of 7 "camera" unknowns
    N = gauge_directions(prob, p)
    ne = nc + 7
    S = mp.matrix(ne, ne)
    rhs = mp.matrix(ne, 1)
    for i in range(nc):
        rhs[i] = g[i]
        for j in range(nc):
            S[i, j] = U[i][j]
        for q in range(7):
            S[i, nc + q] = S[nc + q, i] = N[q][i]
    by_point = {k: [(nc, mp.matrix([[N[q][nc + 3 * k + i] for i in range(3)] for q in range(7)]))] for k in range(len(pts))}
    for (k, c0), Wkc in W.items():
        by_point[k].append((c0, mp.matrix(Wkc)))                      # 6 x 3 each
    Vinv = [mp.matrix(V[k]) ** -1 for k in range(len(pts))]
    for k, blocks in by_point.items():
        gt = mp.matrix(g[nc + 3 * k:nc + 3 * k + 3])
        for c0, Wm in blocks:
            Y = Wm * Vinv[k]
            yg = Y * gt
            for i in range(Wm.rows):
                rhs[c0 + i] -= yg[i]
            for c1, W2 in blocks:
                B = Y * W2.T
                for i in range(Wm.rows):
                    for j in range(W2.rows):
                        S[c0 + i, c1 + j] -= B[i, j]
    dc = mp.lu_solve(S, rhs)
    d = [dc[i] for i in range(nc)] + [mpf(0)] * (n - nc)
    for k in range(len(pts)):
        s = mp.matrix(g[nc + 3 * k:nc + 3 * k + 3])
        for c0, Wm in by_point[k]:
            s -= Wm.T * mp.matrix([dc[c0 + i] for i in range(Wm.rows)])
        dx = Vinv[k] * s
        for i in range(3):
            d[nc + 3 * k + i] = dx[i]
    return d, g, total / 2


def drop_single_observations(prob):
    """the problem without the observation of every point that only one masked camera sees"""
    out = dict(prob)
    out["obs"] = [int(prob["obs"][t]) if len(bits_of(prob, t)) != 1 else 0 for t in range(len(prob["obs"]))]
    return out


def onto_ray(prob, pars, X, t):
    """the point of the viewing ray of point t's ONE observation at the depth X has now: residual 0"""
    c = bits_of(prob, t)[0]
    Kc = pm.vec(prob["K"][c])
    xo = pm.vec(prob["x"][t][c])
    R = pm.exp_so3(pars[c][:3])
    z = pm.cam_point(R, pars[c][3:], X)[2]
    Xc = [z * (xo[0] - Kc[1]) / Kc[0], z * (xo[1] - Kc[2]) / Kc[0], z]
    return [sum(R[m][i] * (Xc[m] - pars[c][3 + m]) for m in range(3)) for i in range(3)]


def polish(prob, p, tol=mpf(10) ** -30, max_steps=25):
    """Newton from a float64 start until the step is < tol.  Returns (p, steps); raises if it does not get there.  A point that one
    camera sees can always be moved onto its ray, so at the minimum its term is 0 and it binds nothing: its observation is left out of
    the iteration (its block of the Hessian has rank 2) and the point is put onto the ray of the polished camera at the end."""
    p = pm.vec(p)
    pars, X = unpack(prob, p)
    red = drop_single_observations(prob)
    q = pack(red, pars, X)
    for it in range(max_steps):
        d, _, _ = newton_step(red, q)
        if max(abs(v) for v in d) < tol:
            pars, Xr = unpack(red, q)
            X = {t: (Xr[t] if t in Xr else onto_ray(prob, pars, X[t], t)) for t in points_of(prob)}
            return pack(prob, pars, X), it
        q = [u + v for u, v in zip(q, d)]
    raise RuntimeError("ba_mp.polish: no convergence in %d steps" % max_steps)

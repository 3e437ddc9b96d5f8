"""High-precision reference of the perspective-three-point problem (mpmath, 60 digits and more): what coloc_amd/csrc/p3p.h computes,
stated plainly, certified per solution, with the sensitivity each solution needs to be compared with a float64 solver.

  bearings           unit rays of three float pixels through a general upper-triangular K (skew included)
  quartic            Grunert's quartic in v = s3 / s1, built by polynomial arithmetic from the law of cosines on the three pairs
  solve              every real root v > 0 with u > 0 and W > 0 -> depths -> triads -> [R|t]; each solution certifies itself: the pose
                     maps the three world points onto the three scaled bearings to 1e-40, or the precision is raised (near-double
                     roots lose digits) until it does; solve raises NotCertified when it never does
  rho                smallest relative separation of any two of the four quartic roots, complex ones included
  sensitivity        J_k = sum_j |dP_k / dx_j| over the six pixel inputs, central differences with step 1e-20 (the perturbed solution is
                     followed by Newton on the three law-of-cosines equations from the unperturbed depths)
  backward_error     worst |du|, |dv| of a FLOAT pose on its own three sample points, evaluated at 50 digits
  bound_B / sigma    the two quantities of the rules in DESIGN.md (P3P): B = 4096 * 2^-53 * max(|x|_inf, fx, fy), sigma = sine of
                     the world triangle's angle at the first sample point

Plain lists of mpf, no vectorisation.  A problem with two solutions and their sensitivities takes about 30 ms.
"""
from mpmath import mp, mpf

DPS = 60
CERT_TOL = mpf(10) ** -40
DIFF_STEP = mpf(10) ** -20
MAX_DPS = 480


class NotCertified(Exception):
    pass


def _v(a):
    return [mpf(float(e)) for e in a]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _unit(a):
    n = mp.sqrt(_dot(a, a))
    return [a[0] / n, a[1] / n, a[2] / n]


def _pmul(a, b):
    out = [mpf(0)] * (len(a) + len(b) - 1)
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            out[i + j] += ai * bj
    return out


def _padd(*ps):
    n = max(len(p) for p in ps)
    return [sum((p[i] for p in ps if i < len(p)), mpf(0)) for i in range(n)]


def _pscale(s, a):
    return [s * e for e in a]


def _peval(p, v):
    acc = mpf(0)
    for c in reversed(p):
        acc = acc * v + c
    return acc


def bearings(x, K):
    """Unit rays K^-1 (u, v, 1) of three pixels; K upper triangular with K[2][2] = 1."""
    fx, sk, cx, fy, cy = (mpf(float(K[0][0])), mpf(float(K[0][1])), mpf(float(K[0][2])), mpf(float(K[1][1])), mpf(float(K[1][2])))
    out = []
    for u, v in x:
        yn = (mpf(float(v)) - cy) / fy
        xn = (mpf(float(u)) - cx - sk * yn) / fx
        out.append(_unit([xn, yn, mpf(1)]))
    return out


def sides_and_cosines(X, f):
    """(a2, b2, c2) = |X1 X2|^2, |X0 X2|^2, |X0 X1|^2 and (ca, cb, cg) = f1.f2, f0.f2, f0.f1."""
    d01, d02, d12 = _sub(X[0], X[1]), _sub(X[0], X[2]), _sub(X[1], X[2])
    return (_dot(d12, d12), _dot(d02, d02), _dot(d01, d01)), (_dot(f[1], f[2]), _dot(f[0], f[2]), _dot(f[0], f[1]))


def quartic(sides, cosines):
    """(co ascending, N, D, W): s2 = u s1, s3 = v s1; u = N(v) / D(v); s1^2 W(v) = b2; co(v) = 0."""
    a2, b2, c2 = sides
    ca, cb, cg = cosines
    q = (a2 - c2) / b2
    N = [q + 1, -2 * q * cb, q - 1]
    D = [2 * cg, -2 * ca]
    W = [mpf(1), -2 * cb, mpf(1)]
    DD = _pmul(D, D)
    co = _padd(_pscale(b2, _padd(DD, _pmul(N, N), _pscale(-2 * cg, _pmul(N, D)))), _pscale(-c2, _pmul(DD, W)))
    return co, N, D, W


def _g(s, sides, cosines):
    a2, b2, c2 = sides
    ca, cb, cg = cosines
    return [s[0] * s[0] + s[1] * s[1] - 2 * s[0] * s[1] * cg - c2,
            s[0] * s[0] + s[2] * s[2] - 2 * s[0] * s[2] * cb - b2,
            s[1] * s[1] + s[2] * s[2] - 2 * s[1] * s[2] * ca - a2]


def _newton_depths(s, sides, cosines, steps):
    """Newton on the three law-of-cosines equations; returns (depths, size of the last step)."""
    ca, cb, cg = cosines
    last = mpf(1)
    for _ in range(steps):
        g = _g(s, sides, cosines)
        Jm = mp.matrix([[2 * (s[0] - s[1] * cg), 2 * (s[1] - s[0] * cg), 0],
                        [2 * (s[0] - s[2] * cb), 0, 2 * (s[2] - s[0] * cb)],
                        [0, 2 * (s[1] - s[2] * ca), 2 * (s[2] - s[1] * ca)]])
        try:
            d = mp.lu_solve(Jm, mp.matrix(g))
        except ZeroDivisionError:
            return s, mpf(1)
        s = [s[0] - d[0], s[1] - d[1], s[2] - d[2]]
        last = max(abs(d[0]), abs(d[1]), abs(d[2]))
        if last == 0:
            break
    return s, last


def triad(A, B, C):
    """Columns e1, e2, e3 of the orthonormal frame of three points: e1 along AB, e3 normal to the plane."""
    e1 = _unit(_sub(B, A))
    e3 = _unit(_cross(e1, _sub(C, A)))
    e2 = _cross(e3, e1)
    return [[e1[i], e2[i], e3[i]] for i in range(3)]


def pose_from_depths(X, f, s):
    """12 mpf, row-major [R|t], x_cam = R X + t, and the certificate max |R X_i + t - s_i f_i|."""
    Q = [[s[i] * f[i][j] for j in range(3)] for i in range(3)]
    E = triad(X[0], X[1], X[2])
    G = triad(Q[0], Q[1], Q[2])
    R = [[G[i][0] * E[j][0] + G[i][1] * E[j][1] + G[i][2] * E[j][2] for j in range(3)] for i in range(3)]
    t = [Q[0][i] - _dot(R[i], X[0]) for i in range(3)]
    cert = max(abs(_dot(R[i], X[p]) + t[i] - Q[p][i]) for p in range(3) for i in range(3))
    P = [R[0][0], R[0][1], R[0][2], t[0], R[1][0], R[1][1], R[1][2], t[1], R[2][0], R[2][1], R[2][2], t[2]]
    return P, cert


def _solve_at(X, x, K, dps):
    with mp.workdps(dps):
        Xm = [_v(p) for p in X]
        f = bearings(x, K)
        sides, cosines = sides_and_cosines(Xm, f)
        co, N, D, W = quartic(sides, cosines)
        roots = mp.polyroots(list(reversed(co)), maxsteps=400, extraprec=4 * dps)
        sep = min(abs(roots[i] - roots[j]) / max(abs(roots[i]), abs(roots[j])) for i in range(4) for j in range(i))
        real_tol = mpf(10) ** (-dps // 3)
        step_tol = mpf(10) ** (8 - dps)
        vs = []
        for r in roots:
            if abs(mp.im(r)) > real_tol * (1 + abs(mp.re(r))):
                continue
            v = mp.re(r)
            if not any(abs(v - w) <= real_tol * (1 + abs(v)) for w in vs):      # a double root is one solution
                vs.append(v)
        sols = []
        for v in sorted(vs):
            if not v > 0:
                continue
            den, w = _peval(D, v), _peval(W, v)
            if den == 0 or not w > 0:
                continue
            u = _peval(N, v) / den
            if not u > 0:
                continue
            s1 = mp.sqrt(sides[1] / w)
            s, last = _newton_depths([s1, u * s1, v * s1], sides, cosines, 12)
            if last > step_tol * (1 + max(s)) or min(s) <= 0:
                raise NotCertified("depths of root %s do not settle at %d digits" % (mp.nstr(v, 12), dps))
            P, cert = pose_from_depths(Xm, f, s)
            if cert > CERT_TOL:
                raise NotCertified("certificate %s at %d digits" % (mp.nstr(cert, 3), dps))
            sols.append(dict(v=v, s=s, P=P, cert=cert))
        return dict(sols=sols, rho=sep, co=co, dps=dps, f=f, sides=sides, cosines=cosines, X=Xm)


def solve(X, x, K, dps=DPS):
    """All poses of the P3P problem on world points X (3 x 3 floats), pixels x (3 x 2 floats) and K: dict(sols=[dict(v, s, P, cert)],
    rho, co, dps) at the first precision dps, 2 dps, 4 dps, ... <= MAX_DPS at which every solution certifies itself."""
    err = None
    while dps <= MAX_DPS:
        try:
            return _solve_at(X, x, K, dps)
        except (NotCertified, mp.NoConvergence) as e:
            err = e
            dps *= 2
    raise NotCertified("never certified: %s" % err)


def sensitivity(X, x, K, sol, dps=DPS):
    """J (12 mpf): sum over the six pixel inputs of |dP_k / dx_j|, central differences with step DIFF_STEP."""
    with mp.workdps(max(dps, DPS)):
        Xm = [_v(p) for p in X]
        J = [mpf(0)] * 12
        for j in range(6):
            P2 = []
            for sign in (1, -1):
                xp = [[mpf(float(e)) for e in row] for row in x]
                xp[j // 2][j % 2] += sign * DIFF_STEP
                fx, sk, cx, fy, cy = (mpf(float(K[0][0])), mpf(float(K[0][1])), mpf(float(K[0][2])), mpf(float(K[1][1])), mpf(float(K[1][2])))
                f = []
                for u, v in xp:
                    yn = (v - cy) / fy
                    f.append(_unit([(u - cx - sk * yn) / fx, yn, mpf(1)]))
                sides, cosines = sides_and_cosines(Xm, f)
                s, last = _newton_depths(list(sol["s"]), sides, cosines, 6)
                if last > mpf(10) ** -35 * (1 + max(s)):
                    raise NotCertified("perturbed depths do not settle")
                P2.append(pose_from_depths(Xm, f, s)[0])
            for k in range(12):
                J[k] += abs(P2[0][k] - P2[1][k]) / (2 * DIFF_STEP)
        return J


def sigma(X):
    """Sine of the world triangle's angle at the first point."""
    with mp.workdps(DPS):
        Xm = [_v(p) for p in X]
        a, b = _sub(Xm[1], Xm[0]), _sub(Xm[2], Xm[0])
        c = _cross(a, b)
        return mp.sqrt(_dot(c, c) / (_dot(a, a) * _dot(b, b)))


def bound_B(x, K):
    """4096 roundings of the largest coordinate the data carries (float)."""
    big = max(max(abs(float(e)) for row in x for e in row), abs(float(K[0][0])), abs(float(K[1][1])))
    return 4096.0 * 2.0 ** -53 * big


def backward_error(P, X, x, K):
    """Worst |du|, |dv| (float) of the float pose P (12, row-major [R|t]) on its three sample points, evaluated at 50 digits
    through the full K."""
    with mp.workdps(50):
        Pm = _v(P)
        Km = [_v(row) for row in K]
        worst = mpf(0)
        for Xi, xi in zip(X, x):
            Xi = _v(Xi)
            c = [Pm[4 * i] * Xi[0] + Pm[4 * i + 1] * Xi[1] + Pm[4 * i + 2] * Xi[2] + Pm[4 * i + 3] for i in range(3)]
            h = [_dot(Km[i], c) for i in range(3)]
            worst = max(worst, abs(h[0] / h[2] - mpf(float(xi[0]))), abs(h[1] / h[2] - mpf(float(xi[1]))))
        return float(worst)


def pose_from_stored_depths(X, x, K, s_hi, s_lo):
    """(hi (12 floats), lo (12 floats), certificate) of the pose whose depths are s_hi + s_lo: the fixture keeps a reference solution
    as its three depths, and the pose is their triads, rebuilt here at DPS digits."""
    with mp.workdps(DPS):
        s = [mpf(float(h)) + mpf(float(l)) for h, l in zip(s_hi, s_lo)]
        P, cert = pose_from_depths([_v(p) for p in X], bearings(x, K), s)
        hi, lo = hi_lo(P)
        return hi, lo, cert


def hi_lo(vals):
    """float64 pairs (hi, lo) with hi + lo = the value to 2^-106."""
    with mp.workdps(DPS):
        hi = [float(v) for v in vals]
        lo = [float(v - mpf(h)) for v, h in zip(vals, hi)]
    return hi, lo

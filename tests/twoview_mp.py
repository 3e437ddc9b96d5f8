"""High-precision reference of the two-view minimal problems (mpmath, 60 digits and more): what coloc_amd/csrc/twoview_min.h ('F' seven
points, 'H' four points) and coloc_amd/csrc/fivept.h ('E' five points) compute, stated plainly, certified per solution, with the
sensitivity each solution needs to be compared with a float64 solver.  Nothing here is shared with the product or the oracle.

  condition          ACKernelAdaptor's conditioning by the image size, x_n = (x - (w, h) / 2) / sqrt(w h), at full precision
  nullspace          the last rows of V of mp.svd_r
  solve('F')         the pencil det(a + x b) = 0 by polynomial arithmetic, all three roots by mp.polyroots; each real root -> a unit-norm
                     model, Newton-polished on the full system and certified: det = 0 and the seven equations to 1e-50
  solve('H')         the one null vector of the 8 x 9 system, certified the same way
  rho                smallest chordal distance, on the projective line, between two of the pencil's three roots (complex ones included):
                     |x_i - x_j| / sqrt((1 + |x_i|^2)(1 + |x_j|^2)); an orthonormal change of the null-space basis is a unitary Moebius
                     map of the line, which leaves it unchanged
  sensitivity        J_k = sum_j |dM_k / dx_j| over the 28 (16, 20) sample pixel coordinates, M the unit-norm model: central differences
                     with step 1e-20, the perturbed model followed by chord-Newton steps on the full system until they settle at 1e-40
  backward_error     'F': distance in pixels that one point of each pair has to move for the nearest rank-2 matrix of a FLOAT model to be
                     exact (worst of the sample); 'H': worst |x2 - H x1| in pixels; 'E': as 'F' for the nearest essential matrix
  solve_five         Nister's five-point problem: null space, the ten cubic constraints by polynomial arithmetic, Gauss-Jordan
                     elimination, the action matrix's eigenvalues by mp.eig, Newton on the constraints in (x, y, z), certified

Plain lists of mpf.  A seven-point problem with its sensitivities takes about a quarter of a second.
"""
from mpmath import mp, mpf

DPS = 60
CERT_TOL = mpf(10) ** -50
DIFF_STEP = mpf(10) ** -20
MAX_DPS = 480


class NotCertified(Exception):
    pass


def _pmul(a, b):
    out = [mpf(0)] * (len(a) + len(b) - 1)
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            out[i + j] += ai * bj
    return out


def _padd(*ps):
    n = max(len(p) for p in ps)
    return [sum((p[i] for p in ps if i < len(p)), mpf(0)) for i in range(n)]


def _pneg(a):
    return [-e for e in a]


def _det3(m):
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def _cof3(m):
    """d det / d m_e, row-major."""
    return [m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6],
            m[2] * m[7] - m[1] * m[8], m[0] * m[8] - m[2] * m[6], m[1] * m[6] - m[0] * m[7],
            m[1] * m[5] - m[2] * m[4], m[2] * m[3] - m[0] * m[5], m[0] * m[4] - m[1] * m[3]]


def _unit_sign(m):
    n = mp.sqrt(sum(e * e for e in m))
    big = max(m, key=abs)
    s = n if big > 0 else -n
    return [e / s for e in m]


def condition(x, wh):
    """([(u, v)] conditioned, d): x_n = (x - (w, h) / 2) d, d = 1 / sqrt(w h); x may hold floats or mpf."""
    w, h = mpf(int(wh[0])), mpf(int(wh[1]))
    d = 1 / mp.sqrt(w * h)
    return [[(mpf(p[0]) - w / 2) * d, (mpf(p[1]) - h / 2) * d] for p in x], d


def _mpf_rows(x):
    return [[mpf(float(p[0])), mpf(float(p[1]))] for p in x]


def rows(model, q1, q2):
    """The linear equations of a sample on the row-major nine entries: x2^T F x1 = 0 ('F', 'E'), x2 ~ H x1 ('H')."""
    out = []
    for (u1, v1), (u2, v2) in zip(q1, q2):
        if model == "H":
            out.append([u1, v1, mpf(1), mpf(0), mpf(0), mpf(0), -u2 * u1, -u2 * v1, -u2])
            out.append([mpf(0), mpf(0), mpf(0), u1, v1, mpf(1), -v2 * u1, -v2 * v1, -v2])
        else:
            out.append([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, mpf(1)])
    return out


def nullspace(A, k):
    """k orthonormal vectors (lists of 9) spanning the null space of the (9 - k) x 9 system A."""
    _, _, V = mp.svd_r(mp.matrix(A), full_matrices=True, compute_uv=True)
    return [[V[9 - k + z, e] for e in range(9)] for z in range(k)]


def pencil_cubic(a, b):
    """Coefficients, ascending, of det(a + x b)."""
    e = [[a[i], b[i]] for i in range(9)]
    m = lambda p, q: _pmul(e[p], e[q])
    return _padd(_pmul(e[0], _padd(m(4, 8), _pneg(m(5, 7)))), _pneg(_pmul(e[1], _padd(m(3, 8), _pneg(m(5, 6))))),
                 _pmul(e[2], _padd(m(3, 7), _pneg(m(4, 6)))))


def chordal(r, s):
    return abs(r - s) / mp.sqrt((1 + abs(r) ** 2) * (1 + abs(s) ** 2))


def _essential_cubics(m):
    """The nine entries of 2 E E^T E - tr(E E^T) E."""
    EEt = [[sum(m[3 * i + k] * m[3 * j + k] for k in range(3)) for j in range(3)] for i in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    return [2 * sum(EEt[i][k] * m[3 * k + j] for k in range(3)) - tr * m[3 * i + j] for i in range(3) for j in range(3)]


def _residual(model, A, m):
    """The full system of a unit-norm model: the sample's equations, det m = 0 ('F', 'E'), 2 E E^T E - tr(E E^T) E = 0 ('E'), |m|^2 = 1."""
    g = [sum(r[e] * m[e] for e in range(9)) for r in A]
    if model != "H":
        g.append(_det3(m))
    if model == "E":
        g += _essential_cubics(m)
    g.append(sum(e * e for e in m) - 1)
    return g


def _jacobian(model, A, m):
    Jm = [list(r) for r in A]
    if model != "H":
        Jm.append(_cof3(m))
    if model == "E":                            # the cubics are homogeneous of degree 3 and exact polynomials: their derivative along e_k is
        cols = []                               # the polarisation P(m, m, e_k), read off P(m + e_k) - P(m - e_k) = 2 dP + 2 P(e_k)
        for k in range(9):
            up = [m[e] + (1 if e == k else 0) for e in range(9)]
            dn = [m[e] - (1 if e == k else 0) for e in range(9)]
            ek = [mpf(1 if e == k else 0) for e in range(9)]
            cols.append([(a - b) / 2 - c for a, b, c in zip(_essential_cubics(up), _essential_cubics(dn), _essential_cubics(ek))])
        Jm += [[cols[k][r] for k in range(9)] for r in range(9)]
    Jm.append([2 * e for e in m])
    return mp.matrix(Jm)


def _newton(model, A, m, steps):
    last = mpf(1)
    for _ in range(steps):
        try:
            d = mp.lu_solve(_jacobian(model, A, m), mp.matrix(_residual(model, A, m)))
        except ZeroDivisionError:
            return m, mpf(1)
        m = [m[e] - d[e] for e in range(9)]
        last = max(abs(d[e]) for e in range(9))
        if last == 0:
            break
    return m, last


def certificate(model, A, m):
    return max(abs(g) for g in _residual(model, A, m))


def _solve_at(model, x1, x2, wh, dps):
    with mp.workdps(dps):
        q1, d = condition(_mpf_rows(x1), wh)
        q2, _ = condition(_mpf_rows(x2), wh)
        A = rows(model, q1, q2)
        step_tol = mpf(10) ** (8 - dps)
        sols = []
        if model == "H":
            m, last = _newton(model, A, _unit_sign(nullspace(A, 1)[0]), 3)
            cands = [(m, last, None)]
            sep, nreal = mpf(1), 1
        else:
            a, b = nullspace(A, 2)
            co = pencil_cubic(a, b)
            if abs(co[3]) < mpf(10) ** (-dps // 2):
                raise NotCertified("the pencil's cubic has no leading coefficient")
            roots = mp.polyroots(list(reversed(co)), maxsteps=400, extraprec=4 * dps)
            sep = min(chordal(roots[i], roots[j]) for i in range(3) for j in range(i))
            real_tol = mpf(10) ** (-dps // 3)
            xs = sorted(mp.re(r) for r in roots if abs(mp.im(r)) <= real_tol * (1 + abs(mp.re(r))))
            nreal = len(xs)
            cands = []
            for x in xs:
                m, last = _newton(model, A, _unit_sign([a[e] + x * b[e] for e in range(9)]), 4)
                cands.append((m, last, x))
        for m, last, x in cands:
            if last > step_tol:
                raise NotCertified("the model does not settle at %d digits (last step %s)" % (dps, mp.nstr(last, 3)))
            m = _unit_sign(m)
            cert = certificate(model, A, m)
            if cert > CERT_TOL:
                raise NotCertified("certificate %s at %d digits" % (mp.nstr(cert, 3), dps))
            sols.append(dict(M=m, x=x, cert=cert))
        for i in range(len(sols)):
            for j in range(i):
                if max(abs(p - q) for p, q in zip(sols[i]["M"], sols[j]["M"])) < mpf(10) ** -30:
                    raise NotCertified("two roots polished onto one model")
        sols.sort(key=lambda s: tuple(s["M"]))              # (the roots' own order belongs to the basis the SVD happened to return)
        return dict(sols=sols, rho=sep, nreal=nreal, dps=dps, d=d)


def solve(model, x1, x2, wh, dps=DPS):
    """All models of a seven-point ('F') or four-point ('H') sample given in pixels: dict(sols=[dict(M (9 mpf, unit norm, largest entry
    positive, conditioned coordinates), x, cert)], rho, nreal, dps) at the first precision dps, 2 dps, ... <= MAX_DPS at which every
    solution certifies itself."""
    err = None
    while dps <= MAX_DPS:
        try:
            return _solve_at(model, x1, x2, wh, dps)
        except (NotCertified, mp.NoConvergence) as e:
            err = e
            dps *= 2
    raise NotCertified("never certified: %s" % err)


def _sensitivity_of(residual, jacobian, m, x1, x2, build):
    """sum_j |dM_k / dx_j| by central differences: `build(x1, x2)` -> the data the residual needs."""
    n = len(m)
    Jm = jacobian(build(x1, x2), m)
    Ji = Jm ** -1 if Jm.rows == Jm.cols else (Jm.T * Jm) ** -1 * Jm.T    # (16 consistent equations on 9 entries for 'E')
    J = [mpf(0)] * n
    for side in (0, 1):
        for p in range(len(x1)):
            for c in (0, 1):
                pm = []
                for sign in (1, -1):
                    xa = [list(r) for r in x1]
                    xb = [list(r) for r in x2]
                    (xa if side == 0 else xb)[p][c] += sign * DIFF_STEP
                    data = build(xa, xb)
                    v = list(m)
                    for _ in range(12):         # (a chord step gains the digits of step / separation^2: two steps on ordinary data)
                        dlt = Ji * mp.matrix(residual(data, v))
                        v = [v[e] - dlt[e] for e in range(n)]
                        if max(abs(dlt[e]) for e in range(n)) <= mpf(10) ** -40:
                            break
                    if max(abs(dlt[e]) for e in range(n)) > mpf(10) ** -40:
                        raise NotCertified("the perturbed model does not settle")
                    pm.append(v)
                for k in range(n):
                    J[k] += abs(pm[0][k] - pm[1][k]) / (2 * DIFF_STEP)
    return J


def calibrate(x, K):
    """[(xn, yn)] = K^-1 (u, v, 1) for an upper-triangular K with K[2][2] = 1."""
    fx, sk, cx, fy, cy = (mpf(float(K[0][0])), mpf(float(K[0][1])), mpf(float(K[0][2])), mpf(float(K[1][1])), mpf(float(K[1][2])))
    out = []
    for p in x:
        yn = (mpf(p[1]) - cy) / fy
        out.append([(mpf(p[0]) - cx - sk * yn) / fx, yn])
    return out


def _normalise(model, x, cam):
    """cam: the image size (w, h) for 'F' and 'H', the calibration matrix for 'E'."""
    return calibrate(x, cam) if model == "E" else condition(x, cam)[0]


def sensitivity(model, x1, x2, cam, sol, dps=DPS):
    """J (9 mpf): sum over the sample's pixel coordinates of |dM_k / dx_j|, M the unit-norm model."""
    with mp.workdps(max(dps, DPS)):
        def build(xa, xb):
            return rows(model, _normalise(model, xa, cam), _normalise(model, xb, cam))
        return _sensitivity_of(lambda A, v: _residual(model, A, v), lambda A, v: _jacobian(model, A, v), list(sol["M"]),
                               _mpf_rows(x1), _mpf_rows(x2), build)


def _svd3(m):
    U, S, V = mp.svd_r(mp.matrix([m[0:3], m[3:6], m[6:9]]), full_matrices=True, compute_uv=True)
    return U, [S[i] for i in range(3)], V


def _rebuild(U, s, V):
    return [sum(U[i, k] * s[k] * V[k, j] for k in range(3)) for i in range(3) for j in range(3)]


def nearest_rank2(m):
    """The nearest matrix of rank 2 (smallest singular value zeroed), and the ratio of the zeroed value to the largest."""
    U, s, V = _svd3(m)
    k = min(range(3), key=lambda i: s[i])
    ratio = s[k] / max(s) if max(s) else mpf(0)
    return _rebuild(U, [mpf(0) if i == k else s[i] for i in range(3)], V), ratio


def nearest_essential(m):
    """The nearest essential matrix: singular values (s, s, 0), s the mean of the two largest."""
    U, s, V = _svd3(m)
    order = sorted(range(3), key=lambda i: -s[i])
    mean = (s[order[0]] + s[order[1]]) / 2
    t = [mpf(0)] * 3
    t[order[0]] = t[order[1]] = mean
    return _rebuild(U, t, V)


def _line_error(F, q1, q2):
    """Worst over the sample of the smaller of dist(x2, F x1) and dist(x1, F^T x2)."""
    worst = mpf(0)
    for (u1, v1), (u2, v2) in zip(q1, q2):
        l2 = [F[0] * u1 + F[1] * v1 + F[2], F[3] * u1 + F[4] * v1 + F[5], F[6] * u1 + F[7] * v1 + F[8]]
        l1 = [F[0] * u2 + F[3] * v2 + F[6], F[1] * u2 + F[4] * v2 + F[7], F[2] * u2 + F[5] * v2 + F[8]]
        r = abs(l2[0] * u2 + l2[1] * v2 + l2[2])
        n2, n1 = mp.sqrt(l2[0] ** 2 + l2[1] ** 2), mp.sqrt(l1[0] ** 2 + l1[1] ** 2)
        if n1 == 0 and n2 == 0:
            return mp.inf
        worst = max(worst, r / max(n1, n2))
    return worst


def backward_error(model, M, x1, x2, wh):
    """Backward error in pixels (float) of the FLOAT model M (9, conditioned coordinates, any scale) on its own sample (pixels).
    'F': M' = M with its smallest singular value zeroed at 60 digits; per correspondence the smaller of the distances x2 -- M' x1 and
    x1 -- M'^T x2; moving one point of each pair by that much makes M' the exact answer.  'H': |x2 - M x1|.  Worst of the sample,
    divided by the conditioning scale.  'E' (wh is then the calibration matrix K of both cameras, M in calibrated coordinates): M' the
    nearest essential matrix, the same line distances under K^-T M' K^-1, in pixels."""
    with mp.workdps(DPS):
        m = [mpf(float(e)) for e in M]
        if model == "E":
            Ki = mp.matrix([[mpf(float(e)) for e in r] for r in wh]) ** -1
            E = nearest_essential(m)
            F = Ki.T * mp.matrix([E[0:3], E[3:6], E[6:9]]) * Ki
            return float(_line_error([F[i, j] for i in range(3) for j in range(3)], _mpf_rows(x1), _mpf_rows(x2)))
        q1, d = condition(_mpf_rows(x1), wh)
        q2, _ = condition(_mpf_rows(x2), wh)
        if model == "F":
            return float(_line_error(nearest_rank2(m)[0], q1, q2) / d)
        worst = mpf(0)
        for (u1, v1), (u2, v2) in zip(q1, q2):
            w = m[6] * u1 + m[7] * v1 + m[8]
            if w == 0:
                return float("inf")
            worst = max(worst, mp.sqrt(((m[0] * u1 + m[1] * v1 + m[2]) / w - u2) ** 2 + ((m[3] * u1 + m[4] * v1 + m[5]) / w - v2) ** 2))
        return float(worst / d)


def sigma_ratio(M):
    """Smallest over largest singular value of a FLOAT 3 x 3 model, at 60 digits."""
    with mp.workdps(DPS):
        return float(nearest_rank2([mpf(float(e)) for e in M])[1])


def recertify(model, x1, x2, cam, M_hi, steps=2):
    """(hi (9 floats), lo (9 floats), certificate): the fixture keeps a reference solution as nine float64 (float32 for 'E'); Newton steps
    on the full system at 60 digits bring it back to the certified one (a float64 start is 1e-16 away: 1e-32, then 1e-64 over the
    root separation; a float32 start 6e-8: four steps).  The generator checks, per solution, that they do."""
    with mp.workdps(DPS):
        A = rows(model, _normalise(model, _mpf_rows(x1), cam), _normalise(model, _mpf_rows(x2), cam))
        m, _ = _newton(model, A, [mpf(float(e)) for e in M_hi], steps)
        hi, lo = hi_lo(m)
        return hi, lo, certificate(model, A, m)


def hi_lo(vals):
    """float64 pairs (hi, lo) with hi + lo = the value to 2^-106."""
    with mp.workdps(DPS):
        hi = [float(v) for v in vals]
        lo = [float(v - mpf(h)) for v, h in zip(vals, hi)]
    return hi, lo


# ---- five points ----------------------------------------------------------------------------------------------------------------
_CUBIC = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
_BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _qmul(a, b):
    out = {}
    for ka, va in a.items():
        for kb, vb in b.items():
            k = (ka[0] + kb[0], ka[1] + kb[1], ka[2] + kb[2])
            out[k] = out.get(k, mpf(0)) + va * vb
    return out


def _qadd(*terms):
    """sum of (scalar, polynomial) pairs"""
    out = {}
    for sc, p in terms:
        for k, v in p.items():
            out[k] = out.get(k, mpf(0)) + sc * v
    return out


def _qeval(p, v):
    return sum(c * v[0] ** k[0] * v[1] ** k[1] * v[2] ** k[2] for k, c in p.items())


def _qdiff(p, axis):
    out = {}
    for k, c in p.items():
        if k[axis]:
            kk = list(k); kk[axis] -= 1
            out[tuple(kk)] = out.get(tuple(kk), mpf(0)) + k[axis] * c
    return out


def five_constraints(N):
    """The ten cubics in (x, y, z) that E = x N0 + y N1 + z N2 + N3 must meet: det E and the nine entries of 2 E E^T E - tr(E E^T) E."""
    E = [{(1, 0, 0): N[0][e], (0, 1, 0): N[1][e], (0, 0, 1): N[2][e], (0, 0, 0): N[3][e]} for e in range(9)]
    m = lambda p, q: _qmul(E[p], E[q])
    det = _qadd((1, _qmul(E[0], _qadd((1, m(4, 8)), (-1, m(5, 7))))), (-1, _qmul(E[1], _qadd((1, m(3, 8)), (-1, m(5, 6))))),
                (1, _qmul(E[2], _qadd((1, m(3, 7)), (-1, m(4, 6))))))
    EEt = [[_qadd(*[(1, m(3 * i + k, 3 * j + k)) for k in range(3)]) for j in range(3)] for i in range(3)]
    tr = _qadd((1, EEt[0][0]), (1, EEt[1][1]), (1, EEt[2][2]))
    out = [det]
    for i in range(3):
        for j in range(3):
            out.append(_qadd(*([(2, _qmul(EEt[i][k], E[3 * k + j])) for k in range(3)] + [(-1, _qmul(tr, E[3 * i + j]))])))
    return out


def action_matrix(polys):
    """Multiplication by x on the quotient ring's basis x^2, xy, xz, y^2, yz, z^2, x, y, z, 1: the ten cubics are eliminated (Gauss-Jordan
    on the 10 x 20 coefficient matrix, cubic monomials first) so that every cubic monomial is a combination of the basis."""
    A1 = mp.matrix([[p.get(k, mpf(0)) for k in _CUBIC] for p in polys])
    A2 = mp.matrix([[p.get(k, mpf(0)) for k in _BASIS] for p in polys])
    C = (A1 ** -1) * A2
    M = mp.matrix(10, 10)
    for i in range(6):                          # x * basis_i is the cubic monomial i: x^3, x^2 y, x^2 z, x y^2, x y z, x z^2
        for j in range(10):
            M[i, j] = -C[i, j]
    M[6, 0] = M[7, 1] = M[8, 2] = M[9, 6] = 1   # x * x = x^2, x * y = xy, x * z = xz, x * 1 = x
    return M


def _five_at(x1, x2, K, dps):
    with mp.workdps(dps):
        A = rows("E", calibrate(_mpf_rows(x1), K), calibrate(_mpf_rows(x2), K))
        N = nullspace(A, 4)
        polys = five_constraints(N)
        grads = [[_qdiff(p, ax) for ax in range(3)] for p in polys]
        ev, ER = mp.eig(action_matrix(polys))
        real_tol = mpf(10) ** (-dps // 3)
        step_tol = mpf(10) ** (8 - dps)
        sols = []
        for c in range(10):
            if abs(ER[9, c]) == 0:
                continue
            v = [ER[6 + k, c] / ER[9, c] for k in range(3)]
            if any(abs(mp.im(e)) > real_tol * (1 + abs(e)) for e in v):
                continue
            v = [mp.re(e) for e in v]
            last = mpf(1)
            for _ in range(8):                  # Gauss-Newton on the ten cubics in (x, y, z): they all vanish at a solution
                g = mp.matrix([_qeval(p, v) for p in polys])
                Jm = mp.matrix([[_qeval(d, v) for d in gr] for gr in grads])
                dlt = mp.lu_solve(Jm.T * Jm, Jm.T * g)
                v = [v[k] - dlt[k] for k in range(3)]
                last = max(abs(dlt[k]) for k in range(3))
                if last == 0:
                    break
            if last > step_tol * (1 + max(abs(e) for e in v)):
                raise NotCertified("a five-point root does not settle at %d digits" % dps)
            m = _unit_sign([v[0] * N[0][e] + v[1] * N[1][e] + v[2] * N[2][e] + N[3][e] for e in range(9)])
            cert = certificate("E", A, m)
            if cert > CERT_TOL:
                raise NotCertified("certificate %s at %d digits" % (mp.nstr(cert, 3), dps))
            if any(max(abs(p - q) for p, q in zip(m, s["M"])) < mpf(10) ** -30 for s in sols):
                raise NotCertified("two roots polished onto one model")
            sols.append(dict(M=m, x=v, cert=cert))
        sols.sort(key=lambda s: tuple(s["M"]))
        return dict(sols=sols, rho=mpf(1), nreal=len(sols), dps=dps)


def solve_five(x1, x2, K, dps=DPS):
    """All essential matrices of a five-point sample given in pixels and K (both cameras): dict(sols=[dict(M (9 mpf, unit norm, largest
    entry positive, calibrated coordinates), x, cert)], nreal, dps), every solution certified: the five equations, det = 0 and
    2 E E^T E - tr(E E^T) E = 0 to 1e-50."""
    err = None
    while dps <= MAX_DPS:
        try:
            return _five_at(x1, x2, K, dps)
        except (NotCertified, mp.NoConvergence, ZeroDivisionError) as e:
            err = e
            dps *= 2
    raise NotCertified("never certified: %s" % err)

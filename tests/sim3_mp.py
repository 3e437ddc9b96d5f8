"""50-digit reference of the 3-D similarity (mpmath, mp.dps = 50), stated without any of the product's formulas or orders of operation:

  minimal(x3, y3)   the similarity of three correspondences as coloc_amd/csrc/sim3_math.h defines it: the rotation that carries the frame
                    of the new triangle (first edge, its normal) onto the old triangle's, s = sqrt(S_y / S_x) with S the triangle's
                    moment about its centroid, t from the centroids.  The frame is built here by classical Gram-Schmidt on the two
                    EDGES (the product normalises the first edge and the normal): the same frame in exact arithmetic.
  umeyama(x, y)     S. Umeyama, "Least-squares estimation of transformation parameters between two point patterns", PAMI 1991: the SVD of
                    the cross-covariance by mpmath's own routine, R = U diag(1, 1, det U det V) V^T, s = tr(D S) / var_x, t = ybar - s R xbar.
  sine / spread     the conditioning of a case: the triangle's sine (|e1 x e2| / (|e1| |e2|), the smaller of the two clouds') and
                    (sigma2 + sigma3) / sigma1 of the cross-covariance.
  forward_error     of a computed (s, R, t) against the reference: max of |s - s*| / s*, max |R - R*| and max |t - t*| / (|ybar| + s* |xbar| + L),
                    L the old cloud's extent -- t is a difference of the two centroid terms and cannot be asked for more.
Plain lists of mpf."""
from mpmath import mp, mpf, matrix

mp.dps = 50


def _v(a):
    return [mpf(float(c)) for c in a]


def _sub(a, b):
    return [a[i] - b[i] for i in range(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(a):
    return mp.sqrt(_dot(a, a))


def _frame(p):
    e1, e2 = _sub(p[1], p[0]), _sub(p[2], p[0])
    u1 = [c / _norm(e1) for c in e1]
    w = [e2[i] - _dot(e2, u1) * u1[i] for i in range(3)]
    u2 = [c / _norm(w) for c in w]
    return u1, u2, _cross(u1, u2)


def _mean(p):
    n = len(p)
    return [sum(q[i] for q in p) / n for i in range(3)]


def _moment(p, c):
    return sum(_dot(_sub(q, c), _sub(q, c)) for q in p)


def sine(p3):
    p = [_v(q) for q in p3]
    e1, e2 = _sub(p[1], p[0]), _sub(p[2], p[0])
    if _norm(e1) == 0 or _norm(e2) == 0:
        return mpf(0)
    return _norm(_cross(e1, e2)) / (_norm(e1) * _norm(e2))


def minimal(x3, y3):
    """-> (s, R (3 x 3 nested), t)"""
    x, y = [_v(q) for q in x3], [_v(q) for q in y3]
    fx, fy = _frame(x), _frame(y)
    R = [[sum(fy[k][i] * fx[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    cx, cy = _mean(x), _mean(y)
    s = mp.sqrt(_moment(y, cy) / _moment(x, cx))
    t = [cy[i] - s * sum(R[i][j] * cx[j] for j in range(3)) for i in range(3)]
    return s, R, t


def _cov(x, y):
    n = len(x)
    cx, cy = _mean(x), _mean(y)
    S = matrix(3, 3)
    for a, b in zip(x, y):
        dx, dy = _sub(a, cx), _sub(b, cy)
        for i in range(3):
            for j in range(3):
                S[i, j] += dy[i] * dx[j] / n
    return S, cx, cy, _moment(x, cx) / n


def spread(x, y):
    """(sigma2 + sigma3) / sigma1 of the cross-covariance"""
    S, _, _, _ = _cov([_v(q) for q in x], [_v(q) for q in y])
    sg = sorted([mp.re(v) for v in mp.svd_r(S, compute_uv=False)], reverse=True)
    return (sg[1] + sg[2]) / sg[0]


def umeyama(x, y):
    """-> (s, R, t, d)"""
    x, y = [_v(q) for q in x], [_v(q) for q in y]
    S, cx, cy, var_x = _cov(x, y)
    U, sg, Vt = mp.svd_r(S)
    d = mpf(1) if mp.det(U) * mp.det(Vt) > 0 else mpf(-1)
    D = matrix(3, 3)
    D[0, 0] = D[1, 1] = mpf(1)
    D[2, 2] = d
    Rm = U * D * Vt
    s = (sg[0] + sg[1] + d * sg[2]) / var_x
    R = [[Rm[i, j] for j in range(3)] for i in range(3)]
    t = [cy[i] - s * sum(R[i][j] * cx[j] for j in range(3)) for i in range(3)]
    return s, R, t, int(d)


def forward_error(got, ref, x, y):
    """got = (s, R (3 x 3 array), t) in doubles, ref = (s, R, t) in mpf, x / y the clouds the model came from -> float"""
    s, R, t = got
    rs, rR, rt = ref[0], ref[1], ref[2]
    xs, ys = [_v(q) for q in x], [_v(q) for q in y]
    cx, cy = _mean(xs), _mean(ys)
    L = max(_norm(_sub(q, cy)) for q in ys)
    e_s = abs(mpf(float(s)) - rs) / rs
    e_R = max(abs(mpf(float(R[i][j])) - rR[i][j]) for i in range(3) for j in range(3))
    e_t = max(abs(mpf(float(t[i])) - rt[i]) for i in range(3)) / (_norm(cy) + rs * _norm(cx) + L)
    return float(max(e_s, e_R, e_t))

"""Independent numpy minimal solvers used by the tests as cross-checks (never by the product)."""
import numpy as np


def _bearings(xs, K):
    f = (np.linalg.inv(K) @ np.concatenate([xs, np.ones((3, 1))], 1).T).T
    return f / np.linalg.norm(f, axis=1, keepdims=True)


def _newton_depths(s, Xs, f, steps):
    """Newton (np.linalg.solve) on the law of cosines of the three point pairs in the depths s."""
    d2 = [((Xs[0] - Xs[1]) ** 2).sum(), ((Xs[0] - Xs[2]) ** 2).sum(), ((Xs[1] - Xs[2]) ** 2).sum()]
    pairs = [(0, 1), (0, 2), (1, 2)]
    s = np.array(s, dtype=np.float64)
    for _ in range(steps):
        g = np.zeros(3); Jm = np.zeros((3, 3))
        for r, (i, j) in enumerate(pairs):
            c = f[i] @ f[j]
            g[r] = s[i] * s[i] + s[j] * s[j] - 2.0 * s[i] * s[j] * c - d2[r]
            Jm[r, i] = 2.0 * (s[i] - s[j] * c); Jm[r, j] = 2.0 * (s[j] - s[i] * c)
        s = s - np.linalg.solve(Jm, g)
    return s


def _kabsch(Xs, Q):
    mx, mq = Xs.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - mq).T @ (Xs - mx))
    R = U @ np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    return np.concatenate([R, (mq - R @ mx)[:, None]], 1)


def numpy_p3p_sensitivity(Xs, xs, K, pose, h=1e-3):
    """J (12,): sum over the six pixel inputs of |dP_k / dx_j| at the solution `pose` (3 x 4), by central differences with step h px;
    the perturbed solution is followed by Newton on the depths from the unperturbed ones (no root matching).  Float64: the rounding of
    a difference is 2^-53 |P| / h, about 1e-12 at h = 1e-3, against J of 1e-4 and more."""
    s0 = np.linalg.norm(Xs @ pose[:, :3].T + pose[:, 3], axis=1)
    J = np.zeros(12)
    for j in range(6):
        P2 = []
        for sign in (1.0, -1.0):
            xp = np.array(xs, dtype=np.float64); xp.flat[j] += sign * h
            f = _bearings(xp, K)
            P2.append(_kabsch(Xs, _newton_depths(s0, Xs, f, 3)[:, None] * f))
        J += np.abs(P2[0] - P2[1]).reshape(-1) / (2.0 * h)
    return J


def numpy_p3p(Xs, xs, K, polish=False):
    """Independent minimal solver for the test: same distance formulation, but the quartic is solved by
    numpy's companion-matrix eigenvalues and the rigid transform by Kabsch/SVD.  polish: three Newton steps on the law of cosines in
    the depths before the transform (the companion roots alone leave the pose up to 1e-5 off on ordinary data).  The polish is the
    same method as p3p.h's p3p_polish_depths, in numpy's own arithmetic (np.linalg.solve): with it the forward comparison in
    test_gpu_pnp.py is independent in the quartic, the root finder and the transform, not in the polish; what is independent of the
    product altogether is that test's backward assertion and the mpmath reference of tests/p3p_mp.py."""
    f = _bearings(xs, K)
    a2 = ((Xs[1] - Xs[2]) ** 2).sum(); b2 = ((Xs[0] - Xs[2]) ** 2).sum(); c2 = ((Xs[0] - Xs[1]) ** 2).sum()
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    q = (a2 - c2) / b2
    P = np.polynomial.polynomial
    Np = np.array([q + 1, -2 * q * cb, q - 1]); D = np.array([2 * cg, -2 * ca]); W = np.array([1, -2 * cb, 1.0])
    DD = P.polymul(D, D)
    poly = b2 * P.polyadd(P.polyadd(DD, P.polymul(Np, Np)), -2 * cg * P.polymul(Np, D))
    poly = P.polysub(poly, c2 * P.polymul(DD, W))
    sols = []
    for v in P.polyroots(poly):
        if abs(v.imag) > 1e-9 or v.real <= 0:
            continue
        v = v.real
        u = P.polyval(v, Np) / P.polyval(v, D)
        w = P.polyval(v, W)
        if u <= 0 or w <= 0:
            continue
        s1 = np.sqrt(b2 / w)
        s = np.array([s1, u * s1, v * s1])
        if polish:
            s = _newton_depths(s, Xs, f, 3)
        sols.append(_kabsch(Xs, s[:, None] * f))
    return sols


def undistort_k3(x, K, k, eps=1e-10):
    """OpenMVG Pinhole_Intrinsic_Radial_K3::get_ud_pixel: bisection on r^2 (1 + k1 r^2 + k2 r^4 + k3 r^6)^2."""
    f, pp = K[0, 0], np.array([K[0, 2], K[1, 2]])
    out = np.zeros_like(x, dtype=np.float64)

    def functor(r2):
        t = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
        return r2 * t * t

    for i, p in enumerate(x):
        c = (p - pp) / f
        r2 = float(c @ c)
        if r2 == 0.0:
            out[i] = p
            continue
        lo = hi = r2
        while functor(lo) > r2:
            lo /= 1.05
        while functor(hi) < r2:
            hi *= 1.05
        while eps < hi - lo:
            mid = 0.5 * (lo + hi)
            if functor(mid) > r2:
                hi = mid
            else:
                lo = mid
        out[i] = c * np.sqrt(0.5 * (lo + hi) / r2) * f + pp
    return out

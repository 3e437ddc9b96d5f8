"""CPU tests of the 50-digit pose reference (tests/pose_mp.py) and of the oracle's PnP residuals / scores against it.

The GPU tests hold the residual and score kernels to the oracle bit for bit (tests/test_gpu_pnp.py, tests/test_gpu_pose_edges.py);
here the oracle itself is held to the reference on cameras with skew, fx != fy, an off-centre principal point and a scaled K (the
residuals apply all nine entries of K), on rotations up to a half turn and on points behind the camera.

Bound on a squared error (derived, not fitted): err = du^2 + dv^2 with du = obs - u / w, about 25 rounded operations in all; the
projection u / w carries a relative error of a few ulp, so du is off by k 2^-53 max(|obs|, |proj|) ABSOLUTELY (the difference
cancels), and err by 2 sqrt(err) times that plus its own relative rounding:
    |err - err_ref| <= 64 * 2^-53 * (2 sqrt(err_ref) max(|obs|, |proj|)_inf + err_ref),
for points that are not next to the principal plane (|w| >= 1e-3 ||K Xc||_inf, asserted for every compared point).
"""
import numpy as np
from mpmath import mp, mpf

import pose_mp as pm

EPS = 2.0 ** -53

KS = {
    "suite": np.array([[1000.0, 0, 320], [0, 1000, 240], [0, 0, 1]]),
    "fx900_fy1100": np.array([[900.0, 0, 320], [0, 1100, 240], [0, 0, 1]]),
    "skew3.5": np.array([[1000.0, 3.5, 320], [0, 1000, 240], [0, 0, 1]]),
    "skew-40_aniso": np.array([[900.0, -40, 320], [0, 1100, 240], [0, 0, 1]]),
    "pp_100_650": np.array([[1000.0, 0, 100], [0, 1000, 650], [0, 0, 1]]),
    "scaled_2K": 2.0 * np.array([[900.0, -40, 320], [0, 1100, 240], [0, 0, 1]]),
    "full_last_row": np.array([[900.0, -40, 320], [1e-3, 1100, 240], [1e-4, -2e-4, 1.5]]),
}


def test_log_inverts_exp_at_50_digits():
    rng = np.random.default_rng(1)
    pi = mp.pi
    for ang in [mpf(0), mpf(10) ** -30, mpf(10) ** -12, mpf(10) ** -9, mpf(10) ** -8, mpf(10) ** -6, mpf(1), mpf(3), pi - mpf(10) ** -3,
                pi - mpf(10) ** -6, pi - mpf(10) ** -9, pi]:
        for ax in [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), np.array([1.0, -1, 0]), np.array([0, 1.0, -1]),
                   np.array([-1.0, -1, -1])] + list(rng.standard_normal((6, 3))):
            k = pm.vec(ax)
            n = mp.sqrt(sum(v * v for v in k))
            w = [ang * v / n for v in k]
            back = pm.log_so3(pm.exp_so3(w))
            d = max(abs(a - b) for a, b in zip(back, w))
            if ang == pi:                      # both signs of the axis are logarithms of a half turn
                d = min(d, max(abs(a + b) for a, b in zip(back, w)))
            assert d < mpf(10) ** -40, (float(ang), ax, float(d))
            R = pm.exp_so3(w)                  # and exp gives a rotation: R R^T = I
            RRt = [[sum(R[i][m] * R[j][m] for m in range(3)) - int(i == j) for j in range(3)] for i in range(3)]
            assert max(abs(v) for row in RRt for v in row) < mpf(10) ** -45


def _scene(n, seed, K, w_true, t_true=(0.1, -0.2, 0.3), noise=0.5):
    """n points 4 - 20 units in front of the camera [exp(w_true) | t_true], observed with Gaussian pixel noise."""
    rng = np.random.default_rng(seed)
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 20, n)], 1)
    R = pm.to_float(pm.exp_so3(w_true))
    t = np.array(t_true)
    X = (Xc - t) @ R                                         # R^T (Xc - t)
    uvw = (X @ R.T + t) @ K.T
    x = uvw[:, :2] / uvw[:, 2:3] + noise * rng.standard_normal((n, 2))
    return X, x, np.concatenate([w_true, t])


def test_gradient_and_jacobian_of_the_reference_agree_with_differences_of_its_cost():
    K = KS["skew-40_aniso"]
    for w_true, a in ((np.array([0.3, -2.0, 1.4]), 16.0), (np.zeros(3), 2.0)):
        X, x, p = _scene(12, 3, K, w_true)
        x[:3] += 60.0                                       # three points in the Huber tail
        p = p + np.array([1e-3, -2e-3, 1e-3, 2e-3, 1e-3, -1e-3])
        A, g, cost = pm.normal_equations(p, X, x, K, a)
        assert abs(cost - pm.huber_cost(p, X, x, K, a)) < mpf(10) ** -40
        h = mpf(10) ** -15
        for k in range(6):
            pp = pm.vec(p); pq = pm.vec(p)
            pp[k] += h; pq[k] -= h
            dc = (pm.huber_cost(pp, X, x, K, a) - pm.huber_cost(pq, X, x, K, a)) / (2 * h)
            assert abs(dc + g[k]) < mpf(10) ** -25 * (1 + abs(dc))       # g is the DESCENT right-hand side: -grad
        # chain-rule Jacobian == Jacobian of the whole projection, both by differences
        Xi = X[5]
        Jd = pm.jacobian_direct(p, Xi, K)
        A1, _, _ = pm.normal_equations(p, X[5:6], x[5:6], K, 1e9)
        for i in range(6):
            for j in range(6):
                assert abs(A1[i, j] - (Jd[0][i] * Jd[0][j] + Jd[1][i] * Jd[1][j])) < mpf(10) ** -25 * (1 + abs(A1[i, j]))


def test_newton_polish_finds_the_stationary_point():
    K = KS["skew3.5"]
    X, x, p = _scene(40, 4, K, np.array([0.0, 2.5, 0.0]))
    q, steps = pm.newton_polish(p + 1e-3, X, x, K)
    d, _, g, _ = pm.newton_step(q, X, x, K)
    assert steps >= 1 and max(abs(v) for v in d) < mpf(10) ** -30
    assert pm.huber_cost(q, X, x, K) <= pm.huber_cost(p, X, x, K)


def _hypotheses(p_true, seed, n):
    """n poses [R|t] (flat 12) near the true one, rounded to float64."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q = p_true + np.concatenate([0.02 * rng.standard_normal(3), 0.05 * rng.standard_normal(3)])
        out.append(np.concatenate([pm.to_float(pm.exp_so3(q[:3])), q[3:, None]], 1).reshape(12))
    return np.array(out)


def _check_against_reference(oracle, Rt, X, x, K, thr2):
    """err of the oracle within the derived bound of the 50-digit value; count == the reference's.  Returns the worst error / bound."""
    err = oracle.pnp_residuals(Rt, X, x, K)
    cnt, _ = oracle.pnp_score(err, thr2)
    Km = pm.mat3(K)
    worst = 0.0
    for h in range(len(Rt)):
        P = Rt[h].reshape(3, 4)
        R, t = pm.mat3(P[:, :3]), pm.vec(P[:, 3])
        n_in = 0
        for i in range(len(X)):
            Xc = pm.cam_point(R, t, pm.vec(X[i]))
            KX = [sum(Km[r][c] * Xc[c] for c in range(3)) for r in range(3)]
            if KX[2] == 0:
                assert not np.isfinite(err[h, i])           # on the principal plane: inf or NaN, never a number
                continue
            assert abs(KX[2]) >= mpf(10) ** -3 * max(abs(v) for v in KX), "case construction: point next to the principal plane"
            u, v = KX[0] / KX[2], KX[1] / KX[2]
            e_ref = (mpf(float(x[i, 0])) - u) ** 2 + (mpf(float(x[i, 1])) - v) ** 2
            big = max(abs(float(x[i, 0])), abs(float(x[i, 1])), abs(float(u)), abs(float(v)))
            bound = 64 * EPS * (2 * mp.sqrt(e_ref) * big + e_ref)
            assert np.isfinite(err[h, i])
            diff = abs(mpf(float(err[h, i])) - e_ref)
            assert diff <= bound, (h, i, float(diff), float(bound))
            if bound > 0:
                worst = max(worst, float(diff / bound))
            assert abs(e_ref - thr2) > mpf(10) ** -9 * thr2, "case construction: an error next to the threshold"
            n_in += 1 if e_ref < thr2 else 0
        assert cnt[h] == n_in, (h, int(cnt[h]), n_in)
    return worst


def test_oracle_residuals_and_counts_against_the_reference(oracle):
    rots = [np.zeros(3), np.array([1e-8, 0, 0]), 2.5 * np.array([0.6, -0.48, 0.64]), (np.pi - 1e-6) * np.array([0.0, 0.6, 0.8]),
            np.pi * np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)]
    for ki, (kname, K) in enumerate(sorted(KS.items())):
        for ri, w_true in enumerate(rots):
            X, x, p = _scene(24, 100 * ki + ri, K / K[2, 2] if kname == "scaled_2K" else K, w_true)
            if kname == "full_last_row":                   # observations of THIS camera (a homography of the pixel plane)
                uvw = (X @ pm.to_float(pm.exp_so3(w_true)).T + p[3:]) @ K.T
                x = uvw[:, :2] / uvw[:, 2:3] + 0.5
            Rt = _hypotheses(p, 7 + ri, 3)
            worst = _check_against_reference(oracle, Rt, X, x, K, 16.0)
            print("oracle vs reference %-14s rotation %d: worst |err - ref| / bound = %.3f" % (kname, ri, worst))
            assert worst <= 1.0


def test_oracle_behind_the_camera_and_on_the_principal_plane(oracle):
    """Negative depth gives an ordinary (large) error, never an inlier by accident; w == 0 gives inf / NaN, which is no inlier and
    costs thr2 in the score."""
    K = KS["skew-40_aniso"]
    X, x, p = _scene(40, 9, K, np.array([0.0, 0.0, 0.0]), t_true=(0.0, 0.0, 0.0))
    X[:4, 2] = -X[:4, 2]                                     # four points behind the camera (R = I, t = 0: depth = Z)
    Rt = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).reshape(1, 12)
    worst = _check_against_reference(oracle, Rt, X, x, K, 16.0)
    assert worst <= 1.0
    err = oracle.pnp_residuals(Rt, X, x, K)
    assert (err[0, :4] > 16.0).all()
    X[4] = [1.0, 2.0, 0.0]                                   # u / 0: inf
    X[5] = [0.0, 0.0, 0.0]                                   # 0 / 0: NaN
    err = oracle.pnp_residuals(Rt, X, x, K)
    assert np.isinf(err[0, 4]) and np.isnan(err[0, 5])
    _check_against_reference(oracle, Rt, X, x, K, 16.0)
    cnt, cost = oracle.pnp_score(err, 16.0)
    fin = np.isfinite(err[0])
    assert cnt[0] == (err[0][fin] < 16.0).sum()
    assert np.isclose(cost[0], np.minimum(err[0][fin], 16.0).sum() + 2 * 16.0, rtol=1e-13)

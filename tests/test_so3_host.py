"""The host build of coloc_amd/csrc/so3.h (the statements pnp_refine_kernel runs) against the 50-digit reference (tests/pose_mp.py).

Tolerance rule: nobody hands float64 a number here, so each row (one rotation angle, 56 axes) measures a YARDSTICK first -- a plain
numpy float64 statement of the well-conditioned formulas (logarithm: angle from atan2, axis from the antisymmetric part below 2 rad and
from the symmetric part above; Rodrigues and its derivative from the coefficient functions sin(th)/th, (1 - cos th)/th^2 and their
derivatives, Taylor series below 1e-4 resp. 0.5 rad) -- against the same 50-digit values, and the product must stay within
16 x max(yardstick, 2^-53) of that row (16: another operation order, libm against numpy; 2^-53: half an ulp of the entries of size 1,
which no float64 result can beat).  The yardstick never sees the product's output.

Measured (worst over the 56 axes; printed by the tests, run with -s).  Columns: max |exp(log R) - R|, max |exp(w) - exp_ref(w)|,
max |d exp(w) - reference| / max |reference|; left the numpy yardstick, right the host build of so3.h:

  angle        yardstick: log, exp, d exp       | so3.h: log, exp, d exp
  0            0.00e+00   0.00e+00   1.67e-41   | 0.00e+00   0.00e+00   1.67e-41
  1e-30        2.50e-61   2.50e-61   4.32e-32   | 2.50e-61   2.50e-61   4.32e-32
  1e-12        5.00e-25   5.00e-25   5.00e-25   | 5.00e-25   5.00e-25   5.00e-25
  1e-10        5.00e-21   5.00e-21   5.00e-21   | 5.00e-21   5.00e-21   5.00e-21
  1e-9         5.00e-19   5.00e-19   5.00e-19   | 5.00e-19   5.00e-19   5.00e-19
  1e-8         5.00e-17   5.00e-17   5.00e-17   | 5.00e-17   5.00e-17   5.00e-17
  1e-6         5.45e-17   5.45e-17   7.73e-17   | 5.45e-17   9.57e-17   7.73e-17
  1e-5         5.52e-17   5.52e-17   6.28e-17   | 5.52e-17   5.87e-17   6.28e-17
  1            2.07e-16   1.82e-16   3.49e-16   | 2.07e-16   1.98e-16   2.77e-16
  2.5          3.52e-16   4.57e-16   3.83e-16   | 4.92e-16   5.35e-16   8.27e-16
  3            4.80e-16   4.85e-16   4.80e-16   | 4.76e-16   6.95e-16   5.85e-16
  pi-1e-3      4.48e-16   6.95e-16   3.97e-16   | 5.11e-16   6.41e-16   4.57e-16
  pi-1e-5      4.31e-16   7.07e-16   4.57e-16   | 4.78e-16   8.29e-16   7.80e-16
  pi-1.1e-6    4.36e-16   5.32e-16   5.78e-16   | 5.33e-16   7.51e-16   4.55e-16
  pi-1e-6      4.30e-16   5.69e-16   3.88e-16   | 6.10e-16   6.81e-16   5.97e-16
  pi-1e-9      4.40e-16   6.26e-16   4.39e-16   | 4.69e-16   6.90e-16   6.17e-16
  pi           4.22e-16   6.31e-16   4.43e-16   | 5.03e-16   6.42e-16   4.67e-16
  exact half turns (integer matrices): 7.3e-17 .. 1.2e-16 both (the rounding of pi)

(Below 1e-8 rad the figures are th^2 / 2: the second-order term that the float64 matrix itself cannot hold; the floor 2^-53 governs.)
With the logarithm this header replaced (acos, axis signs from R - R^T next to pi, th / (2 sin th)) the rows from 3 rad upwards and the
half turns about (1,-1,0), (0,1,-1), (1,0,-1) fail: 180 degrees at the half turns, 0.14 degrees at pi - 1.1e-6.
"""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import pose_mp as pm
import so3_host

EPS = 2.0 ** -53
PI = math.pi
ANGLES = [("0", 0.0), ("1e-30", 1e-30), ("1e-12", 1e-12), ("1e-10", 1e-10), ("1e-9", 1e-9), ("1e-8", 1e-8), ("1e-6", 1e-6), ("1e-5", 1e-5),
          ("1", 1.0), ("2.5", 2.5), ("3", 3.0), ("pi-1e-3", PI - 1e-3), ("pi-1e-5", PI - 1e-5), ("pi-1.1e-6", PI - 1.1e-6),
          ("pi-1e-6", PI - 1e-6), ("pi-1e-9", PI - 1e-9), ("pi", PI)]


def axes():
    r2, r3 = math.sqrt(0.5), math.sqrt(1.0 / 3.0)
    named = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (r2, -r2, 0), (0, r2, -r2), (-r3, -r3, -r3)]
    rng = np.random.default_rng(20)
    rnd = rng.standard_normal((50, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    return [np.array(a, dtype=np.float64) for a in named] + list(rnd)


# ---- the yardstick: plain float64 numpy -----------------------------------------------------------------------------------------

def _skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)


def _series(x, first_n, n_terms):
    """sum_m (-1)^m x^m / (2 m + first_n)!"""
    return sum((-1.0) ** m * x ** m / math.factorial(2 * m + first_n) for m in range(n_terms))


def np_coeff(th2, small):
    th = math.sqrt(th2)
    if th < small:
        a = _series(th2, 1, 10); b = _series(th2, 2, 10)
        a1 = sum((-1.0) ** m * 2 * m * th2 ** (m - 1) / math.factorial(2 * m + 1) for m in range(1, 11))
        b1 = sum((-1.0) ** m * 2 * m * th2 ** (m - 1) / math.factorial(2 * m + 2) for m in range(1, 11))
        return a, b, a1, b1
    s, c = math.sin(th), math.cos(th)
    b = 2 * math.sin(th / 2) ** 2 / th2
    return s / th, b, (th * c - s) / th ** 3, (th * s - 2 * b * th2) / th ** 4


def np_exp(w):
    W = _skew(w)
    a, b, _, _ = np_coeff(float(w @ w), 1e-4)
    return np.eye(3) + a * W + b * (W @ W)


def np_dexp(w):
    W = _skew(w)
    a, b, a1, b1 = np_coeff(float(w @ w), 0.5)
    out = np.zeros((3, 3, 3))
    for k in range(3):
        e = np.zeros(3); e[k] = 1.0
        G = _skew(e)
        out[k] = a * G + a1 * w[k] * W + b * (G @ W + W @ G) + b1 * w[k] * (W @ W)
    return out


def np_log(R):
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.linalg.norm(a)
    c = 0.5 * (np.trace(R) - 1.0)
    th = math.atan2(s, c)
    if th < 2.0:
        return 0.5 * a if s == 0.0 else (th / (2.0 * s)) * a
    S = 0.5 * (R + R.T)
    p = int(np.argmax(np.diag(S)))
    kp = math.sqrt((S[p, p] - c) / (1.0 - c))
    k = S[p] / ((1.0 - c) * kp)
    k[p] = kp
    if k @ a < 0:
        k = -k
    return th * k


# ---- cases -----------------------------------------------------------------------------------------------------------------------

def _cases(angle):
    out = []
    for ax in axes():
        w = angle * ax
        Rm = pm.exp_so3(w)
        out.append((w, Rm, pm.to_float(Rm)))       # float64 angle-axis, its 50-digit rotation, that rotation rounded to float64
    return out


def _maxabs(A, Bm):
    """max |A - B|, A float64 array, B nested list of mpf: the difference is taken at 50 digits."""
    A = np.asarray(A)
    return float(max(abs(mpf(float(A[i, j])) - Bm[i][j]) for i in range(3) for j in range(3)))


def _tol(yard):
    return 16.0 * max(yard, EPS)


@pytest.mark.parametrize("name,angle", ANGLES)
def test_so3_against_the_50_digit_reference(name, angle):
    worst = dict(y_log=0.0, p_log=0.0, y_exp=0.0, p_exp=0.0, y_d=0.0, p_d=0.0, bit=True)
    for w, Rm, Rf in _cases(angle):
        # exp(log R) against R: the logarithm is judged by the rotation it stands for, at 50 digits
        worst["y_log"] = max(worst["y_log"], _maxabs(Rf, pm.exp_so3(np_log(Rf))))
        worst["p_log"] = max(worst["p_log"], _maxabs(Rf, pm.exp_so3(so3_host.log_so3(Rf))))
        worst["y_exp"] = max(worst["y_exp"], _maxabs(np_exp(w), Rm))
        worst["p_exp"] = max(worst["p_exp"], _maxabs(so3_host.rodrigues(w), Rm))
        dRm = pm.d_exp_so3(w)
        scale = float(max(abs(dRm[k][i][j]) for k in range(3) for i in range(3) for j in range(3)))
        yd, pd = np_dexp(w), so3_host.d_rodrigues(w)
        worst["y_d"] = max(worst["y_d"], max(_maxabs(yd[k], dRm[k]) for k in range(3)) / scale)
        worst["p_d"] = max(worst["p_d"], max(_maxabs(pd[k], dRm[k]) for k in range(3)) / scale)
        worst["bit"] = worst["bit"] and np.array_equal(pd, so3_host.d_rodrigues_entries(w))
    print("\nso3 %-10s yardstick: log %.2e exp %.2e d %.2e | product: log %.2e exp %.2e d %.2e (bound 16 x max(yardstick, 2^-53))"
          % (name, worst["y_log"], worst["y_exp"], worst["y_d"], worst["p_log"], worst["p_exp"], worst["p_d"]))
    assert worst["bit"], "d_rodrigues_entry differs from d_rodrigues"
    assert worst["p_log"] <= _tol(worst["y_log"])
    assert worst["p_exp"] <= _tol(worst["y_exp"])
    assert worst["p_d"] <= _tol(worst["y_d"])


HALF_TURNS = {"e1": np.diag([1.0, -1.0, -1.0]), "e2": np.diag([-1.0, 1.0, -1.0]), "e3": np.diag([-1.0, -1.0, 1.0]),
              "(1,-1,0)/sqrt2": np.array([[0.0, -1, 0], [-1, 0, 0], [0, 0, -1]]),
              "(0,1,-1)/sqrt2": np.array([[-1.0, 0, 0], [0, 0, -1], [0, -1, 0]]),
              "(1,1,0)/sqrt2": np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]]),
              "(1,0,-1)/sqrt2": np.array([[0.0, 0, -1], [0, -1, 0], [-1, 0, 0]])}


@pytest.mark.parametrize("name", sorted(HALF_TURNS))
def test_exact_half_turns(name):
    """R a signed permutation matrix: the antisymmetric part is exactly 0, every sign of the axis has to come from R + R^T."""
    R = HALF_TURNS[name]
    y = _maxabs(R, pm.exp_so3(np_log(R)))
    w = so3_host.log_so3(R)
    p = _maxabs(R, pm.exp_so3(w))
    back = np.abs(so3_host.rodrigues(w) - R).max()
    print("\nhalf turn %-16s yardstick %.2e product %.2e (float64 round trip %.2e)" % (name, y, p, back))
    assert abs(np.linalg.norm(w) - PI) <= 16 * EPS * PI
    assert p <= _tol(y) and back <= _tol(y)


def test_log_is_the_inverse_for_small_and_large_vectors():
    """The logarithm as a vector (not only as a rotation): |log(exp w) - w| relative to |w|, away from the half turn where w -> -w."""
    for name, angle in ANGLES[1:-1]:
        for w, Rm, Rf in _cases(angle)[:12]:
            wm = pm.log_so3(Rf)                       # the exact logarithm of the rounded matrix
            y = max(abs(mpf(float(v)) - e) for v, e in zip(np_log(Rf), wm))
            p = max(abs(mpf(float(v)) - e) for v, e in zip(so3_host.log_so3(Rf), wm))
            assert p <= 16 * max(float(y), EPS * angle), (name, float(p), float(y))


# ---- solve6 / invert6_column ------------------------------------------------------------------------------------------------------

def _spd(cond, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    A = (Q * np.logspace(0, -math.log10(cond), 6)) @ Q.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("cond", [1.0, 1e2, 1e4, 1e6, 1e8, 1e10, 1e12])
def test_solve6_and_inverse_against_lu_at_50_digits(cond):
    worst_s = worst_i = 0.0
    for seed in range(8):
        A = _spd(cond, 100 + seed)
        Am = mp.matrix(A.tolist())
        c2 = float(np.linalg.cond(A))
        bound = 64.0 * c2 * EPS
        g = np.random.default_rng(seed).standard_normal(6)
        ok, d = so3_host.solve6(A, g, 0.0)
        ref = pm.to_float(mp.lu_solve(Am, mp.matrix(g.tolist()))).reshape(6)
        assert ok
        worst_s = max(worst_s, np.abs(d - ref).max() / np.abs(ref).max() / bound)
        oks, inv = so3_host.invert6(A)
        refi = pm.to_float(mp.inverse(Am))
        assert all(oks)
        worst_i = max(worst_i, np.abs(inv - refi).max() / np.abs(refi).max() / bound)
        # the damped system the Levenberg-Marquardt step solves: (A + lambda diag(A)) d = g
        ok, d = so3_host.solve6(A, g, 1e-4)
        Ad = A + 1e-4 * np.diag(np.maximum(np.diag(A), 1e-12))
        ref = pm.to_float(mp.lu_solve(mp.matrix(Ad.tolist()), mp.matrix(g.tolist()))).reshape(6)
        assert ok and np.abs(d - ref).max() <= 64.0 * float(np.linalg.cond(Ad)) * EPS * np.abs(ref).max()
    print("\nsolve6 cond %.0e: worst error / (64 cond2 2^-53): solve %.3f, inverse %.3f" % (cond, worst_s, worst_i))
    assert worst_s <= 1.0 and worst_i <= 1.0


def test_solve6_refuses_what_is_not_positive_definite():
    rng = np.random.default_rng(5)
    # J^T J of two points (rank 4) and of one point (rank 2): what a mask that leaves one or two correspondences produces
    for rows in (2, 4):
        J = rng.standard_normal((rows, 6)) * np.array([900.0, 900, 900, 80, 80, 20])
        A = J.T @ J
        ok, _ = so3_host.solve6(A, np.ones(6), 0.0)
        oks, inv = so3_host.invert6(A)
        assert not ok and not any(oks) and np.isnan(inv).all()         # all six lanes alike; nothing written
    A = _spd(10.0, 1); A[5, 5] = -A[5, 5]                              # indefinite
    assert not so3_host.solve6(A, np.ones(6), 0.0)[0] and not any(so3_host.invert6(A)[0])
    assert not so3_host.solve6(np.zeros((6, 6)), np.zeros(6), 0.0)[0]  # empty mask, undamped
    ok, d = so3_host.solve6(np.zeros((6, 6)), np.zeros(6), 1e-4)       # empty mask, damped: a step of zero
    assert ok and not d.any()

"""The 50-digit reference of the bundle adjustment (tests/ba_mp.py) held to itself: the gradient and the Jacobian agree with differences of
the cost, the normal matrix annihilates the seven gauge directions (and a single observation's viewing ray), the polish reaches a
stationary point without raising the cost."""
from mpmath import mp, mpf

import ba_host as bh
import ba_mp
import pose_mp as pm

_CACHE = {}


def _scene_a():
    if "A" not in _CACHE:
        s = bh.scene("A")
        prob = bh.mp_problem(s)
        p = bh.mp_params(prob, s["Rt0"], s["X0"])
        _CACHE["A"] = (s, prob, p, ba_mp.normal_equations(prob, p))
    return _CACHE["A"]


def test_the_scene_has_what_it_is_for():
    s, prob, p, _ = _scene_a()
    res = ba_mp.residuals(prob, bh.mp_params(prob, s["Rt_true"], s["X_true"]))
    tail = [(t, c) for t, c, r0, r1, w, _ in res if w != 1]
    assert tail == s["tails"] and len(tail) == 1
    t, c, r0, r1, _, _ = [r for r in res if (r[0], r[1]) == tail[0]][0]
    assert 37 < float(mp.sqrt(r0 * r0 + r1 * r1)) < 41
    assert [t for t in ba_mp.points_of(prob) if len(ba_mp.bits_of(prob, t)) == 1] == s["singles"] and len(s["singles"]) == 1
    assert len(p) == 18 + 36


def test_gradient_and_jacobian_agree_with_differences_of_the_cost():
    s, prob, p, (A, g, c) = _scene_a()
    assert abs(c - ba_mp.cost(prob, p)) < mpf(10) ** -40 * c
    h = mpf(10) ** -15
    with mp.workdps(75):
        for i in (0, 2, 4, 7, 11, 17, 18, 20, 21, 23, 40, 53):
            pp, pm_ = list(p), list(p)
            pp[i] += h
            pm_[i] -= h
            d = (ba_mp.cost(prob, pp) - ba_mp.cost(prob, pm_)) / (2 * h)
            assert abs(-d - g[i]) < mpf(10) ** -20 * max(abs(g[i]), 1), i          # g is the descent side: -grad
    # the rows: a difference of the pixel itself along a random direction
    rows = ba_mp.jacobian_rows(prob, p)
    K = [pm.vec(k) for k in prob["K"]]
    import random
    rnd = random.Random(5)
    v = [mpf(rnd.uniform(-1, 1)) for _ in p]
    with mp.workdps(75):
        pars_p, X_p = ba_mp.unpack(prob, [a + h * b for a, b in zip(p, v)])
        pars_m, X_m = ba_mp.unpack(prob, [a - h * b for a, b in zip(p, v)])
        for t, c, du, dv in rows[::3]:
            up, _ = ba_mp.project(K[c], pars_p[c], X_p[t])
            um, _ = ba_mp.project(K[c], pars_m[c], X_m[t])
            for k, row in enumerate((du, dv)):
                want = (up[k] - um[k]) / (2 * h)
                got = sum(row[i] * v[i] for i in row)
                assert abs(got - want) < mpf(10) ** -20 * max(abs(want), 1), (t, c)


def test_the_normal_matrix_annihilates_the_gauge():
    s, prob, p, (A, g, c) = _scene_a()
    n = len(p)
    scale = max(A[i][i] for i in range(n))
    dirs = ba_mp.null_directions(prob, p)
    assert len(dirs) == 7 + 1
    for d in dirs:
        nd = mp.sqrt(sum(x * x for x in d))
        Ad = [sum(A[i][j] * d[j] for j in range(n)) for i in range(n)]
        assert max(abs(x) for x in Ad) < mpf(10) ** -40 * scale * nd
        assert abs(sum(x * y for x, y in zip(g, d))) < mpf(10) ** -40 * scale * nd          # and g has no component there
    # ... and nothing else of that kind: a direction that bends the scene is seen
    bend = [mpf(0)] * n
    bend[18] = mpf(1)
    assert max(abs(sum(A[i][j] * bend[j] for j in range(n))) for i in range(n)) > mpf(10) ** -6 * scale


def test_the_polish_reaches_a_stationary_point_and_does_not_raise_the_cost():
    s, prob, p, _ = _scene_a()
    r = bh.solve_scene(s)
    p1 = bh.mp_params(prob, r["Rt"], r["X"])
    c1 = ba_mp.cost(prob, p1)
    q, steps = ba_mp.polish(prob, p1)
    cq = ba_mp.cost(prob, q)
    assert steps <= 6 and cq <= c1
    _, g, _ = ba_mp.normal_equations(prob, q)
    assert max(abs(x) for x in g) < mpf(10) ** -24
    # the single observation's point lies on its ray: its residual is zero
    t = s["singles"][0]
    r0, r1 = [(a, b) for tt, _, a, b, _, _ in ba_mp.residuals(prob, q) if tt == t][0]
    assert abs(r0) < mpf(10) ** -40 and abs(r1) < mpf(10) ** -40

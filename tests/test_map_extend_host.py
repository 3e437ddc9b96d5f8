"""The map extension's statement (tests/map_extend_host.py) and the g++ build of coloc_amd/csrc/extend_math.h it stands on.  No GPU.

F from two poses is held to a 50-digit mpmath evaluation by a FORWARD bound: per entry |dF_ij| <= 64 * 2^-53 * S_ij, where S_ij is the
sum of the absolute values of the products that form the entry -- the same formulas evaluated in mpmath with every product's operands
replaced by their absolute sums and every subtraction by an addition, i.e. the sum of |monomial| over the entry's expansion in the
inputs.  The chain is five stages of at most five roundings each on such sums (R, t, E, E K_a^-1, K_b^-T ...), so 64 units in the last
place of S bound it with room; nothing is fitted to what the code gives."""
import mpmath as mp
import numpy as np
import pytest

import map_extend_host as mh
import unique_host as uh


@pytest.fixture(scope="module")
def main():
    views, info, par = mh.main_case()
    st = mh.statement(views[0], views[1], par["band"], par["threshold"], par["max_distance"], par["map_n"], 4096)
    return views, info, par, st


def test_main_case_holds_every_class(main):
    _, _, _, st = main
    c = st["classes"]
    print("classes of the main case:", c)
    for name in mh.CLASSES:
        assert c[name] >= 5, (name, c)
    assert c["guided"] == sum(c[k] for k in mh.CLASSES[1:])                 # the six classes partition the guided matches


def test_mask_is_extend_keeps(main):
    views, _, par, st = main
    hit = np.nonzero(st["guided"] >= 0)[0]
    keeps = mh.cxx_keeps(views[0]["track"][hit], views[1]["track"][st["guided"][hit]], st["best"][hit], par["max_distance"])
    assert np.array_equal(keeps, st["masked"][hit] >= 0)
    # the boundaries of the rule itself
    got = mh.cxx_keeps([-1, 0, -1, -1, -1, -1], [-1, -1, 0, -1, -1, -1], [5, 5, 5, 64, 65, 65535], 64)
    assert got.tolist() == [True, False, False, True, False, False]
    assert mh.cxx_keeps([-1, -1], [-1, -1], [0, 1], 0).tolist() == [True, False]
    assert mh.cxx_keeps([-1, -1], [-1, -1], [512, 513], 512).tolist() == [True, False]


def _mp_fundamental(cam_a, Rt_a, cam_b, Rt_b):
    """(F, S) in 50 digits: F by the definition, S the sum of |products| per entry"""
    mp.mp.dps = 50
    A = [[mp.mpf(float(v)) for v in row] for row in np.asarray(Rt_a, dtype=np.float64).reshape(3, 4)]
    B = [[mp.mpf(float(v)) for v in row] for row in np.asarray(Rt_b, dtype=np.float64).reshape(3, 4)]
    fa, pxa, pya = (mp.mpf(float(v)) for v in cam_a[:3])
    fb, pxb, pyb = (mp.mpf(float(v)) for v in cam_b[:3])

    def chain(ab):
        m = (lambda x, y: abs(x) * abs(y)) if ab else (lambda x, y: x * y)
        sub = (lambda x, y: x + y) if ab else (lambda x, y: x - y)
        one = (lambda x: abs(x)) if ab else (lambda x: x)
        R = [[m(B[r][0], A[c][0]) + m(B[r][1], A[c][1]) + m(B[r][2], A[c][2]) for c in range(3)] for r in range(3)]
        t = [sub(one(B[r][3]), m(R[r][0], A[0][3]) + m(R[r][1], A[1][3]) + m(R[r][2], A[2][3])) for r in range(3)]
        E = [[sub(m(t[1], R[2][c]), m(t[2], R[1][c])) for c in range(3)],
             [sub(m(t[2], R[0][c]), m(t[0], R[2][c])) for c in range(3)],
             [sub(m(t[0], R[1][c]), m(t[1], R[0][c])) for c in range(3)]]
        G = [[E[r][0] / fa, E[r][1] / fa, sub(E[r][2], (m(E[r][0], pxa) + m(E[r][1], pya)) / fa)] for r in range(3)]
        return [[G[0][c] / fb for c in range(3)], [G[1][c] / fb for c in range(3)],
                [sub(G[2][c], (m(G[0][c], pxb) + m(G[1][c], pyb)) / fb) for c in range(3)]]

    return chain(False), chain(True)


def _poses(rng):
    def rot():
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.column_stack([rot(), rng.normal(size=3) * 3.0]), np.column_stack([rot(), rng.normal(size=3) * 3.0])


def test_fundamental_within_the_forward_bound_of_a_50_digit_evaluation():
    rng = np.random.RandomState(5)
    cases = [(mh.CAM, mh.pose(0.0, (0, 0, 0)), mh.CAM, mh.pose(0.03, (0.6, 0, 0))),
             (mh.CAM, mh.pose(0.03, (0.6, 0, 0)), mh.CAM_K1, mh.pose(0.06, (1.2, 0, 0)))]
    for _ in range(20):
        Rt_a, Rt_b = _poses(rng)
        cases.append(((rng.uniform(300, 900), rng.uniform(200, 500), rng.uniform(150, 400)), Rt_a,
                      (rng.uniform(300, 900), rng.uniform(200, 500), rng.uniform(150, 400)), Rt_b))
    worst = 0.0
    for cam_a, Rt_a, cam_b, Rt_b in cases:
        F = mh.fundamental(cam_a, Rt_a, cam_b, Rt_b)
        Fm, S = _mp_fundamental(cam_a, Rt_a, cam_b, Rt_b)
        for i in range(3):
            for j in range(3):
                err, bound = abs(mp.mpf(float(F[i, j])) - Fm[i][j]), 64 * mp.mpf(2) ** -53 * S[i][j]
                worst = max(worst, float(err / bound) if bound > 0 else 0.0)
                assert err <= bound, (i, j, float(err), float(bound))
    print("F from poses: worst |dF| / bound = %.3f" % worst)


def test_noise_free_projections_lie_on_their_lines():
    views, info = mh.make_views([200, 200], seed=3, noise=0.0, doubles=False)
    a, b = views
    F = mh.fundamental(a["cam"], a["Rt"], b["cam"], b["Rt"])
    xa = np.column_stack([a["feat"][info[0]["common"]].astype(np.float64), np.ones(len(info[0]["common"]))])
    xb = np.column_stack([b["feat"][info[1]["common"]].astype(np.float64), np.ones(len(info[1]["common"]))])
    # (the positions are float32: re-project in float64 from the scene instead)
    pa, _ = mh._project(a["cam"], a["Rt"], info[0]["X"])
    pb, _ = mh._project(b["cam"], b["Rt"], info[0]["X"])
    xa[:, :2], xb[:, :2] = pa, pb
    r = np.abs(np.einsum("ni,ij,nj->n", xb, F, xa))
    lim = 1e-9 * np.linalg.norm(F) * np.linalg.norm(xa, axis=1) * np.linalg.norm(xb, axis=1)
    assert (r < lim).all(), float((r / lim).max())


def test_equal_centres_give_no_fundamental_and_no_rows():
    # both centres at the origin under different rotations; one pose twice under an axis permutation (R R^T exact)
    Rt_b = mh.pose(0.2, (0.0, 0.0, 0.0))
    perm = np.column_stack([np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), np.array([0.5, -2.0, 3.0])])
    for Rt_1, Rt_2 in ((mh.pose(0.0, (0.0, 0.0, 0.0)), Rt_b), (perm, perm)):
        F = mh.fundamental(mh.CAM, Rt_1, mh.CAM_K1, Rt_2)
        assert (F == 0.0).all()
    views, _ = mh.make_views([120, 120], seed=9)
    views[1]["Rt"] = views[0]["Rt"] = mh.pose(0.0, (0.0, 0.0, 0.0))
    st = mh.statement(views[0], views[1], mh.BAND, mh.THRESHOLD, mh.CAP, 40, 4096)
    assert (st["F"] == 0.0).all() and st["n_guided"] == 0 and st["n_added"] == 0 and st["n_dropped"] == 0


def test_appended_rows_are_one_to_one_untracked_and_ascending(main):
    views, _, par, st = main
    q, t = st["new_q"], st["new_t"]
    assert len(q) >= 5 and len(np.unique(q)) == len(q) and len(np.unique(t)) == len(t)
    assert (views[0]["track"][q] < 0).all() and (views[1]["track"][t] < 0).all()
    assert (np.diff(q) > 0).all()
    # the tracks afterwards name the new rows, and only there
    rows = par["map_n"] + np.arange(len(q))
    assert np.array_equal(st["track_a"][q], rows) and np.array_equal(st["track_b"][t], rows)
    other_a, other_b = np.setdiff1d(np.arange(400), q), np.setdiff1d(np.arange(400), t)
    assert np.array_equal(st["track_a"][other_a], views[0]["track"][other_a]) and np.array_equal(st["track_b"][other_b], views[1]["track"][other_b])
    # the filter left nothing to do
    again, _ = uh.unique(st["unique"], st["best"], 400)
    assert np.array_equal(again, st["unique"])


def test_truncation_keeps_a_prefix_of_the_unbounded_result(main):
    views, _, par, st = main
    for room in (0, 1, 7, st["n_added"], st["n_added"] + 3):
        cut = mh.statement(views[0], views[1], par["band"], par["threshold"], par["max_distance"], par["map_n"], par["map_n"] + room)
        n = min(room, st["n_added"])
        assert cut["n_added"] == n and cut["n_dropped"] == st["n_added"] - n
        assert np.array_equal(cut["new_q"], st["new_q"][:n]) and np.array_equal(cut["new_t"], st["new_t"][:n])
        assert np.array_equal(cut["X"].view(np.uint64), st["X"][:n].view(np.uint64))
        assert (cut["track_a"] >= par["map_n"]).sum() == n


def test_most_appended_points_are_the_scene_s(main):
    """what the rule is for: an appended landmark lies where the scene point of its two rows lies (the noise is 0.3 px)"""
    views, info, _, st = main
    row_to_point = {int(r): i for i, r in enumerate(info[0]["common"])}
    hits = [(row_to_point[int(q)], X) for q, X in zip(st["new_q"], st["X"]) if int(q) in row_to_point]
    assert len(hits) >= 0.8 * st["n_added"]
    err = np.array([np.linalg.norm(X - info[0]["X"][i]) / info[0]["X"][i][2] for i, X in hits])
    assert np.median(err) < 0.05, float(np.median(err))

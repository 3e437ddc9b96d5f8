"""The host statement of the map update's tail (tests/map_update_host.py over tests/host/map_update_lib.cpp: scale_term, scale_from_sum,
rescale_pose of coloc_amd/csrc/inter_math.h / map_math.h, built by g++ without contraction) against an independent Python restatement:
plain loops over Python floats (IEEE doubles) with numpy.float32 for the rule's two casts, the same IEEE operations in the same order --
so scale, n_terms and status are EXACTLY equal.  rescale_pose is held to a numpy.longdouble reference within a bound that follows from
its operation count."""
import math

import numpy as np
import pytest

import map_update_host as mu


def _dist32(a, b):
    """(float)sqrt(sum of squared differences): the differences, products and the left-to-right sum in double, the root in double, one cast"""
    d = [float(b[i]) - float(a[i]) for i in range(3)]
    s = d[0] * d[0] + d[1] * d[1]
    s = s + d[2] * d[2]
    return np.float32(math.sqrt(s))


def _scale_restated(old_X, new_X, cq, ct):
    total, good = 0.0, 0
    for k in range(len(cq) - 1):
        d1 = _dist32(old_X[cq[k]], old_X[cq[k + 1]])
        d2 = _dist32(new_X[ct[k]], new_X[ct[k + 1]])
        if d2 > np.float32(1e-9):
            total = total + float(np.float32(d1 / d2))           # float / float in float, widened
            good += 1
    if good == 0:
        return 1.0, 0, mu.NO_SCALE
    s = total / float(good)
    if not (s > 0.0) or not math.isfinite(s):
        return 1.0, good, mu.NO_SCALE
    return s, good, mu.OK


def _random_case(n_common, seed, n_old=None, n_new=None, true_scale=2.75):
    rng = np.random.default_rng(seed)
    n_old = n_old or n_common + 40
    n_new = n_new or n_common + 25
    new_X = np.stack([rng.uniform(-5, 5, n_new), rng.uniform(-3, 3, n_new), rng.uniform(4, 20, n_new)], 1)
    cq = np.sort(rng.choice(n_old, n_common, replace=False)).astype(np.int32)
    ct = rng.permutation(n_new)[:n_common].astype(np.int32)
    old_X = rng.uniform(-50, 50, (n_old, 3))
    old_X[cq] = new_X[ct] * true_scale + rng.normal(0, 0.01, (n_common, 3))
    return old_X, new_X, cq, ct


def _same(got, want):
    assert got[1] == want[1] and got[2] == want[2], (got, want)
    assert np.float64(got[0]).view(np.uint64) == np.float64(want[0]).view(np.uint64), (got, want)


@pytest.mark.parametrize("n_common", [2, 3, 1025, 3000])
def test_scale_of_random_lists_is_the_restatement_exactly(n_common):
    old_X, new_X, cq, ct = _random_case(n_common, 100 + n_common)
    got = mu.scale_of(old_X, new_X, cq, ct)
    _same(got, _scale_restated(old_X, new_X, cq, ct))
    assert got[2] == mu.OK and got[1] == n_common - 1 and abs(got[0] / 2.75 - 1) < 0.05


def test_repeated_new_rows_are_guarded_terms():
    old_X, new_X, cq, ct = _random_case(400, 7)
    ct[10] = ct[9]                      # two consecutive old rows matched to ONE new row: a zero denominator
    ct[200] = ct[201] = ct[199]         # and three
    ct[300] = ct[100]                   # a repeat that is NOT consecutive divides by an ordinary distance
    got = mu.scale_of(old_X, new_X, cq, ct)
    _same(got, _scale_restated(old_X, new_X, cq, ct))
    assert got[1] == 399 - 3 and got[2] == mu.OK and math.isfinite(got[0])


def test_empty_single_and_all_guarded_lists_give_one():
    old_X, new_X, cq, ct = _random_case(50, 9)
    for k in (0, 1):
        got = mu.scale_of(old_X, new_X, cq[:k], ct[:k])
        _same(got, _scale_restated(old_X, new_X, cq[:k], ct[:k]))
        assert got == (1.0, 0, mu.NO_SCALE)
    one = np.full(50, ct[3], dtype=np.int32)                     # every old row matched to one new row: every term guarded
    got = mu.scale_of(old_X, new_X, cq, one)
    _same(got, _scale_restated(old_X, new_X, cq, one))
    assert got == (1.0, 0, mu.NO_SCALE)
    # coincident OLD points: every term is 0, the mean is not positive
    flat = np.zeros_like(old_X)
    got = mu.scale_of(flat, new_X, cq, ct)
    _same(got, _scale_restated(flat, new_X, cq, ct))
    assert got == (1.0, 49, mu.NO_SCALE)


def test_common_list_is_ascending_old_row_and_drops_indices_outside_the_new_map():
    match = np.array([3, -1, 7, 5, 3, 8, -2, 0], dtype=np.int32)
    cq, ct = mu.common_list(match, 8)
    assert cq.tolist() == [0, 2, 3, 4, 7] and ct.tolist() == [3, 7, 5, 3, 0]
    assert mu.clean_match(match, 8).tolist() == [3, -1, 7, 5, 3, -1, -1, 0]
    r = mu.align(np.arange(24.0).reshape(8, 3), np.arange(24.0).reshape(8, 3) * 0.5, match)
    assert r["n_common"] == 5 and r["n_terms"] == 4 and r["status"] == mu.OK


def test_rescaled_points_are_one_multiply_each():
    rng = np.random.default_rng(3)
    X = rng.normal(0, 30, (777, 3))
    for s in (1.0, 2.75, 1.0 / 3.0, 1e-3):
        assert np.array_equal(mu.rescale_points(X, s).view(np.uint64), (X * s).view(np.uint64))


def test_rescale_pose_against_longdouble():
    """t' = -R (s C), C = -R^T t: two 3-term dot products and one multiply per component.  Each dot product of three products of size
    <= |R_ij| |v_j| carries at most 3 roundings relative to the sum of magnitudes (gamma_3), the multiply one more, and the error of C
    goes through the second dot product: |t' - t_ref|_max <= (3 + 1 + 3 + slack) u s |C|_1 with u = 2^-53 and |R_ij| <= 1; 32 * 2^-52
    leaves a factor of some eight over that count.  Not fitted to a run."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in range(200):
        a, b, c = rng.uniform(-np.pi, np.pi, 3)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
        R = Rz @ Ry @ Rx
        Cc = rng.uniform(-100, 100, 3) * 10.0 ** rng.integers(-2, 3)
        Rt = np.hstack([R, (-R @ Cc)[:, None]])
        s = float(rng.uniform(0.05, 20.0))
        got = mu.rescale_pose(Rt, s)
        assert np.array_equal(got[:, :3].view(np.uint64), Rt[:, :3].view(np.uint64))              # the rotation is not touched
        Rl, tl = Rt[:, :3].astype(np.longdouble), Rt[:, 3].astype(np.longdouble)
        C_ref = -(Rl.T @ tl)
        t_ref = -(Rl @ (C_ref * np.longdouble(s)))
        err = float(np.abs(got[:, 3].astype(np.longdouble) - t_ref).max())
        bound = 32.0 * 2.0 ** -52 * s * float(np.abs(C_ref).sum())
        print("rescale_pose case %d: err %.3e bound %.3e" % (k, err, bound))
        assert err <= bound, (k, err, bound)
        worst = max(worst, err / bound)
    print("worst err / bound", worst)

"""CPU tests of the 3-D similarity's arithmetic (coloc_amd/csrc/sim3_math.h through its host build, tests/sim3_host.py): the minimal
solver and Umeyama's refit against a 50-digit reference (tests/sim3_mp.py), the guard on both sides, the two apply rules against plain
numpy, and the sequential statement of clc_sim3_acransac on planted scenes.  The GPU equals this host build bit for bit
(tests/test_gpu_sim3.py), so what holds here holds there."""
import functools

import numpy as np
import pytest

import sim3_cases
import sim3_host
import sim3_mp

# Forward error of (s, R, t) against the 50-digit reference (sim3_mp.forward_error), measured on the well-conditioned cases below
# (triangle sine >= 1e-3; (sigma2 + sigma3) / sigma1 >= 1e-3): worst minimal case 3.65e-14 (thin0, sine 1.001e-3: the error grows like
# eps / sine), worst refit 8.82e-16 (cloud128).  The bound is 16 x the worst measured value: the device has the host's bits, so the
# margin only has to absorb the choice of cases.
SIM3_FORWARD_BOUND = 16 * 3.65e-14
MIN_SINE, MIN_SPREAD = 1e-3, 1e-3


def _host_minimal(x, y):
    A = sim3_host.minimal(x, y)
    return A, (None if np.isnan(A).any() else sim3_host.from_model(A))


@functools.lru_cache(maxsize=None)
def measured():
    """(worst minimal error, its case, worst refit error, its case) over the well-conditioned cases"""
    worst_m, name_m, worst_r, name_r = 0.0, None, 0.0, None
    for name, x, y, expect in sim3_cases.minimal_cases():
        if expect != "model" or min(sim3_mp.sine(x), sim3_mp.sine(y)) < MIN_SINE:
            continue
        _, got = _host_minimal(x, y)
        e = sim3_mp.forward_error(got, sim3_mp.minimal(x, y), x, y)
        if e > worst_m:
            worst_m, name_m = e, name
    for name, x, y, expect in sim3_cases.refit_cases():
        if expect != "refit" or sim3_mp.spread(x, y) < MIN_SPREAD:
            continue
        ok, s, R, t, _ = sim3_host.refit(x, y)
        e = sim3_mp.forward_error((s, R, t), sim3_mp.umeyama(x, y), x, y)
        if e > worst_r:
            worst_r, name_r = e, name
    return worst_m, name_m, worst_r, name_r


def test_forward_error_against_the_50_digit_reference():
    worst_m, name_m, worst_r, name_r = measured()
    print("sim3 forward error: minimal %.3g (%s), refit %.3g (%s), bound %.3g" % (worst_m, name_m, worst_r, name_r, SIM3_FORWARD_BOUND))
    assert name_m is not None and name_r is not None
    assert worst_m <= SIM3_FORWARD_BOUND and worst_r <= SIM3_FORWARD_BOUND


def test_well_conditioned_cases_cover_every_class():
    """the restriction to well-conditioned cases must not empty a class: general, scales, both rotation ends, thin triangles, every refit size"""
    kept = {n.rstrip("0123456789") for n, x, y, e in sim3_cases.minimal_cases() if e == "model" and min(sim3_mp.sine(x), sim3_mp.sine(y)) >= MIN_SINE}
    assert {"general", "scale", "angle", "thin"} <= kept
    kept = {n for n, x, y, e in sim3_cases.refit_cases() if e == "refit" and sim3_mp.spread(x, y) >= MIN_SPREAD}
    assert {"cloud4", "cloud128", "cloud129", "cloud2000", "exact300", "planar", "planar_reflected", "mirrored"} <= kept


@pytest.mark.parametrize("case", sim3_cases.minimal_cases(), ids=lambda c: c[0])
def test_minimal_solver(case):
    name, x, y, expect = case
    A, got = _host_minimal(x, y)
    if expect == "nan":
        assert np.isnan(A).all()
        return
    assert np.isfinite(A).all()
    s, R, t = got
    # a similarity: R orthonormal and proper, A = [sR | t]; it carries the new triangle's centroid onto the old one's
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-9) and abs(np.linalg.det(R) - 1) < 1e-9
    assert np.allclose(A.reshape(3, 4)[:, :3], s * R, rtol=1e-14, atol=0) and np.array_equal(A.reshape(3, 4)[:, 3], t)
    assert np.allclose(s * R @ x.mean(0) + t, y.mean(0), atol=1e-9 * (1 + np.abs(y).max()))
    ref = sim3_mp.minimal(x, y)
    sine = float(min(sim3_mp.sine(x), sim3_mp.sine(y)))
    err = sim3_mp.forward_error(got, ref, x, y)
    # beyond the well-conditioned cases the error may grow like eps / sine, no faster
    assert err <= (SIM3_FORWARD_BOUND if sine >= MIN_SINE else SIM3_FORWARD_BOUND * MIN_SINE / sine), (name, err, sine)


def test_guard_is_the_documented_rule():
    """degenerate iff |e1 x e2|^2 <= 1e-12 |e1|^2 |e2|^2 in either cloud"""
    for name, x, y, expect in sim3_cases.minimal_cases():
        def thin(p):
            e1, e2 = p[1] - p[0], p[2] - p[0]
            c = np.cross(e1, e2)
            return not (c @ c > 1e-12 * (e1 @ e1) * (e2 @ e2))
        assert (thin(x) or thin(y)) == (expect == "nan"), name


def test_exactly_similar_triangles_give_the_planted_similarity():
    rng = np.random.default_rng(3)
    for _ in range(50):
        x = rng.uniform(-5, 5, (3, 3))
        s, R, t = rng.uniform(0.1, 10), sim3_cases.rot(rng.normal(size=3), rng.uniform(0, np.pi)), rng.uniform(-5, 5, 3)
        A, (gs, gR, gt) = _host_minimal(x, sim3_cases.similar(x, s, R, t))
        assert abs(gs - s) <= 1e-12 * s and np.allclose(gR, R, atol=1e-11) and np.allclose(gt, t, atol=1e-10)
        assert sim3_host.residuals(A, x, sim3_cases.similar(x, s, R, t)).max() < 1e-20


@pytest.mark.parametrize("case", sim3_cases.refit_cases(), ids=lambda c: c[0])
def test_refit(case):
    name, x, y, expect = case
    ok, s, R, t, A = sim3_host.refit(x, y)
    if expect == "refused":
        assert not ok
        return
    assert ok and np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1) < 1e-12
    assert np.allclose(A[:, :3], s * R, rtol=1e-15, atol=0) and np.array_equal(A[:, 3], t)
    ref = sim3_mp.umeyama(x, y)
    assert sim3_mp.forward_error((s, R, t), ref, x, y) <= SIM3_FORWARD_BOUND, name
    if name in ("planar_reflected", "mirrored"):
        assert ref[3] == -1                                            # the reflection case was reached
    if name in ("exact300", "planar", "planar_reflected"):
        assert sim3_host.residuals(A, x, y).max() < 1e-18 * (1 + np.abs(y).max()) ** 2


def test_refit_takes_inliers_in_ascending_index_whatever_their_order():
    _, x, y, _ = sim3_cases.refit_cases()[1]
    rng = np.random.default_rng(1)
    inl = rng.permutation(len(x))[:100]
    a, b = sim3_host.refit(x, y, inl), sim3_host.refit(x[np.sort(inl)], y[np.sort(inl)])
    assert a[0] and b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_apply_rules_against_numpy():
    rng = np.random.default_rng(5)
    s, R, t = 2.5, sim3_cases.rot([1, -2, 0.5], 0.4), np.array([1.0, -2.0, 3.0])
    A = np.concatenate([s * R, t[:, None]], 1)
    X = rng.uniform(-10, 10, (50, 3))
    assert np.allclose(sim3_host.apply_points(A, X), s * X @ R.T + t, rtol=1e-14, atol=1e-13)
    Rc, C = sim3_cases.rot(rng.normal(size=3), 1.2), rng.uniform(-5, 5, 3)
    Rt = np.concatenate([Rc, (-Rc @ C)[:, None]], 1)
    got = sim3_host.apply_pose(s, R, t, Rt)
    # R_c' = R_c R^T, and the centre moves like a point: s R C + t
    assert np.allclose(got[:, :3], Rc @ R.T, atol=1e-14)
    assert np.allclose(-got[:, :3].T @ got[:, 3], s * R @ C + t, atol=1e-12)
    # a point keeps its coordinates in the moved camera up to the scale: R_c' X' + t_c' = s (R_c X + t_c)
    assert np.allclose((s * X @ R.T + t) @ got[:, :3].T + got[:, 3], s * (X @ Rc.T + Rt[:, 3]), atol=1e-11)
    # the scale-only rule: one multiplication per component; the pose's centre times s
    assert np.array_equal(sim3_host.scale_points(s, X), X * s)
    sp = sim3_host.scale_pose(s, Rt)
    assert np.array_equal(sp[:, :3], Rc) and np.allclose(-Rc.T @ sp[:, 3], C * s, atol=1e-12)


@pytest.mark.parametrize("n,share,seed", [(12, 0.25, 11), (64, 0.30, 12), (300, 0.25, 13), (300, 0.60, 14)])
def test_statement_recovers_the_planted_set(n, share, seed):
    sc = sim3_cases.planted_scene(n, share, seed)
    res = sim3_host.acransac(sc["x"], sc["y"], max_iteration=256, seed=seed)
    assert res["found"] and res["refit"] == 1
    assert np.array_equal(res["mask"], sc["planted"]) and sorted(res["inliers"]) == list(np.nonzero(sc["planted"])[0])
    assert abs(res["s"] - 2.5) <= SIM3_FORWARD_BOUND * 2.5
    assert np.allclose(res["R"], sc["R"], atol=SIM3_FORWARD_BOUND) and res["min_nfa"] < 0 and 0 <= res["valid"] < res["iterations"] <= 256


def test_statement_under_depth_dependent_noise():
    sc = sim3_cases.planted_scene(300, 0.25, 21, noise=1e-5)
    res = sim3_host.acransac(sc["x"], sc["y"], max_iteration=256, seed=4)
    assert res["found"] and abs(res["s"] - 2.5) < 1e-4 and not (res["mask"] & ~sc["planted"]).any()
    assert (res["mask"] & sc["planted"]).sum() >= 0.9 * sc["planted"].sum()


def test_statement_finds_nothing_where_there_is_nothing():
    rng = np.random.default_rng(9)
    x, y = rng.uniform(-10, 10, (40, 3)), rng.uniform(-10, 10, (40, 3))
    res = sim3_host.acransac(x, y, max_iteration=256, seed=3)
    assert not res["found"] and res["n_inliers"] == 0 and not res["mask"].any() and res["iterations"] == 256
    assert res["s"] == 1.0 and np.array_equal(res["R"], np.eye(3)) and not res["t"].any() and res["min_nfa"] >= 0
    # three correspondences: no solve runs
    res = sim3_host.acransac(x[:3], y[:3])
    assert not res["found"] and res["iterations"] == 0 and res["s"] == 1.0
    # a flat box of old points admits no alpha
    flat = y.copy()
    flat[:, 2] = 1.0
    res = sim3_host.acransac(x, flat)
    assert not res["found"] and res["iterations"] == 0 and sim3_host.box_volume(flat) == 0.0


def test_acceptance_needs_more_than_seven_inliers():
    """12 correspondences, 7 of them right: a meaningful model may exist, the rule of Localize (more than 2.5 x 3 inliers) refuses it"""
    sc = sim3_cases.planted_scene(12, 5 / 12, 31)
    assert sc["planted"].sum() == 7
    res = sim3_host.acransac(sc["x"], sc["y"], max_iteration=256, seed=1)
    assert not res["found"] and res["n_inliers"] == 0 and res["valid"] == -1 and res["s"] == 1.0

"""P3P against a high-precision reference, on the CPU: the reference against itself, the fixture against a recomputation, and the host
build of coloc_amd/csrc/p3p.h against the two rules of DESIGN.md (P3P) on every class of tests/p3p_cases.py.

The rules (B = 4096 * 2^-53 * max(|x|_inf, fx, fy); sigma = sine of the world triangle's angle at the first sample point):
  backward   every returned pose reprojects its own three sample points, at 50 digits, within B / sigma;
  forward    every in-range reference solution has a returned pose within J_k B / sigma + 16 * 2^-53 |P|_inf in all 12 entries, and every
             returned pose is within that bound of some reference solution.
Run with -s to see the measured figures of every class.
"""
import importlib.util
import os

import numpy as np
import pytest

import p3p_cases as cases
import p3p_host
import p3p_mp
from mpmath import mp, mpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return cases.load_fixture()


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_p3p_reference", os.path.join(ROOT, "tools", "make_p3p_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def host_slots(X, x, K):
    return np.stack([p3p_host.sample_poses(X[i], x[i], K, [0, 1, 2]).reshape(4, 12) for i in range(len(X))])


@pytest.mark.parametrize("name", cases.ASSERTED + cases.HARD)
def test_reference_certifies_itself_and_agrees_with_80_digits(fx, name):
    X, x, K = cases.class_inputs(name, fx)
    n = 0
    for i in (0, 31, 59):
        a = p3p_mp.solve(X[i], x[i], K)
        b = p3p_mp.solve(X[i], x[i], K, dps=max(80, a["dps"] + 20))
        assert len(a["sols"]) == len(b["sols"])
        with mp.workdps(100):
            for sa, sb in zip(a["sols"], b["sols"]):
                assert sa["cert"] <= p3p_mp.CERT_TOL and sb["cert"] <= p3p_mp.CERT_TOL
                assert max(abs(p - q) for p, q in zip(sa["P"], sb["P"])) <= mpf(10) ** -45
                n += 1
    assert n > 0


def test_fixture_inputs_are_the_case_table(fx):
    for name in cases.ASSERTED + cases.HARD:
        Xf, xf, Kf = cases.class_inputs(name, fx)
        X, x, K = cases.class_inputs(name)
        assert np.array_equal(X, Xf) and np.array_equal(x, xf) and np.array_equal(K, Kf), name


def test_fixture_size(fx):
    golden = os.path.dirname(cases.FIXTURE)
    others = [os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != os.path.basename(cases.FIXTURE)]
    assert os.path.getsize(cases.FIXTURE) <= max(others)


@pytest.mark.parametrize("name", cases.STORED)
def test_fixture_subset_recomputes_unchanged(fx, maker, name):
    X, x, K = cases.class_inputs(name, fx)
    stored = cases.class_references(fx, name)
    for i in ([0] if name in cases.BRANCH else [3, 42]):
        sig, rho, sols = stored[i]
        r = maker.reference_problem(X[i], x[i], K)
        assert r is not None and r["sigma"] == sig and np.float32(r["rho"]) == np.float32(rho) and len(r["sols"]) == len(sols)
        for a, b in zip(r["sols"], sols):
            assert np.array_equal(a["s_hi"], b["s_hi"]) and np.array_equal(a["s_lo"].astype(np.float64), b["s_lo"])
            assert np.array_equal(cases.half_to_float(a["J"]), b["J"]) and a["in_range"] == b["in_range"]


def test_asserted_classes_are_in_range(fx):
    """What the generator refuses to write: at most 5 % of an asserted class out of range; at most 25 % of a hard class under the rho cap."""
    for name in cases.ASSERTED + cases.HARD:
        refs = cases.class_references(fx, name)
        sols = [(rho, s) for _, rho, ss in refs for s in ss]
        assert all(rho >= 0 for _, rho, _ in refs) or name in cases.HARD
        out = sum(not s["in_range"] for _, s in sols)
        capped = sum(s["in_range"] and rho < cases.RHO_CAP for rho, s in sols)
        if name in cases.ASSERTED:
            assert out <= 0.05 * len(sols)
        else:
            assert capped <= 0.25 * len(sols)


@pytest.mark.parametrize("name", cases.ASSERTED + cases.HARD)
def test_host_build_meets_both_rules(fx, name):
    X, x, K = cases.class_inputs(name, fx)
    fig = cases.evaluate(name, host_slots(X, x, K), fx)
    print("\n%s (host): %s" % (name, fig))
    assert fig["poses"] > 0
    assert fig["backward_ratio"] <= 1.0
    assert fig["missed"] == 0 and fig["spurious"] == 0


# The `den` case: D(v) = 0 at the solution the case is built around.  N(v) = 0 there too and the quartic has a double root (rho = 6.5e-17),
# so the float root lands 1e-8 away, |D| = 1.9e-7 is far above the 1e-12 guard (test_den_case_does_not_reach_its_guard), u = N / D is
# 0 / 0 in disguise and two of the four slots hold poses that are not solutions.  Measured, host and device alike: worst backward
# error 10.4 px = 1.6e10 x B / sigma, 2 reference solutions missed, 2 poses spurious.  strict: the mark comes off when u is taken
# from the other two equations there.
DEN_XFAIL = "D(v) = 0 is a double root, the |den| guard is not reached: 10.4 px = 1.6e10 x B/sigma, 2 missed, 2 spurious"
BRANCH_PARAMS = [pytest.param(n, marks=pytest.mark.xfail(strict=True, reason=DEN_XFAIL)) if n == "den" else n for n in cases.BRANCH]


@pytest.mark.parametrize("name", BRANCH_PARAMS)
def test_branch_case_takes_its_branch_and_meets_both_rules(fx, name):
    X, x, K = cases.class_inputs(name, fx)
    br = p3p_host.sample_branches(X[0], x[0], K, [0, 1, 2])
    assert br["ok"]
    scale = np.abs(br["co"]).sum()
    if name == "cubic":
        assert not br["polish"] and abs(br["co"][4]) <= 1e-12 * scale and abs(br["co"][3]) > 1e-12 * scale
    elif name == "biquadratic":
        assert br["polish"] and br["biquadratic"]
    fig = cases.evaluate(name, host_slots(X, x, K), fx)
    print("\n%s (host): %s" % (name, fig))
    assert fig["backward_ratio"] <= 1.0
    assert fig["missed"] == 0 and fig["spurious"] == 0


def test_den_case_does_not_reach_its_guard(fx):
    """The case is built so that D vanishes at a solution, and the instrumented entry shows that no root is refused by the guard: the
    smallest |D(v)| over the polished roots is small (below 1e-5: the case is what it claims to be) and yet above the guard's 1e-12."""
    X, x, K = cases.class_inputs("den", fx)
    br = p3p_host.sample_branches(X[0], x[0], K, [0, 1, 2])
    assert br["ok"] and br["polish"] and not br["biquadratic"]
    assert not br["den_guard"].any()
    assert 1e-12 <= np.nanmin(np.abs(br["den"])) < 1e-5
    assert cases.class_references(fx, "den")[0][1] < 1e-12          # rho: a double root


@pytest.mark.parametrize("name", cases.REPORT)
def test_report_only_classes_keep_their_structure(name):
    """No rule is asserted here (DESIGN.md section 10 has the figures): a slot is all NaN or wholly finite, R R^T = I to 1e-9,
    det R > 0 -- cases.check_slots, inside evaluate.  Printed: the worst backward error over the class, and the missed and spurious
    poses over the problems that cases.report_table gives a reference."""
    fig = cases.evaluate(name, host_slots(*cases.report_table(name)[:3]), table=cases.report_table(name))
    print("\n%s (host, report only): poses %d, worst backward error %.3g px = %.3g x B/sigma; over the first %d problems (%d reference "
          "solutions): missed %d, spurious %d" % (name, fig["poses"], fig["backward_px"], fig["backward_ratio"], cases.N_REPORT_REF,
                                                  fig["refs"], fig["missed"], fig["spurious"]))

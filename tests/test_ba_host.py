"""The host statement of the bundle adjustment (tests/ba_host.py over the g++ build of coloc_amd/csrc/ba_math.h, tests/host/ba_lib.cpp)
against the 50-digit reference (tests/ba_mp.py) on the scenes the GPU tests use: the costs are the reference's, the result is the
minimum by rule b of tests/test_gpu_pose_edges.py with five times to spare, the single-observation points and the tail behave.

Measured here (and quoted by tests/test_gpu_map_ba.py): relative excess over cost(polish(output)) at the default tolerance A 1.5e-12, B
3.0e-11; at function_tolerance 1e-12 A 2.6e-14, B 3.6e-15."""
import ctypes as C
import math

import numpy as np
import pytest
from mpmath import mpf

import ba_host as bh
import ba_mp

_POLISHED = {}


def _polished(name):
    """the scene, its reference problem, the host result at the default tolerance and the polished cost of that result, formed once"""
    if name not in _POLISHED:
        s = bh.scene(name)
        prob = bh.mp_problem(s)
        r = bh.solve_scene(s)
        p1 = bh.mp_params(prob, r["Rt"], r["X"])
        q, _ = ba_mp.polish(prob, p1)
        _POLISHED[name] = (s, prob, r, ba_mp.cost(prob, p1), ba_mp.cost(prob, q))
    return _POLISHED[name]


@pytest.mark.parametrize("name", ["A", "B"])
def test_costs_and_minimum_against_the_reference(name):
    s, prob, r, c1, cq = _polished(name)
    c0 = ba_mp.cost(prob, bh.mp_params(prob, s["Rt0"], s["X0"]))
    assert r["status"] == bh.BA_OK and 3 <= r["iterations"] < 60
    assert r["n_obs"] == len(ba_mp.observations(prob)) and r["n_points"] == len(ba_mp.points_of(prob))
    assert abs(mpf(r["cost_initial"]) - c0) < mpf(10) ** -12 * c0 and abs(mpf(r["cost_final"]) - c1) < mpf(10) ** -12 * c1
    assert r["cost_final"] < r["cost_initial"]
    excess = float((c1 - cq) / cq)
    print(name, "excess", excess, "iterations", r["iterations"])
    assert 0 <= excess < 2e-10                   # the GPU test's bound is 1e-9: five times inside
    r12 = bh.solve_scene(s, function_tolerance=1e-12)
    spread = (mpf(r12["cost_final"]) - cq) / cq
    print(name, "spread at 1e-12", float(spread))
    assert -mpf(10) ** -15 < spread < 2.6e-14    # ten times this is scene C's margin in tests/test_gpu_map_ba.py


def test_scene_c_fills_the_system_and_skips_the_unmasked_camera():
    s = bh.scene("C")
    prob = bh.mp_problem(s)
    r = bh.solve_scene(s, function_tolerance=1e-12)
    assert r["status"] == bh.BA_OK and r["n_cams"] == 7 and r["n_points"] > 256
    assert r["n_obs"] == len(ba_mp.observations(prob)) and r["n_points"] == len(ba_mp.points_of(prob)) == len(s["obs"]) - 2
    c1 = ba_mp.cost(prob, bh.mp_params(prob, r["Rt"], r["X"]))
    assert abs(mpf(r["cost_final"]) - c1) < mpf(10) ** -12 * c1 and r["cost_final"] < 0.01 * r["cost_initial"]
    out = s["out_cam"]
    assert np.array_equal(r["Rt"][out], s["Rt0"][out])
    idle = [t for t in range(len(s["obs"])) if not (int(s["obs"][t]) & s["mask"])]
    assert len(idle) == 2 and np.array_equal(r["X"][idle], s["X0"][idle])
    assert len(s["singles"]) == 3 and len(s["tails"]) == 5


def test_statuses_of_the_edges():
    s = bh.scene("A")
    clean = bh.scene("A", noise=0.0, perturb=False)
    r = bh.solve_scene(clean)
    assert r["status"] == bh.BA_OK and r["cost_final"] <= r["cost_initial"] < 1e-12
    X0 = s["X0"].copy()
    Rt = s["Rt0"][0]
    X0[3] = Rt[:, :3].T @ (np.array([0.3, -0.2, -5.0]) - Rt[:, 3])
    r = bh.solve(s["K"], s["mask"], s["obs"], s["x"], s["Rt0"], X0)
    assert r["status"] == bh.BA_BAD_START and np.array_equal(r["X"], X0)
    r = bh.solve(s["K"], s["mask"], np.zeros_like(s["obs"]), s["x"], s["Rt0"], s["X0"])
    assert r["status"] == bh.BA_EMPTY
    r = bh.solve_scene(s, max_iterations=1)
    assert r["status"] == bh.BA_MAX_ITERATIONS and r["iterations"] == 1 and r["cost_final"] <= r["cost_initial"]


def test_a_rank_two_block_is_inverted_only_with_damping_and_never_gives_a_nan():
    lib = bh.lib()
    rng = np.random.RandomState(1)
    J = rng.standard_normal((2, 3)) * 100.0
    V = J.T @ J                                   # one observation: rank 2
    packed = np.array([V[0, 0], V[0, 1], V[0, 2], V[1, 1], V[1, 2], V[2, 2]])
    inv = np.zeros(6)
    assert lib.ba_host_invert3(packed.ctypes.data_as(C.c_void_p), C.c_double(0.0), inv.ctypes.data_as(C.c_void_p)) == 0
    for lam in (1e-12, 1e-9, 1e-4, 1.0):
        assert lib.ba_host_invert3(packed.ctypes.data_as(C.c_void_p), C.c_double(lam), inv.ctypes.data_as(C.c_void_p)) == 1
        M = np.array([[inv[0], inv[1], inv[2]], [inv[1], inv[3], inv[4]], [inv[2], inv[4], inv[5]]])
        D = V + lam * np.diag(np.diag(V))
        assert np.isfinite(M).all() and np.abs(M @ D - np.eye(3)).max() < 1e-3
    assert lib.ba_host_invert3(np.zeros(6).ctypes.data_as(C.c_void_p), C.c_double(1e-4), inv.ctypes.data_as(C.c_void_p)) in (0, 1) and np.isfinite(inv).all()
    # the scenes' single-observation points stay finite through the whole run
    for name in ("A", "B"):
        s, _, r, _, _ = _polished(name)
        assert np.isfinite(r["X"][s["singles"]]).all() and math.isfinite(r["cost_final"])

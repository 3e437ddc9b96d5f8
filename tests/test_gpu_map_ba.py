"""The grown map bundle-adjusted on the device (include/coloc_hip.h: clc_ba_dev, clc_map_build_grow_ba_dev, clc_map_init_grow_ba_batch_dev,
clc_map_update_grow_ba_batch_dev; coloc_amd/csrc/map_ba.hip) against the 50-digit reference (tests/ba_mp.py) and the host statement
(tests/ba_host.py) on the scenes of ba_host.scene.  The poses and points themselves are never compared across two arithmetics: the seven
gauge directions are free, so only the cost, the counts and -- between two runs of the SAME arithmetic -- the bits are.

Measured with the host statement (tests/ba_host.py; g++ build of ba_math.h, libm in place of the device's sincos) on the committed seeds:
  relative excess of cost_final over cost(polish(output)), default tolerance:   A 1.5e-12, B 3.0e-11   (bound 1e-9: 30 x and more inside)
  the same at function_tolerance 1e-12 (the spread of ba_host against ba_mp):   A 2.6e-14, B 3.6e-15   -> scene C's margin 10 x 2.6e-14
Measured on an MI355X with these seeds: excess A 1.5e-12 (9 iterations), B 3.0e-11 (14); reported costs within 3e-14 of the 50-digit
costs; scene C at function_tolerance 1e-12 ends 2.8e-15 BELOW the host statement's final cost (11 iterations each).
"""
import math

import numpy as np
import pytest
from mpmath import mpf

import ba_host as bh
import ba_mp

pytestmark = pytest.mark.gpu

W, H = 1280, 720
C_MARGIN = 2.6e-13          # 10 x the largest spread of ba_host against ba_mp on A and B at function_tolerance 1e-12 (docstring)


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _ctx(maxkp=4000):
    from coloc_amd import Context
    return Context(device=0, width=W, height=H, maxkp=maxkp, match_thresh=60)


@pytest.fixture(scope="module")
def ctx():
    c = _ctx()
    yield c
    c.close()


def _run(ctx, s, Rt0=None, X0=None, obs=None, x=None, mask=None, **kw):
    """clc_ba_dev on a scene -> (result dict, X after)"""
    Rt0 = s["Rt0"] if Rt0 is None else Rt0
    X0 = s["X0"] if X0 is None else X0
    obs = s["obs"] if obs is None else obs
    x = s["x"] if x is None else x
    d_X, d_obs, d_x = _dev(np.asarray(X0, dtype=np.float64)), _dev(np.asarray(obs, dtype=np.uint32).view(np.int32)), _dev(np.asarray(x, dtype=np.float64))
    cams = [tuple(k) + (0.0, 0.0, 0.0) for k in s["K"]]
    r = ctx.ba_dev(cams, s["mask"] if mask is None else mask, Rt0, len(obs), d_X.data_ptr(), d_obs.data_ptr(), d_x.data_ptr(), **kw)
    ctx.sync()
    return r, d_X.cpu().numpy()


_MP = {}


def _mp(s):
    """the scene's 50-digit problem and the cost at its start, formed once"""
    if s["name"] not in _MP:
        prob = bh.mp_problem(s)
        _MP[s["name"]] = (prob, ba_mp.cost(prob, bh.mp_params(prob, s["Rt0"], s["X0"])))
    return _MP[s["name"]]


def _rel(a, b):
    return float(abs(mpf(a) - b) / b)


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B"])
def test_costs_are_the_reference_costs_and_the_result_is_the_minimum(ctx, name):
    s = bh.scene(name)
    prob, c0 = _mp(s)
    r, X = _run(ctx, s)
    p1 = bh.mp_params(prob, r["Rt"], X)
    c1 = ba_mp.cost(prob, p1)
    q, steps = ba_mp.polish(prob, p1)
    cq = ba_mp.cost(prob, q)
    print(name, "status", r["status"], "iterations", r["iterations"], "cost_initial", r["cost_initial"], "cost_final", r["cost_final"],
          "rel", _rel(r["cost_initial"], c0), _rel(r["cost_final"], c1), "excess", float((c1 - cq) / cq), "polish steps", steps)
    assert r["status"] == bh.BA_OK
    assert r["n_obs"] == len(ba_mp.observations(prob)) and r["n_points"] == len(ba_mp.points_of(prob)) and r["n_cams"] == 3
    assert _rel(r["cost_initial"], c0) < 1e-9 and _rel(r["cost_final"], c1) < 1e-9
    assert r["cost_final"] <= r["cost_initial"]
    assert mpf(r["cost_final"]) <= cq * (1 + mpf(10) ** -9) + mpf(10) ** -9
    assert r["rmse"] == math.sqrt(r["cost_final"] / (2.0 * r["n_obs"]))


# ---- 2. the full system ---------------------------------------------------------------------------------------------------------------

def test_scene_c_fills_the_system_and_leaves_the_unmasked_camera_alone(ctx):
    s = bh.scene("C")
    prob, c0 = _mp(s)
    r, X = _run(ctx, s, function_tolerance=1e-12)
    host = bh.solve_scene(s, function_tolerance=1e-12)
    c1 = ba_mp.cost(prob, bh.mp_params(prob, r["Rt"], X))
    print("C status", r["status"], "iterations", r["iterations"], "cost_final", r["cost_final"], "host", host["cost_final"], host["iterations"],
          "rel", _rel(r["cost_initial"], c0), _rel(r["cost_final"], c1), "over host", r["cost_final"] / host["cost_final"] - 1.0)
    assert r["status"] == bh.BA_OK and r["n_cams"] == 7
    assert r["n_obs"] == host["n_obs"] == len(ba_mp.observations(prob)) and r["n_points"] == host["n_points"] == len(ba_mp.points_of(prob))
    assert r["n_points"] > 256 and r["n_points"] < len(s["obs"])
    assert _rel(r["cost_initial"], c0) < 1e-9 and _rel(r["cost_final"], c1) < 1e-9
    assert r["cost_final"] <= r["cost_initial"]
    assert r["cost_final"] <= host["cost_final"] * (1 + C_MARGIN)
    out = s["out_cam"]
    assert np.array_equal(_bits(r["Rt"][out]), _bits(s["Rt0"][out]))
    idle = [t for t in range(len(s["obs"])) if not (int(s["obs"][t]) & s["mask"])]
    assert len(idle) >= 2 and np.array_equal(_bits(X[idle]), _bits(s["X0"][idle]))
    moved = [t for t in range(len(s["obs"])) if int(s["obs"][t]) & s["mask"]]
    assert (X[moved] != s["X0"][moved]).any(axis=1).all()


# ---- 3. determinism -------------------------------------------------------------------------------------------------------------------

def test_two_runs_and_interleaved_empty_points_give_the_same_bits(ctx):
    s = bh.scene("B")
    r1, X1 = _run(ctx, s)
    r2, X2 = _run(ctx, s)
    keys = ("status", "iterations", "n_obs", "n_points", "cost_initial", "cost_final", "rmse")
    assert all(_bits(np.float64(r1[k])) == _bits(np.float64(r2[k])) for k in keys)
    assert np.array_equal(_bits(X1), _bits(X2)) and np.array_equal(_bits(r1["Rt"]), _bits(r2["Rt"]))
    # 200 points without an observation, interleaved: arbitrary X, arbitrary pixels
    rng = np.random.RandomState(3)
    n = len(s["obs"])
    where = np.sort(rng.choice(n + 200, n, replace=False))
    X0, obs, x = rng.uniform(-50, 50, (n + 200, 3)), np.zeros(n + 200, dtype=np.uint32), rng.uniform(0, 1000, (n + 200, 3, 2))
    X0[where], obs[where], x[where] = s["X0"], s["obs"], s["x"]
    r3, X3 = _run(ctx, s, X0=X0, obs=obs, x=x)
    assert all(_bits(np.float64(r1[k])) == _bits(np.float64(r3[k])) for k in keys)
    assert np.array_equal(_bits(X3[where]), _bits(X1)) and np.array_equal(_bits(r3["Rt"]), _bits(r1["Rt"]))
    empty = np.setdiff1d(np.arange(n + 200), where)
    assert np.array_equal(_bits(X3[empty]), _bits(X0[empty]))


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------------

def test_edges_true_parameters_bad_start_empty_and_one_iteration(ctx):
    from coloc_amd import CLCError, abi
    clean = bh.scene("A", noise=0.0, perturb=False)
    r, X = _run(ctx, clean)
    assert r["status"] == bh.BA_OK and r["cost_final"] <= r["cost_initial"] < 1e-12
    # one point behind a camera that observes it
    s = bh.scene("A")
    X0 = s["X0"].copy()
    t = 3
    assert int(s["obs"][t]) & 1
    Rt = s["Rt0"][0]
    X0[t] = Rt[:, :3].T @ (np.array([0.3, -0.2, -5.0]) - Rt[:, 3])
    r, X = _run(ctx, s, X0=X0)
    assert r["status"] == bh.BA_BAD_START and r["iterations"] == 0
    assert np.array_equal(_bits(X), _bits(X0)) and np.array_equal(_bits(r["Rt"]), _bits(np.ascontiguousarray(s["Rt0"])))
    # nothing to adjust
    r, X = _run(ctx, s, obs=np.zeros_like(s["obs"]))
    assert r["status"] == bh.BA_EMPTY and r["n_obs"] == 0 and r["n_points"] == 0 and np.array_equal(_bits(X), _bits(s["X0"]))
    r, X = _run(ctx, s, mask=0)
    assert r["status"] == bh.BA_EMPTY and r["n_cams"] == 0
    # one step
    r, X = _run(ctx, s, max_iterations=1)
    assert r["status"] == bh.BA_MAX_ITERATIONS and r["iterations"] == 1 and r["cost_final"] <= r["cost_initial"]
    # argument errors
    for kw in (dict(max_iterations=-1), dict(function_tolerance=-1e-9)):
        with pytest.raises(CLCError) as e:
            _run(ctx, s, **kw)
        assert e.value.status == abi.CLC_ERR_BAD_ARG
    bad = dict(s)
    bad["K"] = s["K"].copy()
    bad["K"][1, 0] = 0.0
    with pytest.raises(CLCError) as e:
        _run(ctx, bad)
    assert e.value.status == abi.CLC_ERR_BAD_ARG
    d_X = _dev(s["X0"])
    with pytest.raises(CLCError) as e:
        ctx.ba_dev([(1000.0, 640.0, 360.0, 0, 0, 0)] * 3, 7, s["Rt0"], 12, d_X.data_ptr() + 4, d_X.data_ptr(), d_X.data_ptr())
    assert e.value.status == abi.CLC_ERR_BAD_ARG


# ---- 5. the composition ---------------------------------------------------------------------------------------------------------------

def _job4(seed=31, n=300, n_matches=150):
    """a 4-camera job of the kind tests/test_gpu_map_grow.py builds: scene, all six pairs, descriptors"""
    from test_gpu_map_grow import _descriptors, _scene, _scene_pairs
    sc = _scene(4, n, seed)
    pairs = _scene_pairs(sc, n_matches, seed + 100, wrong=0.02)
    return dict(sc=sc, pairs=pairs, rows=[n] * 4, desc=_descriptors(n, sc["point_of"], seed + 200, flips=6), n=n)


def _dev_job(j, keep):
    from test_gpu_map_grow import _dev_cams, _dev_pairs
    return _dev_pairs(j["pairs"], keep), _dev_cams(j["sc"]["cams"], keep, j["desc"])


def test_composition_equals_the_plain_build_and_the_step_alone_and_the_map_serves():
    torch = _torch()
    j = _job4()
    sc, rows, n = j["sc"], j["rows"], j["n"]
    plain, adjusted, alone = _ctx(), _ctx(), _ctx()
    try:
        keep = []
        pairs_dev, cams_dev = _dev_job(j, keep)
        base = plain.map_build_grow_dev(rows, pairs_dev, cams_dev, 0, sc["Rt"][0], sc["Rt"][1], seed=7)
        got = adjusted.map_build_grow_ba_dev(rows, pairs_dev, cams_dev, 0, sc["Rt"][0], sc["Rt"][1], seed=7)
        gb, gg, ba = base["grow"], got["grow"], got["ba"]
        # (a) the discrete outputs are the plain build's
        assert got["map_n"] == base["map_n"] > 100 and got["n_tracks"] == base["n_tracks"]
        for key in ("track_feat", "map_track", "map_row"):
            assert np.array_equal(got[key], base[key]), key
        for key in ("resected", "status", "n_corr", "n_inliers", "error_max", "n_seed_rows", "n_added"):
            assert gg[key] == gb[key], key
        assert np.array_equal(gg["map_cam"], gb["map_cam"]) and np.array_equal(gg["map_obs"], gb["map_obs"])
        assert gb["resected"] == [False, False, True, True]
        assert ba["status"] == bh.BA_OK and ba["n_cams"] == 4 and ba["n_points"] == base["map_n"]
        assert ba["n_obs"] == int(sum(bin(int(o)).count("1") for o in gb["map_obs"])) and ba["cost_final"] < ba["cost_initial"]
        assert not np.array_equal(_bits(got["X"]), _bits(base["X"]))
        # (b) X and Rt are clc_ba_dev's on the plain build's state laid out per track, the pixels from the resection lists
        nt = base["n_tracks"]
        X_t, obs_t, x_t = np.zeros((nt, 3)), np.zeros(nt, dtype=np.uint32), np.zeros((nt, 4, 2))
        X_t[base["map_track"]] = base["X"]
        obs_t[base["map_track"]] = gb["map_obs"]
        for c in range(4):
            d_Xl, d_xl = torch.zeros(3 * n, dtype=torch.float64, device="cuda"), torch.zeros(2 * n, dtype=torch.float64, device="cuda")
            d_tl, d_nl = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            plain.map_resect_build_dev(rows, cams_dev, c, d_Xl.data_ptr(), d_xl.data_ptr(), d_tl.data_ptr(), None, d_nl.data_ptr(), None)
            plain.sync()
            k = int(d_nl.cpu()[0])
            x_t[d_tl.cpu().numpy()[:k], c] = d_xl.cpu().numpy().reshape(-1, 2)[:k]
        d_X, d_obs, d_x = _dev(X_t), _dev(obs_t.view(np.int32)), _dev(x_t)
        r = alone.ba_dev([c["cam"] for c in sc["cams"]], 0xF, np.array(gb["Rt"]), nt, d_X.data_ptr(), d_obs.data_ptr(), d_x.data_ptr())
        alone.sync()
        assert (r["status"], r["iterations"], r["n_obs"], r["n_points"]) == (ba["status"], ba["iterations"], ba["n_obs"], ba["n_points"])
        assert r["cost_initial"] == ba["cost_initial"] and r["cost_final"] == ba["cost_final"]
        assert np.array_equal(_bits(d_X.cpu().numpy()[base["map_track"]]), _bits(got["X"]))
        assert np.array_equal(_bits(r["Rt"]), _bits(np.array(gg["Rt"])))
        assert np.array_equal(_bits(got["Rt_seed_a"]), _bits(gg["Rt"][0])) and np.array_equal(_bits(got["Rt_seed_b"]), _bits(gg["Rt"][1]))
        # (c) the installed map serves: camera 2's frame is localized against it
        d_q, d_f = _dev(j["desc"][2]), _dev(sc["cams"][2]["feat"])
        d_match = torch.full((n,), -5, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        adjusted.match_map_dev(d_q.data_ptr(), n, 60, d_match.data_ptr(), None)
        loc = adjusted.track_localize_dev(d_match=d_match.data_ptr(), nq=n, cam=sc["cams"][2]["cam"], d_feat=d_f.data_ptr(), feat_stride=4, seed=3)
        adjusted.sync()
        assert loc["Rt"] is not None and len(loc["inliers"]) > 40
        # a null ba and a negative tolerance are refused before anything runs
        from coloc_amd import CLCError, abi
        with pytest.raises(CLCError) as e:
            adjusted.map_build_grow_ba_dev(rows, pairs_dev, cams_dev, 0, sc["Rt"][0], sc["Rt"][1], seed=7, function_tolerance=-1.0)
        assert e.value.status == abi.CLC_ERR_BAD_ARG
        torch.cuda.synchronize()
    finally:
        for c in (plain, adjusted, alone):
            c.close()


# ---- 6. the update form ---------------------------------------------------------------------------------------------------------------

def test_update_form_rescales_the_refined_map():
    from coloc_amd import abi
    from test_gpu_map_grow import _composition_scene
    s = _composition_scene((300, 260, 10), 61)
    n, sc, rng = s["n"], s["sc"], s["rng"]
    set1, twins, plain = [_ctx() for _ in range(3)], [_ctx() for _ in range(3)], [_ctx() for _ in range(3)]
    try:
        origin_R, origin_C, scale = np.eye(3), np.array([0.3, -0.2, 0.1]), 3.0
        prev_rows = rng.choice(n, 150, replace=False)
        prev_desc = rng.integers(0, 256, (200, 64), dtype=np.uint8)
        where = np.sort(rng.choice(200, 150, replace=False))
        prev_desc[where] = s["desc"][0][prev_rows]
        prev_X = np.stack([rng.uniform(-5, 5, 200), rng.uniform(-3, 3, 200), rng.uniform(8, 20, 200)], 1) * 2.5
        prev_X[where] = sc["X"][sc["point_of"][0][prev_rows]] * 2.5
        set1[0].set_map(prev_desc)
        set1[0].set_map_points(prev_X)
        kw = dict(origin_R=origin_R, origin_C=origin_C, scale=scale, seed=11)
        tw, _ = abi.map_init_grow_ba_batch_dev(twins, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], **kw)
        base, _ = abi.map_init_grow_batch_dev(plain, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], **kw)
        assert tw["ba"]["status"] == bh.BA_OK and tw["ba"]["n_cams"] == 3 and tw["ba"]["cost_final"] < tw["ba"]["cost_initial"]
        assert tw["map_n"] == base["map_n"] and np.array_equal(tw["map_track"], base["map_track"]) and tw["grow"]["resected"] == [False, False, True]
        got, _ = abi.map_update_grow_ba_batch_dev(set1, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], **kw)
        sc_ = got["align"]["scale"]
        assert got["align"]["status"] == abi.MAP_ALIGN_OK and abs(sc_ - 1.0) > 1e-3
        assert got["map_n"] == tw["map_n"] and np.array_equal(got["map_track"], tw["map_track"])
        assert got["ba"] == tw["ba"]
        assert np.array_equal(_bits(got["X"]), _bits(tw["X"] * sc_))
        _torch().cuda.synchronize()
    finally:
        for c in set1 + twins + plain:
            c.close()

"""The map replaced on the device under an a-contrario similarity (include/coloc_hip.h: clc_map_align_sim_dev,
clc_map_update_sim_batch_dev).  Built from the helpers of tests/test_gpu_map_update.py: the descriptors and their oracle-checked matches are
that file's.  Comparison rule: the common list, match, counts, flags and status are compared EXACTLY, s, R, t, error_max, min_nfa and every
point BIT FOR BIT with the host statement (tests/sim3_host.py: the sequential solve on the common features, then the host build's
transform)."""
import numpy as np
import pytest

import map_update_host as mu
import sim3_cases
import sim3_host as sh
import test_gpu_map_build as mb
import test_gpu_map_update as tmu

pytestmark = pytest.mark.gpu


def _align(ctx, c, use_rows=True, install=True, **kw):
    if use_rows:
        d_desc, d_rows = mb._dev(c["block"]), mb._dev(c["rows"])
    else:
        d_desc, d_rows = mb._dev(c["new_desc"]), None
    d_X = mb._dev(c["new_X"])
    r = ctx.map_align_sim_dev(d_desc.data_ptr(), d_X.data_ptr(), c["n_new"], d_rows=None if d_rows is None else d_rows.data_ptr(), install=install, **kw)
    ctx.sync()
    assert np.array_equal(mb._bits(d_X.cpu().numpy()), mb._bits(c["new_X"]))           # d_X itself is not written
    return r, (d_desc, d_rows, d_X)


def _want(c, apply=sh.APPLY_SCALE, **kw):
    return sh.map_align_sim(c["old_X"], c["new_X"], c["match"], apply=apply, **kw)


def _check(got, want, n_old, what):
    assert got["n_old"] == n_old, (what, got["n_old"])
    assert np.array_equal(got["match"], want["match"]), what
    for k in ("n_common", "n_inliers", "iterations", "refit", "status"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["inlier"], want["inlier"]), what
    for k in ("s", "R", "t", "error_max", "min_nfa", "X"):
        assert np.array_equal(mb._bits(np.float64(got[k])), mb._bits(np.float64(want[k]))), (what, k, got[k], want[k])


# ---- 1. hand-placed ----------------------------------------------------------------------------------------------------------------

_HAND = []


def _hand_case():
    """60 old and 60 new rows, every old row matched: 45 true commons under an exact similarity (s = 2.5, 0.1 rad, a translation) and 15
    wrong ones whose old landmarks lie far from where the similarity puts them"""
    if not _HAND:
        rng = np.random.default_rng(7)
        q, t = np.arange(60), rng.permutation(60)
        new_X = tmu._points(rng, 60)
        R, tr = sim3_cases.rot([0.3, -1.0, 0.5], 0.1), np.array([3.0, -2.0, 5.0])
        old_X = np.zeros((60, 3))
        old_X[q] = 2.5 * new_X[t] @ R.T + tr
        wrong = np.sort(rng.choice(60, 15, replace=False))
        old_X[wrong] += rng.uniform(15, 40, (15, 3)) * rng.choice([-1.0, 1.0], (15, 3))
        c = tmu._case(60, 60, q, t, 8, old_X=old_X, new_X=new_X)
        c["true"] = np.ones(60, dtype=bool)
        c["true"][wrong] = False
        c["R"], c["t"] = R, tr
        _HAND.append(c)
    return _HAND[0]


def test_hand_placed():
    c = _hand_case()
    # a condition on the INPUT: the rule of clc_map_align_dev is more than 1 % off the planted scale on it
    old_rule = c["want"]
    assert old_rule["n_common"] == 60 and abs(old_rule["scale"] / 2.5 - 1) > 0.01, old_rule["scale"]
    want = _want(c, sh.APPLY_FULL, seed=3)
    assert want["found"] and want["refit"] == 1 and np.array_equal(want["inlier"], c["true"]) and want["n_inliers"] == 45
    assert abs(want["s"] - 2.5) < 1e-12 and np.allclose(want["R"], c["R"], atol=1e-12) and np.allclose(want["t"], c["t"], atol=1e-11)
    ctx = mb._ctx()
    try:
        tmu._install_old(ctx, c)
        # the common list and match are clc_map_align_dev's report-only output on the same input
        ref, _ = tmu._align(ctx, c, use_rows=False, install=False)
        got, keep = _align(ctx, c, use_rows=False, install=False, apply=sh.APPLY_FULL, seed=3)
        assert np.array_equal(got["match"], ref["match"]) and got["n_common"] == ref["n_common"] == 60 and got["n_old"] == ref["n_old"]
        assert np.array_equal(got["inlier"], c["true"])                # exactly the 45
        _check(got, want, 60, "hand")
    finally:
        ctx.close()


# ---- 2. sizes ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("apply", [sh.APPLY_SCALE, sh.APPLY_FULL])
def test_across_the_passes(apply):
    """2 500 old rows: three passes of the gather over the old rows, 1 800 common features (two elements per thread in the sort)"""
    c = tmu._big_case()
    want = _want(c, apply, seed=11)
    assert want["n_common"] == 1800 and want["found"] and abs(want["s"] / 2.5 - 1) < 0.01
    ctx = mb._ctx(maxkp=4000)
    try:
        tmu._install_old(ctx, c)
        got, keep = _align(ctx, c, use_rows=True, install=True, apply=apply, seed=11)
        _check(got, want, 2500, ("passes", apply))
        tmu._serves_like_host_map(ctx, c["new_desc"], want["X"], ("passes, installed", apply))
    finally:
        ctx.close()


def test_two_old_rows_matched_to_one_new_row():
    """K2NN is not one-to-one: old rows 10 and 11 (and 40, 41, 42) match ONE new row each -- repeated correspondences, which the old rule
    had to guard against, are ordinary data here"""
    rng = np.random.default_rng(17)
    q, t = tmu._spread_commons(120, 100, 60, 18)
    q = np.unique(np.concatenate([q, [10, 11, 40, 41, 42]]))
    t = rng.permutation(100)[:len(q)]
    t[np.searchsorted(q, 11)] = t[np.searchsorted(q, 10)]
    t[np.searchsorted(q, 41)] = t[np.searchsorted(q, 42)] = t[np.searchsorted(q, 40)]
    c = tmu._case(120, 100, q, t, 19)
    want = _want(c, sh.APPLY_FULL, seed=2)
    assert want["found"] and want["n_common"] == len(q) and len(set(t.tolist())) == len(q) - 3
    ctx = mb._ctx()
    try:
        tmu._install_old(ctx, c)
        got, keep = _align(ctx, c, use_rows=False, install=True, apply=sh.APPLY_FULL, seed=2)
        _check(got, want, 120, "repeated")
    finally:
        ctx.close()


# ---- 3. both apply modes, install, report only ------------------------------------------------------------------------------------

@pytest.mark.parametrize("apply", [sh.APPLY_SCALE, sh.APPLY_FULL])
def test_installed_map_serves(apply):
    c = tmu._mid_case()
    want = _want(c, apply, seed=5)
    assert want["found"] and want["n_common"] == 500
    if apply == sh.APPLY_SCALE:
        assert np.array_equal(want["X"], c["new_X"] * want["s"])       # one multiply per component
    ctx = mb._ctx()
    try:
        tmu._install_old(ctx, c)
        got, keep = _align(ctx, c, install=True, apply=apply, seed=5)
        _check(got, want, 700, ("install", apply))
        a = tmu._serves_like_host_map(ctx, c["new_desc"], want["X"], ("installed", apply))
        assert (a[0] >= 0).sum() > 400 and a[1]["Rt"] is not None
    finally:
        ctx.close()


def test_report_only_leaves_the_map():
    c = tmu._mid_case()
    want = _want(c, sh.APPLY_FULL, seed=5)
    ctx = mb._ctx()
    try:
        tmu._install_old(ctx, c)
        frame = tmu._frame(c["old_desc"], c["old_X"], 43)
        before = tmu._answer(ctx, frame)
        for again in range(2):
            got, keep = _align(ctx, c, install=False, apply=sh.APPLY_FULL, seed=5)
            _check(got, want, 700, ("report only", again))
            mb._same_frame(tmu._answer(ctx, frame), before, ("after a report-only call", again))
    finally:
        ctx.close()


# ---- 4. no model -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["zero", "five", "flat"])
def test_no_model_installs_the_unchanged_bits(kind):
    n_old, n_new = 300, 200
    old_X = None
    if kind == "zero":
        q, t = [], []
    elif kind == "five":
        q, t = [10, 50, 90, 150, 250], [5, 6, 7, 8, 9]               # a model may be meaningful; the acceptance rule needs more than 7
    else:
        q, t = tmu._spread_commons(n_old, n_new, 100, 33)
        old_X = tmu._points(np.random.default_rng(34), n_old)
        old_X[:, 2] = 4.0                                            # a flat box of old points
    c = tmu._case(n_old, n_new, q, t, 31, old_X=old_X)
    want = _want(c, sh.APPLY_FULL)
    assert not want["found"] and want["status"] == sh.SIM_NO_MODEL and want["n_common"] == len(q)
    ctx = mb._ctx()
    try:
        tmu._install_old(ctx, c)
        got, keep = _align(ctx, c, use_rows=False, install=True, apply=sh.APPLY_FULL)
        _check(got, want, n_old, kind)
        assert got["s"] == 1.0 and np.array_equal(got["R"], np.eye(3)) and not got["t"].any() and got["status"] == 1 and got["n_inliers"] == 0
        assert np.array_equal(mb._bits(got["X"]), mb._bits(c["new_X"]))
        tmu._serves_like_host_map(ctx, c["new_desc"], c["new_X"], kind)
    finally:
        ctx.close()


# ---- 5. twice in a row -------------------------------------------------------------------------------------------------------------

def test_twice_in_a_row():
    """A by set_map; B aligned to A; C aligned to B AS TRANSFORMED; D aligned to C: the buffers have changed places three times"""
    rng = np.random.default_rng(51)
    sizes = [600, 550, 640, 500]
    qt = [tmu._spread_commons(sizes[k], sizes[k + 1], 400, 52 + k) for k in range(3)]
    ab = tmu._case(sizes[0], sizes[1], qt[0][0], qt[0][1], 61, true_scale=2.0)
    ctx = mb._ctx()
    try:
        tmu._install_old(ctx, ab)
        want = _want(ab, sh.APPLY_FULL, seed=1)
        got, keep = _align(ctx, ab, use_rows=False, install=True, apply=sh.APPLY_FULL, seed=1)
        _check(got, want, sizes[0], "B to A")
        prev_desc, prev_X = ab["new_desc"], want["X"]
        for k in (1, 2):
            apply = sh.APPLY_SCALE if k == 1 else sh.APPLY_FULL
            R, tr = sim3_cases.rot([0.0, 1.0, 0.2], 0.05 * k), np.array([0.5, -0.25, 1.0])
            new_X = tmu._points(rng, sizes[k + 1])
            new_X[qt[k][1]] = ((prev_X[qt[k][0]] - tr) @ R) / (0.4 * k) + rng.normal(0, 0.004, (400, 3))
            c = tmu._case(sizes[k], sizes[k + 1], qt[k][0], qt[k][1], 62 + k, old_X=prev_X, new_X=new_X, old_desc=prev_desc)
            want = _want(c, apply, seed=k)
            got, keep = _align(ctx, c, use_rows=False, install=True, apply=apply, seed=k)
            _check(got, want, sizes[k], ("step", k))
            assert got["status"] == 0 and abs(got["s"] / (0.4 * k) - 1) < 0.01
            prev_desc, prev_X = c["new_desc"], want["X"]
        tmu._serves_like_host_map(ctx, prev_desc, prev_X, "after three installs")
    finally:
        ctx.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------

def test_errors_keep_the_previous_map():
    from coloc_amd import CLCError, abi
    torch = mb._torch()
    c = tmu._mid_case()
    ctx, fresh, rows_only = mb._ctx(maxkp=1000), mb._ctx(maxkp=1000), mb._ctx(maxkp=1000)
    try:
        tmu._install_old(ctx, c)
        frame = tmu._frame(c["old_desc"], c["old_X"], 43)
        before = tmu._answer(ctx, frame)
        d_desc = torch.zeros((1001, 64), dtype=torch.uint8, device="cuda")
        d_X = torch.ones((1001, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for kw, status in ((dict(n_new=1001), abi.CLC_ERR_CAPACITY),
                           (dict(n_new=100, d_desc=d_desc.data_ptr() + 8), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=-1), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, d_X=None), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, d_desc=None), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, d_X=d_X.data_ptr() + 4), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, d_rows=d_X.data_ptr() + 2), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, apply=2), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, max_iteration=-1), abi.CLC_ERR_BAD_ARG)):
            args = dict(dict(d_desc=d_desc.data_ptr(), d_X=d_X.data_ptr(), install=True), **kw)
            with pytest.raises(CLCError) as e:
                ctx.map_align_sim_dev(**args)
            assert e.value.status == status, kw
            mb._same_frame(tmu._answer(ctx, frame), before, ("after", kw))
        rows_only.set_map(c["old_desc"])
        for other in (fresh, rows_only):
            with pytest.raises(CLCError) as e:
                other.map_align_sim_dev(d_desc.data_ptr(), d_X.data_ptr(), 100)
            assert e.value.status == abi.CLC_ERR_STATE
        # the context works afterwards
        got, keep = _align(ctx, c, install=True, apply=sh.APPLY_FULL, seed=5)
        _check(got, _want(c, sh.APPLY_FULL, seed=5), 700, "after the refusals")
    finally:
        for x in (ctx, fresh, rows_only):
            x.close()


def test_an_empty_new_map():
    c = tmu._mid_case()
    ctx = mb._ctx()
    try:
        tmu._install_old(ctx, c)
        frame = tmu._frame(c["old_desc"], c["old_X"], 43)
        before = tmu._answer(ctx, frame)
        got = ctx.map_align_sim_dev(None, None, 0, install=False)
        assert (got["n_old"], got["n_common"], got["status"], got["s"]) == (700, 0, 1, 1.0) and (got["match"] == -1).all()
        mb._same_frame(tmu._answer(ctx, frame), before, "empty, report only")
    finally:
        ctx.close()


# ---- 7. after_stream ---------------------------------------------------------------------------------------------------------------

def test_after_stream_orders_the_call_behind_the_producer():
    torch = mb._torch()
    c = tmu._big_case()
    want = _want(c, sh.APPLY_FULL, seed=11)
    ctx = mb._ctx(maxkp=4000)
    try:
        tmu._install_old(ctx, c)
        src = [mb._dev(c["block"]), mb._dev(c["rows"]), mb._dev(c["new_X"])]
        dst = [torch.zeros_like(s) for s in src]
        a = torch.randn(2048, 2048, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(20):
                a = (a @ a) * 1e-3
            for d, s in zip(dst, src):
                d.copy_(s)
            got = ctx.map_align_sim_dev(dst[0].data_ptr(), dst[2].data_ptr(), c["n_new"], d_rows=dst[1].data_ptr(), install=True, apply=sh.APPLY_FULL,
                                        seed=11, after_stream=torch.cuda.current_stream().cuda_stream)
        _check(got, want, 2500, "after_stream")
        torch.cuda.synchronize()
    finally:
        ctx.close()


# ---- 8. the composition ------------------------------------------------------------------------------------------------------------

_SCENE = []


def _scene():
    """the rendered scene of the existing update tests (tests/test_gpu_map_grow.py) and a previous map: 200 rows, 150 of them copies of
    camera 0's rows, their points the world's at 2.5 x"""
    if not _SCENE:
        from test_gpu_map_grow import _composition_scene
        s = _composition_scene((300, 260, 10), 61)
        n, sc, rng = s["n"], s["sc"], s["rng"]
        prev_rows = rng.choice(n, 150, replace=False)
        prev_desc = rng.integers(0, 256, (200, 64), dtype=np.uint8)
        where = np.sort(rng.choice(200, 150, replace=False))
        prev_desc[where] = s["desc"][0][prev_rows]
        prev_X = np.stack([rng.uniform(-5, 5, 200), rng.uniform(-3, 3, 200), rng.uniform(8, 20, 200)], 1) * 2.5
        prev_X[where] = sc["X"][sc["point_of"][0][prev_rows]] * 2.5
        s["prev_desc"], s["prev_X"] = prev_desc, prev_X
        _SCENE.append(s)
    return _SCENE[0]


@pytest.mark.parametrize("stages,apply", [("plain", sh.APPLY_FULL), ("grow", sh.APPLY_SCALE), ("grow", sh.APPLY_FULL), ("grow_ba", sh.APPLY_FULL)])
def test_composition_equals_init_then_the_step(stages, apply):
    import oracle_lib
    from coloc_amd import abi
    s = _scene()
    n = s["n"]
    set1, twins, old = [mb._ctx() for _ in range(3)], [mb._ctx() for _ in range(3)], [mb._ctx() for _ in range(3)]
    try:
        kw = dict(origin_R=np.eye(3), origin_C=np.array([0.3, -0.2, 0.1]), scale=3.0)
        gkw = dict(kw, seed=11)
        for first in (set1[0], old[0]):
            first.set_map(s["prev_desc"])
            first.set_map_points(s["prev_X"])
        args = (s["jobs"], [n] * 3, s["pair_cams"], s["dc"])
        # the twin set: the init call alone; a third set: the existing update call of the same stages
        if stages == "plain":
            tw, _ = abi.map_init_batch_dev(twins, *args, **kw)
            ex, _ = abi.map_update_batch_dev(old, *args, **kw)
            new_desc = s["desc"][s["pair_cams"][tw["seed_pair"]][0]][tw["map_row"]]
        elif stages == "grow":
            tw, _ = abi.map_init_grow_batch_dev(twins, *args, **gkw)
            ex, _ = abi.map_update_grow_batch_dev(old, *args, **gkw)
        else:
            tw, _ = abi.map_init_grow_ba_batch_dev(twins, *args, **gkw)
            ex, _ = abi.map_update_grow_ba_batch_dev(old, *args, **gkw)
        if stages != "plain":
            new_desc = np.stack([s["desc"][c][r] for c, r in zip(tw["grow"]["map_cam"], tw["map_row"])])
        got, _ = abi.map_update_sim_batch_dev(set1, *args, apply=apply, sim_seed=9, grow=stages != "plain", ba=stages == "grow_ba", **gkw)
        # every discrete output equals the existing call's
        for k in ("seed_pair", "entered", "n_tracks", "map_n", "status"):
            assert got[k] == ex[k], k
        for k in ("track_feat", "map_track", "map_row"):
            assert np.array_equal(got[k], ex[k]), k
        gs, ea = got["sim"], ex["align"]
        assert np.array_equal(gs["match"], ea["match"]) and (gs["n_old"], gs["n_common"]) == (ea["n_old"], ea["n_common"])
        if stages != "plain":
            for k in ("resected", "status", "n_corr", "n_inliers", "n_seed_rows", "n_added"):
                assert got["grow"][k] == ex["grow"][k], k
            assert np.array_equal(got["grow"]["map_cam"], ex["grow"]["map_cam"]) and np.array_equal(got["grow"]["map_obs"], ex["grow"]["map_obs"])
        if stages == "grow_ba":
            assert got["ba"] == ex["ba"] == tw["ba"]
        # the step is the host statement's on the twin's map and the oracle's matches
        want = sh.map_align_sim(s["prev_X"], tw["X"], oracle_lib.Oracle().k2nn(s["prev_desc"], new_desc, 60), apply=apply, seed=9)
        assert want["found"] and want["n_common"] > 50 and abs(want["s"] - 1.0) > 1e-3
        _check(dict(gs, X=got["X"]), want, 200, (stages, apply))
        # ... and the poses are the twin's under the reported similarity
        for key in ("Rt_seed_a", "Rt_seed_b"):
            assert np.array_equal(mb._bits(got[key]), mb._bits(sh.transform_pose(want, tw[key], apply))), key
        if stages != "plain":
            for c in range(3):
                assert np.array_equal(mb._bits(got["grow"]["Rt"][c]), mb._bits(sh.transform_pose(want, tw["grow"]["Rt"][c], apply))), c
        tmu._serves_like_host_map(set1[0], new_desc, want["X"], (stages, apply))
        mb._torch().cuda.synchronize()
    finally:
        for c in set1 + twins + old:
            c.close()


def test_composition_without_an_entering_pair_or_a_previous_map():
    from coloc_amd import CLCError, abi
    s = tmu._composition_scene((10, 9, 8), 91)
    n = s["n"]
    set1 = [mb._ctx() for _ in range(3)]
    try:
        with pytest.raises(CLCError) as e:                                            # no previous map on ctxs[0]
            abi.map_update_sim_batch_dev(set1, s["jobs"], [n] * 3, s["pair_cams"], s["dc"])
        assert e.value.status == abi.CLC_ERR_STATE
        set1[0].set_map(s["prev_desc"])
        set1[0].set_map_points(s["prev_X"])
        frame = tmu._frame(s["prev_desc"], s["prev_X"], 92, n=200)
        before = tmu._answer(set1[0], frame)
        got, filt = abi.map_update_sim_batch_dev(set1, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], grow=True)
        assert got["seed_pair"] == -1 and got["map_n"] == -1 and got["entered"] == [False] * 3 and got["status"] == 0
        assert (got["sim"]["status"], got["sim"]["s"], got["sim"]["n_common"]) == (1, 1.0, 0)
        mb._same_frame(tmu._answer(set1[0], frame), before, "no pair entered")
    finally:
        for c in set1:
            c.close()

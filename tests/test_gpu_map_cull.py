"""The map's observation statistics and the cull on the device (include/coloc_hip.h: clc_map_observe_dev, clc_map_observe_batch_dev,
clc_map_cull_dev, clc_map_stats_get, clc_cull_map_points) against the host statement (tests/map_cull_host.py).  Every comparison is EXACT:
the counters, the epochs, the remap on the host and on the device, the counts and the per-clause counts, the track lists as the call
leaves them, the map's descriptor rows (Hamming distance 0) and its points through their uint64 view.

Shapes: the scan is ONE workgroup of 1 024 that walks the rows in passes of 16 waves, so the map sizes straddle a wave (63, 64, 65), a pass
(1 023, 1 024, 1 025) and a third pass (2 049); the wide launches run 256 threads a workgroup."""
import numpy as np
import pytest

import guided_host as gh
import map_cull_host as ch
import map_extend_host as mh
import proj_host as ph
import test_gpu_map_extend as tme

pytestmark = pytest.mark.gpu

_dev, _torch, _bits = tme._dev, tme._torch, tme._bits
CAM = gh.CAM_EXACT
RULE = dict(ch.DEFAULT_RULE)
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049]
PATTERNS = ("all", "none", "first", "last", "alternating", "random")


def _ctx(M, X, maxkp=4096):
    from coloc_amd import Context
    ctx = Context(device=0, detector=False, maxkp=maxkp)
    ctx.set_map(M)
    ctx.set_map_points(X)
    return ctx


def _points(ctx, n):
    """the context's first n map points in row order (clc_track_build_dev of the identity list)"""
    torch = _torch()
    if n == 0:
        return np.zeros((0, 3))
    ident, d_feat = _dev(np.arange(n, dtype=np.int32)), _dev(np.zeros((n, 2), dtype=np.float32))
    dX, dx = torch.zeros((3 * n,), dtype=torch.float64, device="cuda"), torch.zeros((2 * n,), dtype=torch.float64, device="cuda")
    dn = torch.zeros((1,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.track_build_dev(dX.data_ptr(), dx.data_ptr(), None, None, dn.data_ptr(), d_match=ident.data_ptr(), nq=n, cam=mh.CAM, d_feat=d_feat.data_ptr(),
                        feat_stride=2)
    ctx.sync()
    assert int(dn.cpu().numpy()[0]) == n
    return dX.cpu().numpy().reshape(-1, 3)


class _Obs:
    """device copies of one observed view: positions (float rows of stride 2), the d_track list (one poisoned entry behind it), the count
    word, the { n_in_view, n_hit } output (one poisoned entry behind it)"""

    def __init__(self, v):
        torch = _torch()
        self.n = n = 0 if v.get("track") is None else len(v["track"])
        self.feat = _dev(np.ascontiguousarray(v["feat"], dtype=np.float32).reshape(-1, 2) if n else np.zeros((1, 2), np.float32))
        self.counts = torch.full((3,), -7, dtype=torch.int32, device="cuda")
        self.kw = dict(n=n, cam=v["cam"], Rt=v["Rt"], width=v["width"], height=v["height"], gate=v["gate"], margin=v["margin"],
                       d_feat=self.feat.data_ptr(), feat_stride=2, d_counts=self.counts.data_ptr())
        if v.get("track") is not None:
            self.track = _dev(np.concatenate([np.asarray(v["track"], dtype=np.int32), np.array([-7], dtype=np.int32)]))
            self.kw["d_track"] = self.track.data_ptr()
        if v.get("count") is not None:
            self.count = _dev(np.array([v["count"], v["count"] + 17], dtype=np.uint32).view(np.int32))
            self.kw["d_count"] = self.count.data_ptr()
        torch.cuda.synchronize()

    def out(self):
        c = self.counts.cpu().numpy()
        assert c[2] == -7
        return int(c[0]), int(c[1])


def _same_stats(ctx, st, map_n, what):
    got = ctx.map_stats()
    st.cover(map_n)
    v, f, l = st.arrays()
    assert got["rows"] == map_n and got["epoch"] == st.epoch, (what, got["rows"], got["epoch"], st.epoch)
    assert np.array_equal(got["visible"], v), (what, "visible")
    assert np.array_equal(got["found"], f), (what, "found")
    assert np.array_equal(got["last_view"], l), (what, "last_view")
    assert (got["found"] <= got["visible"]).all()


def _lists(rng, n):
    """two track lists with the entries the rule names: -1, n_before, n_before - 1, a negative other than -1"""
    a = np.concatenate([rng.randint(-2, n + 2, 37), [-1, n, n - 1, -5]]).astype(np.int32)
    b = np.concatenate([[n - 1, -(2 ** 31), n, -1], np.arange(n, dtype=np.int32)[::-1][:300]]).astype(np.int32)
    return [a, b]


def _cull(ctx, st, M, X, rule, flagged, lists, what):
    """one cull on the device against the statement; everything the call returns and leaves -> the statement's result"""
    torch = _torch()
    n = len(M)
    want = ch.cull(st, M, X, rule, flagged, lists)
    d_lists = [_dev(np.concatenate([l, np.array([-7], dtype=np.int32)])) for l in lists]
    d_remap = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    d_flag = _dev(np.concatenate([np.asarray(flagged, dtype=np.uint8), np.array([1], dtype=np.uint8)])) if flagged is not None else None
    torch.cuda.synchronize()
    got = ctx.map_cull_dev(d_flagged=None if d_flag is None else d_flag.data_ptr(), lists=[(d.data_ptr(), len(l)) for d, l in zip(d_lists, lists)],
                           d_remap=d_remap.data_ptr(), **rule)
    assert got["status"] == 0, what
    for k in ("map_n_before", "n_kept", "n_dropped", "n_flagged", "n_ratio", "n_idle"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["n_kept"] + got["n_dropped"] == n and got["n_dropped"] == got["n_flagged"] + got["n_ratio"] + got["n_idle"]
    assert np.array_equal(got["remap"], want["remap"]), (what, "h_remap")
    dr = d_remap.cpu().numpy()
    assert np.array_equal(dr[:n], want["remap"]) and dr[n] == -7, (what, "d_remap")
    for d, l, w in zip(d_lists, lists, want["lists"]):
        h = d.cpu().numpy()
        assert np.array_equal(h[:len(l)], w) and h[len(l)] == -7, (what, "list")
    return want


@pytest.mark.parametrize("n", SIZES)
def test_compaction_edges(n):
    rng = np.random.RandomState(1000 + n)
    M, X = mh.make_map(n, 5 + n)
    ctx = _ctx(M, X)
    try:
        for pattern in PATTERNS if n else ("all",):
            ctx.set_map(M)                                                       # the rows replaced: the statistics start again
            ctx.set_map_points(X)
            st = ch.Stats()
            keep = dict(all=np.ones(n, dtype=bool), none=np.zeros(n, dtype=bool), first=np.arange(n) == 0, last=np.arange(n) == n - 1,
                        alternating=np.arange(n) % 2 == 0, random=rng.uniform(size=n) < 0.7)[pattern]
            if pattern == "random":
                # counters that differ from row to row, planted by two observes: every landmark lies in front of the identity pose and
                # inside the image; the keypoints sit on the projections of the rows they track, every third one 9 px away
                proj = ph.project(np.eye(3, 4), CAM, X)[0]
                for k in range(2):
                    rows = rng.choice(n, max(n // 2, 1), replace=False).astype(np.int32)
                    feat = proj[rows].copy()
                    feat[k::3] += 9.0
                    view = dict(cam=CAM, Rt=np.eye(3, 4), feat=feat, track=rows, count=None, width=640, height=480, gate=2.0, margin=0.0)
                    ch.observe(st, X, [view])
                    ctx.map_observe_dev(**_Obs(view).kw)
                _same_stats(ctx, st, n, (n, pattern, "planted"))
                if n > 8:
                    assert len(set(st.found)) > 1 and min(st.visible) >= 1
            want = _cull(ctx, st, M, X, RULE, (~keep).astype(np.uint8), _lists(rng, n), (n, pattern))
            assert want["n_kept"] == int(keep.sum()) and want["n_flagged"] == n - want["n_kept"]
            tme._check_map(ctx, want["M"], want["X"], (n, pattern))
            _same_stats(ctx, st, want["n_kept"], (n, pattern, "after the install"))
        if n == 0:
            got = ctx.map_cull_dev(**RULE)
            assert (got["n_kept"], got["n_dropped"], got["map_n_before"], len(got["remap"])) == (0, 0, 0, 0)
    finally:
        ctx.close()


def test_a_null_flag_list_and_nothing_dropped_is_the_identity():
    M, X = mh.make_map(70, 3)
    ctx = _ctx(M, X)
    try:
        st = ch.Stats()
        want = _cull(ctx, st, M, X, RULE, None, _lists(np.random.RandomState(1), 70), "identity")
        assert want["n_kept"] == 70 and np.array_equal(want["remap"], np.arange(70))
        tme._check_map(ctx, M, X, "identity")
    finally:
        ctx.close()


def _observe_scene():
    """300 landmarks for CAM_EXACT and three views.  View 0 is the identity pose with margin 4: rows 0 - 3 project EXACTLY onto lo, just
    below lo, hi_x, just above hi_x; rows 4 - 23 lie behind the camera, rows 24 - 43 outside the image.  -> (X, views, info)"""
    rng = np.random.RandomState(77)
    n = 300
    px = np.column_stack([rng.uniform(10, 630, n), rng.uniform(10, 470, n)])
    z = rng.uniform(3.0, 30.0, n)
    X = np.column_stack([(px[:, 0] - 320.0) * z / 512.0, (px[:, 1] - 240.0) * z / 512.0, z])
    X[0], X[1], X[2], X[3] = ph.landmark(4.0, 100.5, 2.0), ph.landmark(3.5, 100.5, 2.0), ph.landmark(635.0, 200.5, 4.0), ph.landmark(635.5, 200.5, 4.0)
    X[4:24, 2] *= -1.0
    X[24:34] = [ph.landmark(-50.5 - i, 100.5, 2.0) for i in range(10)]
    X[34:44] = [ph.landmark(100.5, 700.5 + i, 2.0) for i in range(10)]
    views = []
    poses = [np.eye(3, 4), mh.pose(0.05, (0.4, 0.0, 0.0)), mh.pose(-0.04, (-0.3, 0.1, 0.0))]
    cams = [CAM, mh.CAM_K1, CAM]
    for k in range(3):
        proj = ph.project(poses[k], cams[k], X)[0]
        rows = rng.choice(np.arange(44, n), 200, replace=False).astype(np.int32)
        pos = mh._project(cams[k], poses[k], X[rows])[0] + rng.normal(0.0, 0.8, (200, 2))     # distorted pixels plus noise: both sides of the gate
        track = rows.copy()
        track[:6] = [n, 1000, -1, -5, n + 1, 2 ** 31 - 1]                        # entries that name no row
        twice = int(rows[10])                                                    # two keypoints track one row: one inside the gate, one outside
        pos[10] = mh._project(cams[k], poses[k], X[twice:twice + 1])[0][0] + (0.25, 0.0)
        track[11], pos[11] = twice, pos[10] + (10.0, 0.0)
        far = int(rows[12])                                                      # and one row whose two keypoints are both outside
        pos[12] = mh._project(cams[k], poses[k], X[far:far + 1])[0][0] + (7.0, 0.0)
        track[13], pos[13] = far, pos[12] + (0.0, 9.0)
        if k == 0:                                                               # the border rows are tracked by keypoints ON their projections
            track[14:18], pos[14:18] = [0, 1, 2, 3], proj[0:4]
        views.append(dict(cam=cams[k], Rt=poses[k], feat=pos.astype(np.float32), track=track, count=None, width=640, height=480, gate=1.5,
                          margin=4.0 if k == 0 else 0.0))
    # a d_count that clips the keypoints that would have hit: the last five of view 0 sit exactly on rows nothing else tracks
    lone = np.array([44 + i for i in range(60) if (44 + i) not in set(views[0]["track"].tolist())][:5], dtype=np.int32)
    assert len(lone) == 5
    views[0]["track"][-5:] = lone
    views[0]["feat"][-5:] = ph.project(poses[0], cams[0], X[lone])[0]
    unclipped = dict(views[0])
    views[0]["count"] = 195
    return X, views, dict(lone=lone, unclipped=unclipped, twice=twice, far=far)


def test_observe_single_calls_and_a_batch_of_three():
    X, views, info = _observe_scene()
    n = len(X)
    M = np.random.RandomState(2).randint(0, 256, (n, 64)).astype(np.uint8)
    # what the scene holds, by the statement
    inv0, hit0, proj0 = ch.view_flags(X, views[0])
    assert proj0[0, 0] == np.float32(4.0) and proj0[2, 0] == np.float32(635.0)   # EXACTLY lo and hi_x
    assert list(inv0[:4]) == [True, False, True, False] and list(hit0[:4]) == [True, True, True, True]
    assert not inv0[4:44].any() and inv0[44:].sum() > 200
    assert not hit0[info["lone"]].any() and ch.view_flags(X, info["unclipped"])[1][info["lone"]].all()      # the count clips what would have hit
    for k in range(3):
        inv, hit, _ = ch.view_flags(X, views[k])
        assert 20 < (inv & hit).sum() < inv.sum() - 20                           # both sides of the gate
    single, batch = _ctx(M, X), _ctx(M, X)
    try:
        st = ch.Stats()
        for k in range(3):
            counts = ch.observe(st, X, [views[k]])
            o = _Obs(views[k])
            got = single.map_observe_dev(**o.kw)
            assert (got["epoch"], got["map_n"], got["status"]) == (k + 1, n, 0)
            _same_stats(single, st, n, ("single", k))
            assert o.out() == counts[0], ("single", k)
            assert (o.track.cpu().numpy()[:o.n] == views[k]["track"]).all()      # the list is read only
        sb = ch.Stats()
        counts = ch.observe(sb, X, views)
        obs = [_Obs(v) for v in views]
        got = batch.map_observe_batch_dev([o.kw for o in obs])
        assert [g["epoch"] for g in got] == [1, 1, 1]
        _same_stats(batch, sb, n, "batch")
        assert [o.out() for o in obs] == counts
        # the batch is the three single calls except for the epochs: one batch is one epoch
        assert sb.visible == st.visible and sb.found == st.found and max(st.visible) == 3
        assert (st.epoch, sb.epoch) == (3, 1)
        assert set(st.last_view) > {0, 3} and set(sb.last_view) == {0, 1}          # the last call that saw the row / the one call
        assert [l > 0 for l in st.last_view] == [l > 0 for l in sb.last_view]
        gs, gb = single.map_stats(), batch.map_stats()
        assert np.array_equal(gs["visible"], gb["visible"]) and np.array_equal(gs["found"], gb["found"]) and not np.array_equal(gs["last_view"], gb["last_view"])
        assert batch.map_observe_batch_dev([]) == [] and batch.map_stats()["epoch"] == 2        # an empty batch is an epoch too
    finally:
        single.close()
        batch.close()


def test_cover_of_appended_rows_and_reset():
    views, _, par = mh.main_case()
    par = {k: par[k] for k in ("band", "threshold", "max_distance")}
    ctx, M, X = tme._ctx(maxkp=2048)
    try:
        st = ch.Stats()
        a = views[0]
        ov = dict(cam=a["cam"], Rt=a["Rt"], feat=a["feat"], track=a["track"], count=None, width=mh.W, height=mh.H, gate=3.0, margin=0.0)
        ch.observe(st, X, [ov])
        ctx.map_observe_dev(**_Obs(ov).kw)
        _same_stats(ctx, st, tme.MAP_N, "before the extension")
        ext, M2, X2 = tme._run(ctx, views[0], views[1], par, 2048, tme.MAP_N, M, X, "extend")
        assert ext["n_added"] > 12
        n2 = len(M2)
        _same_stats(ctx, st, n2, "covered")                                      # clc_map_stats_get covers
        assert st.visible[tme.MAP_N:] == [0] * ext["n_added"] and st.last_view[tme.MAP_N:] == [1] * ext["n_added"] and st.epoch == 1
        ov2 = dict(ov, track=ext["track_a"])
        ch.observe(st, X2, [ov2])
        ctx.map_observe_dev(**_Obs(ov2).kw)
        _same_stats(ctx, st, n2, "after the extension")
        assert min(st.found[tme.MAP_N:]) == 1                                    # every new landmark is found by the keypoint it came from
        # an observe straight behind an extension covers too (no clc_map_stats_get between them)
        ext2, M3, X3 = tme._run(ctx, dict(views[0], track=ext["track_a"]), dict(views[1], track=ext["track_b"]), dict(par, band=6.0), 2048, n2, M2, X2, "again")
        ch.observe(st, X3, [ov2])
        ctx.map_observe_dev(**_Obs(ov2).kw)
        _same_stats(ctx, st, len(M3), "observe covers")
        # clc_set_map replaces the rows: the statistics start again
        ctx.set_map(M)
        ctx.set_map_points(X)
        st.reset()
        _same_stats(ctx, st, tme.MAP_N, "reset")
        assert st.epoch == 0 and st.visible == [0] * tme.MAP_N
    finally:
        ctx.close()


def test_idle_clause_drops_the_half_no_pose_looks_at():
    rng = np.random.RandomState(4)
    n, max_idle = 200, 3
    M, X = mh.make_map(n, 8)
    back = rng.permutation(n)[:n // 2]
    X[back, 2] *= -1.0                                                           # half the map lies behind the first pose ...
    turned = mh.pose(np.pi, (0.0, 0.0, 0.0))                                     # ... and in front of the second
    base = dict(cam=CAM, feat=np.zeros((0, 2), np.float32), track=None, count=None, width=640, height=480, gate=2.0, margin=0.0)
    front_view, back_view = dict(base, Rt=np.eye(3, 4)), dict(base, Rt=turned)
    is_back = np.zeros(n, dtype=bool)
    is_back[back] = True
    assert np.array_equal(ch.view_flags(X, front_view)[0], ~is_back) and np.array_equal(ch.view_flags(X, back_view)[0], is_back)
    ctx = _ctx(M, X)
    try:
        st = ch.Stats()
        for _ in range(max_idle + 1):
            ch.observe(st, X, [front_view])
            ctx.map_observe_dev(**_Obs(front_view).kw)
        _same_stats(ctx, st, n, "observed")
        rule = dict(RULE, max_idle=max_idle)
        want = _cull(ctx, st, M, X, rule, None, [], "idle")
        assert np.array_equal(want["remap"] < 0, is_back) and (want["n_idle"], want["n_ratio"], want["n_flagged"]) == (n // 2, 0, 0)
        assert np.array_equal(_bits(_points(ctx, want["n_kept"])), _bits(X[~is_back]))
        _same_stats(ctx, st, want["n_kept"], "after the cull")
        # one observe fewer would have kept them: the idle time must EXCEED max_idle
        assert ch.clause(0, 0, 0, max_idle, False, **rule) == ch.KEPT
    finally:
        ctx.close()


def test_the_map_serves_afterwards_like_a_fresh_context():
    torch = _torch()
    nq, nm = 300, 500
    Q, M, qpos, X = ph.make_case(nq, nm, seed=13)
    rng = np.random.RandomState(6)
    flagged = (rng.uniform(size=nm) < 0.3).astype(np.uint8)
    culled = _ctx(M, X)
    try:
        want = _cull(culled, ch.Stats(), M, X, RULE, flagged, [], "serve")
        fresh = _ctx(want["M"], want["X"])
        try:
            d_q, d_feat = _dev(Q), _dev(qpos)
            outs = []
            for ctx in (culled, fresh):
                m1 = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
                m2 = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
                best, second = torch.full((nq,), 7, dtype=torch.int16, device="cuda"), torch.full((nq,), 7, dtype=torch.int16, device="cuda")
                torch.cuda.synchronize()
                ctx.match_map_dev(d_q.data_ptr(), nq, 40, m1.data_ptr(), None)
                ctx.match_map_binned_dev(d_q=d_q.data_ptr(), nq=nq, cam=CAM, Rt=np.eye(3, 4), radius=3.0, threshold=40, d_match=m2.data_ptr(),
                                         d_best=best.data_ptr(), d_second=second.data_ptr(), d_feat=d_feat.data_ptr(), feat_stride=2)
                ctx.sync()
                outs.append([t.cpu().numpy() for t in (m1, m2, best, second)])
            for a, b in zip(*outs):
                assert np.array_equal(a, b)
            assert (outs[0][0] >= 0).sum() > 20 and (outs[0][1] >= 0).sum() > 20
            # and they are the uncut map's matches through the remap, wherever the row a query took survived
            st = ph.statement(Q, M, X, np.eye(3, 4), 3.0, 40, CAM, feat=qpos)
            took = st["match"] >= 0
            survived = took & (want["remap"][np.where(took, st["match"], 0)] >= 0)
            assert survived.sum() > 20 and np.array_equal(outs[0][1][survived], want["remap"][st["match"][survived]])
        finally:
            fresh.close()
    finally:
        culled.close()


def test_a_cull_makes_room_for_the_extension():
    """the scene of tests/test_gpu_map_extend.py in a context of MAP_N + 7 rows"""
    views, _, par = mh.main_case()
    par = {k: par[k] for k in ("band", "threshold", "max_distance")}
    cap = tme.MAP_N + 7
    ctx, M, X = tme._ctx(maxkp=cap)
    try:
        first, M2, X2 = tme._run(ctx, views[0], views[1], par, cap, tme.MAP_N, M, X, "room for 7")
        assert first["n_added"] == 7 and first["n_dropped"] > 0
        a, b = dict(views[0], track=first["track_a"]), dict(views[1], track=first["track_b"])
        full, _, _ = tme._run(ctx, a, b, par, cap, cap, M2, X2, "full map")
        assert full["n_added"] == 0 and full["n_dropped"] > 0                   # a second extension right away adds nothing
        # eight frames from view A's pose: the old rows are random points nothing near their projections tracks -- visible, never found --,
        # the seven new ones are found by the keypoints they came from
        st = ch.Stats()
        ov = dict(cam=a["cam"], Rt=a["Rt"], feat=a["feat"], track=a["track"], count=None, width=mh.W, height=mh.H, gate=3.0, margin=0.0)
        for _ in range(8):
            ch.observe(st, X2, [ov])
            ctx.map_observe_dev(**_Obs(ov).kw)
        _same_stats(ctx, st, cap, "eight frames")
        lists = [a["track"], b["track"]]
        want = _cull(ctx, st, M2, X2, RULE, None, lists, "cull")
        assert want["n_ratio"] > 20 and want["n_kept"] >= 7 and (want["remap"][tme.MAP_N:] >= 0).all()
        # the lists still name the right landmarks
        X_new = _points(ctx, want["n_kept"])
        assert np.array_equal(_bits(X_new), _bits(want["X"]))
        for old, new in zip(lists, want["lists"]):
            named = (old >= 0) & (old < cap)
            kept = named & (new >= 0)
            assert kept.sum() >= 7 and np.array_equal(_bits(X_new[new[kept]]), _bits(X2[old[kept]]))
            assert (new[~named] == -1).all() and (new[named & ~kept] == -1).all()
        # and the same extension finds room again: min(room, accepted), the number the statement gives
        a2, b2 = dict(a, track=want["lists"][0]), dict(b, track=want["lists"][1])
        again, _, _ = tme._run(ctx, a2, b2, par, cap, want["n_kept"], want["M"], want["X"], "after the cull")
        unbounded = mh.statement(a2, b2, par["band"], par["threshold"], par["max_distance"], want["n_kept"], 1 << 20)
        assert again["n_added"] == min(cap - want["n_kept"], unbounded["n_added"]) > 0
    finally:
        ctx.close()


def test_everything_dropped_leaves_the_extendable_empty_map():
    M, X = mh.make_map(65, 9)
    ctx = _ctx(M, X, maxkp=1024)
    try:
        want = _cull(ctx, ch.Stats(), M, X, RULE, np.ones(65, dtype=np.uint8), [np.arange(-1, 66, dtype=np.int32)], "all dropped")
        assert want["n_kept"] == 0 and (want["lists"][0] == -1).all()
        assert ctx.map_stats()["rows"] == 0
        views, _ = mh.make_views([200, 200], seed=61, map_n=0)
        st, _, _ = tme._run(ctx, views[0], views[1], tme.PAR, 1024, 0, np.zeros((0, 64), np.uint8), np.zeros((0, 3)), "empty map")
        assert st["n_added"] >= 5
    finally:
        ctx.close()


def test_points_only_context_culls_points():
    from coloc_amd import CLCError, Context, abi
    M, X = mh.make_map(300, 12)
    rng = np.random.RandomState(14)
    remap, kept = ch.remap(rng.uniform(size=300) < 0.4)
    loc = Context(device=0, detector=False, maxkp=64)
    ctx = _ctx(M, X)
    try:
        loc.set_map_points(X)
        for bad in (remap[:-1], np.concatenate([remap, [-1]]), np.where(remap == 3, 4, remap), remap[::-1], np.where(remap == -1, -2, remap)):
            with pytest.raises(CLCError) as e:
                loc.cull_map_points(bad)
            assert e.value.status == abi.CLC_ERR_BAD_ARG
        assert np.array_equal(_bits(_points(loc, 300)), _bits(X))                # refused: as it was
        loc.cull_map_points(remap)
        assert np.array_equal(_bits(_points(loc, kept)), _bits(X[remap >= 0]))
        loc.append_map_points(X[:5])                                             # and the extension's companion still follows
        assert np.array_equal(_bits(_points(loc, kept + 5)), _bits(np.vstack([X[remap >= 0], X[:5]])))
        loc.cull_map_points(np.full(kept + 5, -1, dtype=np.int32))               # everything: no points
        loc.cull_map_points(np.zeros(0, dtype=np.int32))
        loc.append_map_points(X[:3])
        assert np.array_equal(_bits(_points(loc, 3)), _bits(X[:3]))
        with pytest.raises(CLCError) as e:                                       # a context that holds rows is culled by clc_map_cull_dev alone
            ctx.cull_map_points(remap)
        assert e.value.status == abi.CLC_ERR_STATE
        tme._check_map(ctx, M, X, "after the refusal")
    finally:
        loc.close()
        ctx.close()


def test_errors_return_their_codes_and_leave_map_and_statistics():
    from coloc_amd import CLCError, Context, abi
    BAD, STATE = abi.CLC_ERR_BAD_ARG, abi.CLC_ERR_STATE
    M, X = mh.make_map(tme.MAP_N, 1)
    ctx = _ctx(M, X, maxkp=2048)
    try:
        rng = np.random.RandomState(15)
        rows = rng.choice(tme.MAP_N, 30).astype(np.int32)
        view = dict(cam=CAM, Rt=np.eye(3, 4), feat=ph.project(np.eye(3, 4), CAM, X)[0][rows], track=rows, count=None, width=640, height=480, gate=2.0,
                    margin=0.0)
        st = ch.Stats()
        ch.observe(st, X, [view])
        o = _Obs(view)
        ctx.map_observe_dev(**o.kw)
        _same_stats(ctx, st, tme.MAP_N, "planted")
        assert sum(st.found) > 10
        d_list = _dev(np.arange(tme.MAP_N, dtype=np.int32))

        def observe_refused(code, views=None, **change):
            with pytest.raises(CLCError) as e:
                if views is not None:
                    ctx.map_observe_batch_dev(views)
                else:
                    ctx.map_observe_dev(**{k: v for k, v in dict(o.kw, **change).items() if v is not Ellipsis})
            assert e.value.status == code, (e.value.status, code, change)

        def cull_refused(code, **change):
            with pytest.raises(CLCError) as e:
                ctx.map_cull_dev(**dict(RULE, **change))
            assert e.value.status == code, (e.value.status, code, change)

        observe_refused(BAD, n=-1)
        for gate in (-1.0, float("inf"), float("nan"), 1.0e30):
            observe_refused(BAD, gate=gate)
        for margin in (-0.5, float("inf"), float("nan")):
            observe_refused(BAD, margin=margin)
        observe_refused(BAD, width=0)
        observe_refused(BAD, height=-3)
        observe_refused(BAD, cam=(0.0, 320.0, 240.0, 0, 0, 0))
        observe_refused(BAD, d_kps=o.feat.data_ptr())                            # both position forms
        observe_refused(BAD, d_feat=Ellipsis, feat_stride=Ellipsis)              # neither
        observe_refused(BAD, Rt=np.full((3, 4), np.nan))
        observe_refused(BAD, d_track=o.kw["d_track"] + 2)
        observe_refused(BAD, views=[o.kw] * (abi.MAX_BATCH + 1))
        observe_refused(BAD, views=[o.kw, dict(o.kw, gate=-1.0)])                # the second view is refused: the first one did not run
        cull_refused(BAD, den=0)
        cull_refused(BAD, den=-4)
        cull_refused(BAD, num=-1)
        cull_refused(BAD, min_visible=0)
        cull_refused(BAD, lists=[(d_list.data_ptr(), 4)] * (abi.MAX_BATCH + 1))
        cull_refused(BAD, lists=[(d_list.data_ptr(), -1)])
        cull_refused(BAD, lists=[(None, 4)])
        cull_refused(BAD, lists=[(d_list.data_ptr() + 2, 4)])
        # nothing was enqueued: the map, the statistics, the epoch and the list are as they were
        _same_stats(ctx, st, tme.MAP_N, "after the refusals")
        tme._check_map(ctx, M, X, "after the refusals")
        assert np.array_equal(d_list.cpu().numpy(), np.arange(tme.MAP_N))
        # the context's state: no map, points without rows, rows without points, points that are not the rows
        bare = Context(device=0, detector=False, maxkp=256)
        try:
            def state(what):
                for call in (lambda: bare.map_observe_dev(**o.kw), lambda: bare.map_cull_dev(**RULE)):
                    with pytest.raises(CLCError) as e:
                        call()
                    assert e.value.status == STATE, what
            state("no map")
            bare.set_map_points(X)
            state("points only")
            bare.set_map(M)
            bare.set_map_points(np.zeros((0, 3)))
            state("rows only")
            bare.set_map_points(X[:-1])
            state("fewer points than rows")
            bare.set_map_points(np.vstack([X, X[:3]]))
            state("more points than rows")
            bare.set_map_points(X)                                               # whole again: untouched by the refusals
            tme._check_map(bare, M, X, "bare")
            assert bare.map_stats()["epoch"] == 0
        finally:
            bare.close()
        nomat = Context(device=0, width=320, height=240, maxkp=256, matcher=False)      # a context without matcher options
        try:
            for call in (lambda: nomat.map_observe_dev(**o.kw), lambda: nomat.map_cull_dev(**RULE)):
                with pytest.raises(CLCError) as e:
                    call()
                assert e.value.status == STATE
        finally:
            nomat.close()
        # and the context still works
        ch.observe(st, X, [view])
        ctx.map_observe_dev(**o.kw)
        _same_stats(ctx, st, tme.MAP_N, "after the refusals, observed")
    finally:
        ctx.close()

"""The map extended in place on the device (include/coloc_hip.h: clc_map_extend_dev, clc_map_extend_batch_dev, clc_append_map_points)
against the host statement (tests/map_extend_host.py).  Every comparison is EXACT: the lists, the points through their uint64 view, the
counts, the d_track lists as the call leaves them, the map's new descriptor rows (Hamming distance 0 from A's rows) and its old rows
and points.

Shapes: the mask, point and filter kernels run 256 threads a workgroup with one thread per query, the append is ONE workgroup of 1 024
that walks the queries in passes, so the shapes straddle a wave (63, 65), several workgroups (400) and the second compaction pass
(1 100); (0, 5), (5, 0) and (1, 1) are the degenerate ends.  Maps stay below 1 200 rows."""
import os

import numpy as np
import pytest

import map_extend_host as mh
import test_gpu_map_guided as tg                     # _dev, _torch

pytestmark = pytest.mark.gpu

_dev, _torch = tg._dev, tg._torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_N = 40
SHAPES = [(0, 5), (5, 0), (1, 1), (63, 65), (400, 400), (1100, 1100)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _ctx(maxkp=2048, map_n=MAP_N, seed=1):
    """a context whose map holds map_n random rows and points -> (ctx, M, X)"""
    from coloc_amd import Context
    ctx = Context(device=0, detector=False, maxkp=maxkp)
    M, X = mh.make_map(map_n, seed)
    ctx.set_map(M)
    ctx.set_map_points(X)
    return ctx, M, X


class _View:
    """device copies of one view: descriptors, positions (float rows of `stride`, or keypoints), the count word, the d_track list (one
    poisoned entry behind it); n may be 0 (the buffers then hold one unused entry)"""

    def __init__(self, v, stride=4, track=True):
        self.v, self.n = v, len(v["desc"])
        n = self.n
        self.keep = [_dev(v["desc"] if n else np.zeros((1, 64), np.uint8))]
        side = {}
        if v.get("kps") is not None:
            d = _dev(v["kps"] if n else np.zeros(1, dtype=v["kps"].dtype))
            side["d_kps"] = d.data_ptr()
        else:
            f = np.full((max(n, 1), stride), 7.0, dtype=np.float32)
            f[:n, :2] = v["feat"]
            d = _dev(f)
            side["d_feat"], side["feat_stride"] = d.data_ptr(), stride
        self.keep.append(d)
        if v.get("count") is not None:
            d = _dev(np.array([v["count"], v["count"] + 17], dtype=np.uint32).view(np.int32))
            self.keep.append(d)
            side["d_count"] = d.data_ptr()
        self.track = None
        if track and v.get("track") is not None:
            self.track = _dev(np.concatenate([np.asarray(v["track"], dtype=np.int32), np.array([-7], dtype=np.int32)]))
            side["d_track"] = self.track.data_ptr()
        self.kw = dict(d_desc=self.keep[0].data_ptr(), n=n, cam=v["cam"], Rt=v["Rt"], **side)

    def tracks(self):
        t = self.track.cpu().numpy()
        assert t[self.n] == -7                                                  # nothing is written past the list
        return t[:self.n]


def _lists(n):
    torch = _torch()
    q = torch.full((max(n, 1) + 1,), -7, dtype=torch.int32, device="cuda")
    t = torch.full((max(n, 1) + 1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return q, t


def _map_dump(ctx, rows):
    """the context's map against the expected descriptor rows: (match, best) of `rows` against the map -- match_map_guided_dev under the
    identity pose with a radius that holds every landmark in front of it -- and the map's points in row order (track_build_dev of the
    identity list)"""
    torch = _torch()
    n = len(rows)
    d_q, d_feat = _dev(rows), _dev(np.zeros((n, 2), dtype=np.float32))
    match = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    best = torch.full((n,), 7, dtype=torch.int16, device="cuda")
    ident = _dev(np.arange(n, dtype=np.int32))
    dX, dx = torch.zeros((3 * n,), dtype=torch.float64, device="cuda"), torch.zeros((2 * n,), dtype=torch.float64, device="cuda")
    dn = torch.zeros((1,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.match_map_guided_dev(d_q=d_q.data_ptr(), nq=n, cam=mh.CAM, Rt=np.eye(3, 4), radius=1.0e5, threshold=0, d_match=match.data_ptr(),
                             d_best=best.data_ptr(), d_feat=d_feat.data_ptr(), feat_stride=2)
    ctx.track_build_dev(dX.data_ptr(), dx.data_ptr(), None, None, dn.data_ptr(), d_match=ident.data_ptr(), nq=n, cam=mh.CAM, d_feat=d_feat.data_ptr(),
                        feat_stride=2)
    ctx.sync()
    assert int(dn.cpu().numpy()[0]) == n
    return match.cpu().numpy(), best.cpu().numpy().view(np.uint16), dX.cpu().numpy().reshape(-1, 3)


def _check_map(ctx, M, X, what, doubled=False):
    """the context's map is exactly the rows M with the points X: every row at distance 0 from its own row, the points bit for bit.
    doubled: M holds equal rows on purpose -- such a row ties with its twin, so it is answered -1"""
    if len(M) == 0:
        return
    match, best, got_X = _map_dump(ctx, M)
    assert (best == 0).all(), (what, "map rows")
    if doubled:
        twin = np.array([(M == r).all(1).sum() > 1 for r in M])
        assert (match[twin] == -1).all() and twin.any()
        assert np.array_equal(match[~twin], np.arange(len(M))[~twin]), (what, "map rows")
    else:
        assert np.array_equal(match, np.arange(len(M))), (what, "map rows")
    assert np.array_equal(_bits(got_X), _bits(X)), (what, "map points")


def _run(ctx, a, b, par, maxkp, map_n, M, X, what, update_tracks=True, stride=4, doubled=False):
    """one job on the device against the statement, the whole map checked afterwards -> (statement, the map's rows, points)"""
    st = mh.statement(a, b, par["band"], par["threshold"], par["max_distance"], map_n, maxkp, update_tracks)
    va, vb = _View(a, stride), _View(b, stride)
    dq, dt = _lists(len(a["desc"]))
    got = ctx.extend_map(va.kw, vb.kw, par["band"], par["threshold"], par["max_distance"], update_tracks=update_tracks, d_new_q=dq.data_ptr(),
                         d_new_t=dt.data_ptr())
    _same(got, st, map_n, what)
    n = st["n_added"]
    hq, ht = dq.cpu().numpy(), dt.cpu().numpy()
    assert np.array_equal(hq[:n], st["new_q"]) and np.array_equal(ht[:n], st["new_t"]) and (hq[n:] == -7).all() and (ht[n:] == -7).all(), what
    if va.track is not None:
        assert np.array_equal(va.tracks(), st["track_a"]), (what, "d_track_a")
    if vb.track is not None:
        assert np.array_equal(vb.tracks(), st["track_b"]), (what, "d_track_b")
    M2 = np.vstack([M, a["desc"][st["new_q"]]]) if n else M
    X2 = np.vstack([X, st["X"]]) if n else X
    _check_map(ctx, M2, X2, what, doubled)
    return st, M2, X2


def _same(got, st, map_n, what):
    assert got["status"] == 0 and got["map_n_before"] == map_n, what
    assert np.array_equal(_bits(got["F"]), _bits(st["F"])), (what, "F")
    assert (got["n_guided"], got["n_added"], got["n_dropped"]) == (st["n_guided"], st["n_added"], st["n_dropped"]), \
        (what, got["n_guided"], got["n_added"], got["n_dropped"], st["n_guided"], st["n_added"], st["n_dropped"])
    assert np.array_equal(got["new_q"], st["new_q"]) and np.array_equal(got["new_t"], st["new_t"]), (what, "lists")
    assert np.array_equal(_bits(got["X"]), _bits(st["X"])), (what, "X")


PAR = dict(band=mh.BAND, threshold=mh.THRESHOLD, max_distance=mh.CAP)


@pytest.mark.parametrize("na,nb", SHAPES)
def test_shapes_equal_the_statement(na, nb):
    ctx, M, X = _ctx()
    try:
        views, _ = mh.make_views([na, nb], seed=100 + na)
        st, _, _ = _run(ctx, views[0], views[1], PAR, 2048, MAP_N, M, X, (na, nb))
        if (na, nb) == (400, 400):
            assert all(st["classes"][c] >= 5 for c in mh.CLASSES), st["classes"]
        if na > 1024:
            assert (st["new_q"] < 1024).any() and (st["new_q"] >= 1024).any()    # both compaction passes append
        if min(na, nb) == 0:
            assert st["n_added"] == 0
    finally:
        ctx.close()


def test_row_forms_distortion_and_device_counts():
    ctx, M, X = _ctx()
    try:
        views, _ = mh.make_views([300, 320], seed=21)
        # positions as detector keypoints on both sides
        st, M, X = _run(ctx, mh.with_kps(views[0]), mh.with_kps(views[1]), PAR, 2048, MAP_N, M, X, "keypoints")
        assert st["n_added"] >= 5
        # a distorted camera on both sides, float rows of another stride
        views, _ = mh.make_views([300, 320], seed=22, cams=[mh.CAM_K1, mh.CAM_K1])
        n0 = len(M)
        st, M, X = _run(ctx, views[0], views[1], PAR, 2048, n0, M, X, "distorted", stride=3)
        assert st["n_added"] >= 5
        plain = mh.statement(dict(views[0], cam=mh.CAM), dict(views[1], cam=mh.CAM), PAR["band"], PAR["threshold"], PAR["max_distance"], n0, 2048)
        assert not np.array_equal(plain["new_q"], st["new_q"]) or not np.array_equal(_bits(plain["X"]), _bits(st["X"]))      # k1 was applied
        # device-side counts that clip both views
        views, _ = mh.make_views([300, 320], seed=23)
        full = mh.statement(views[0], views[1], PAR["band"], PAR["threshold"], PAR["max_distance"], len(M), 2048)
        views[0]["count"], views[1]["count"] = 240, 250
        st, M, X = _run(ctx, views[0], views[1], PAR, 2048, len(M), M, X, "counts")
        assert 5 <= st["n_added"] < full["n_added"] and (st["new_q"] < 240).all() and (st["new_t"] < 250).all()
    finally:
        ctx.close()


def test_capacity_truncates_to_a_prefix_and_a_full_map_takes_nothing():
    views, _, par = mh.main_case()
    par = {k: par[k] for k in ("band", "threshold", "max_distance")}
    unbounded = mh.statement(views[0], views[1], mh.BAND, mh.THRESHOLD, mh.CAP, MAP_N, 4096)
    assert unbounded["n_added"] > 12
    ctx, M, X = _ctx(maxkp=MAP_N + 7)
    try:
        st, M2, X2 = _run(ctx, views[0], views[1], par, MAP_N + 7, MAP_N, M, X, "room for 7")
        assert st["n_added"] == 7 and st["n_dropped"] == unbounded["n_added"] - 7
        assert np.array_equal(st["new_q"], unbounded["new_q"][:7]) and np.array_equal(st["new_t"], unbounded["new_t"][:7])
        assert (st["track_a"] >= MAP_N).sum() == 7 and (st["track_b"] >= MAP_N).sum() == 7          # d_track_* updated for those 7 only
        # the map is full now: nothing is written, CLC_OK, everything accepted is dropped and counted
        views[0]["track"], views[1]["track"] = st["track_a"], st["track_b"]
        full, _, _ = _run(ctx, views[0], views[1], par, MAP_N + 7, MAP_N + 7, M2, X2, "full map")
        assert full["n_added"] == 0 and full["n_dropped"] == unbounded["n_added"] - 7
        assert np.array_equal(full["track_a"], st["track_a"]) and np.array_equal(full["track_b"], st["track_b"])
    finally:
        ctx.close()


def test_update_tracks_off_leaves_the_lists_and_on_makes_a_second_call_add_nothing():
    ctx, M, X = _ctx()
    try:
        views, _ = mh.make_views([300, 300], seed=31)
        st, M, X = _run(ctx, views[0], views[1], PAR, 2048, MAP_N, M, X, "off", update_tracks=False)
        assert st["n_added"] >= 5 and np.array_equal(st["track_a"], views[0]["track"]) and np.array_equal(st["track_b"], views[1]["track"])
        # off: the same call again plants every landmark a second time
        again, M, X = _run(ctx, views[0], views[1], PAR, 2048, len(M), M, X, "off, again", update_tracks=False, doubled=True)
        assert again["n_added"] == st["n_added"]
        # on, then the identical call on the lists the first one left: nothing is added
        n0 = len(M)
        va, vb = _View(views[0]), _View(views[1])
        first = ctx.extend_map(va.kw, vb.kw, **PAR)
        want = mh.statement(views[0], views[1], mh.BAND, mh.THRESHOLD, mh.CAP, n0, 2048)
        _same(first, want, n0, "on")
        second = ctx.extend_map(va.kw, vb.kw, **PAR)
        assert second["n_added"] == 0 and second["n_dropped"] == 0 and second["map_n_before"] == n0 + first["n_added"]
        assert np.array_equal(va.tracks(), want["track_a"]) and np.array_equal(vb.tracks(), want["track_b"])
        # views without a list: no row is tracked, nothing to update
        na_, nb_ = _View(views[0], track=False), _View(views[1], track=False)
        bare = ctx.extend_map(na_.kw, nb_.kw, **PAR)
        none = mh.statement(dict(views[0], track=None), dict(views[1], track=None), mh.BAND, mh.THRESHOLD, mh.CAP, second["map_n_before"], 2048)
        _same(bare, none, second["map_n_before"], "no lists")
    finally:
        ctx.close()


def test_batch_of_three_equals_the_single_calls_in_that_order():
    """A -> B, A -> C, B -> C: a job sees the rows and the d_track updates of the jobs before it, so the second and third depend on the
    device-side running count and on the lists the first one left"""
    views, _ = mh.make_views([320, 300, 310], seed=41)
    order = [(0, 1), (0, 2), (1, 2)]
    # the statement, job after job
    tracks = [v["track"].copy() for v in views]
    want, rows = [], MAP_N
    for ia, ib in order:
        st = mh.statement(dict(views[ia], track=tracks[ia]), dict(views[ib], track=tracks[ib]), mh.BAND, mh.THRESHOLD, mh.CAP, rows, 2048)
        tracks[ia], tracks[ib] = st["track_a"], st["track_b"]
        rows += st["n_added"]
        want.append(st)
    assert all(st["n_added"] >= 5 for st in want)
    assert want[1]["n_added"] < mh.statement(views[0], views[2], mh.BAND, mh.THRESHOLD, mh.CAP, MAP_N, 2048)["n_added"]      # job 1 saw job 0's updates
    batch_ctx, M, X = _ctx()
    single_ctx, _, _ = _ctx()
    try:
        dv = [_View(v) for v in views]
        got = batch_ctx.extend_map_batch([dict(view_a=dv[ia].kw, view_b=dv[ib].kw, **PAR) for ia, ib in order])
        sv = [_View(v) for v in views]
        single = [single_ctx.extend_map(sv[ia].kw, sv[ib].kw, **PAR) for ia, ib in order]
        n = MAP_N
        for k, (g, s, st) in enumerate(zip(got, single, want)):
            _same(g, st, n, ("batch == statement", k))
            _same(s, st, n, ("single == statement", k))
            n += st["n_added"]
        for k in range(3):
            assert np.array_equal(dv[k].tracks(), tracks[k]) and np.array_equal(sv[k].tracks(), tracks[k]), k
        M2 = np.vstack([M] + [views[ia]["desc"][st["new_q"]] for (ia, _), st in zip(order, want)])
        X2 = np.vstack([X] + [st["X"] for st in want])
        _check_map(batch_ctx, M2, X2, "batch")
        _check_map(single_ctx, M2, X2, "single")
        assert batch_ctx.extend_map_batch([]) == []                              # nothing to do
    finally:
        batch_ctx.close()
        single_ctx.close()


def test_the_context_serves_the_extended_map():
    torch = _torch()
    ctx, M, X = _ctx()
    try:
        views, _ = mh.make_views([400, 400], seed=51)
        a = views[0]
        st, M2, X2 = _run(ctx, a, views[1], PAR, 2048, MAP_N, M, X, "extend")
        n, na = st["n_added"], len(a["desc"])
        assert n >= 20
        rows = MAP_N + np.arange(n, dtype=np.int32)
        # clc_match_map_dev of A's frame: the appended rows of A come back as their new map rows
        d_q, d_feat = _dev(a["desc"]), _dev(np.ascontiguousarray(a["feat"]))
        d_match = torch.full((na,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.match_map_dev(d_q.data_ptr(), na, 40, d_match.data_ptr(), None)
        ctx.sync()
        m = d_match.cpu().numpy()
        assert np.array_equal(m[st["new_q"]], rows)
        # clc_track_build_dev of that match: their X, bit for bit
        dX, dx = torch.zeros((3 * na,), dtype=torch.float64, device="cuda"), torch.zeros((2 * na,), dtype=torch.float64, device="cuda")
        dqy, dmp = torch.full((na,), -7, dtype=torch.int32, device="cuda"), torch.full((na,), -7, dtype=torch.int32, device="cuda")
        dn = torch.zeros((1,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.track_build_dev(dX.data_ptr(), dx.data_ptr(), dqy.data_ptr(), dmp.data_ptr(), dn.data_ptr(), d_match=d_match.data_ptr(), nq=na, cam=a["cam"],
                            d_feat=d_feat.data_ptr(), feat_stride=2)
        ctx.sync()
        nt = int(dn.cpu().numpy()[0])
        tq, tm, tX = dqy.cpu().numpy()[:nt], dmp.cpu().numpy()[:nt], dX.cpu().numpy().reshape(-1, 3)[:nt]
        assert np.array_equal(tq, np.nonzero(m >= 0)[0]) and np.array_equal(_bits(tX), _bits(X2[tm]))
        sel = np.isin(tq, st["new_q"])
        assert sel.sum() == n and np.array_equal(_bits(tX[sel]), _bits(st["X"]))
        # the binned match agrees with the guided match on the extended map, under A's pose
        out = []
        for entry in (ctx.match_map_binned_dev, ctx.match_map_guided_dev):
            mm = torch.full((na,), -7, dtype=torch.int32, device="cuda")
            bb = torch.full((na,), 7, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            entry(d_q=d_q.data_ptr(), nq=na, cam=a["cam"], Rt=a["Rt"], radius=6.0, threshold=40, d_match=mm.data_ptr(), d_best=bb.data_ptr(),
                  d_feat=d_feat.data_ptr(), feat_stride=2)
            ctx.sync()
            out.append((mm.cpu().numpy(), bb.cpu().numpy()))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
        assert np.array_equal(out[0][0][st["new_q"]], rows)                     # every new landmark projects onto the keypoint it came from
        assert ctx.map_binned_plan(a["cam"], 6.0)["plan"] == 1
    finally:
        ctx.close()


def test_an_empty_map_is_extendable():
    """map_n == 0 with its points cleared (what a build without an accepted point leaves) counts as an empty map"""
    from coloc_amd import Context
    ctx = Context(device=0, detector=False, maxkp=1024)
    try:
        ctx.set_map(np.zeros((0, 64), np.uint8))
        ctx.set_map_points(np.zeros((0, 3)))
        views, _ = mh.make_views([200, 200], seed=61, map_n=0)
        st, _, _ = _run(ctx, views[0], views[1], PAR, 1024, 0, np.zeros((0, 64), np.uint8), np.zeros((0, 3)), "empty map")
        assert st["n_added"] >= 5
    finally:
        ctx.close()


def test_points_only_context_appends_points():
    """clc_append_map_points on a context that holds only points, then clc_track_build_dev: the same X as the extended matcher context"""
    from coloc_amd import CLCError, Context, abi
    torch = _torch()
    ctx, M, X = _ctx()
    loc = Context(device=0, detector=False, maxkp=2048)
    try:
        views, _ = mh.make_views([300, 300], seed=71)
        st, M2, X2 = _run(ctx, views[0], views[1], PAR, 2048, MAP_N, M, X, "extend")
        assert st["n_added"] >= 5
        loc.set_map_points(X)
        loc.append_map_points(st["X"])
        loc.append_map_points(np.zeros((0, 3)))
        n = len(X2)
        ident, d_feat = _dev(np.arange(n, dtype=np.int32)), _dev(np.zeros((n, 2), dtype=np.float32))
        dX, dx = torch.zeros((3 * n,), dtype=torch.float64, device="cuda"), torch.zeros((2 * n,), dtype=torch.float64, device="cuda")
        dn = torch.zeros((1,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        loc.track_build_dev(dX.data_ptr(), dx.data_ptr(), None, None, dn.data_ptr(), d_match=ident.data_ptr(), nq=n, cam=mh.CAM, d_feat=d_feat.data_ptr(),
                            feat_stride=2)
        loc.sync()
        assert int(dn.cpu().numpy()[0]) == n and np.array_equal(_bits(dX.cpu().numpy().reshape(-1, 3)), _bits(X2))
        # a context without any points takes them as its first; a context that holds map rows is refused
        fresh = Context(device=0, detector=False, maxkp=64)
        try:
            fresh.append_map_points(st["X"])
            fresh.append_map_points(X)
        finally:
            fresh.close()
        with pytest.raises(CLCError) as e:
            ctx.append_map_points(st["X"])
        assert e.value.status == abi.CLC_ERR_STATE
        _check_map(ctx, M2, X2, "after the refusal")
    finally:
        ctx.close()
        loc.close()


def test_argument_errors_return_their_codes_and_leave_the_map():
    from coloc_amd import CLCError, Context, abi
    ctx, M, X = _ctx()
    try:
        views, _ = mh.make_views([100, 100], seed=81)
        va, vb = _View(views[0]), _View(views[1])

        def refused(code, view_a=None, view_b=None, **par):
            p = dict(PAR)
            p.update(par)
            with pytest.raises(CLCError) as e:
                ctx.extend_map(view_a or va.kw, view_b or vb.kw, **p)
            assert e.value.status == code, (e.value.status, code, par)

        BAD, STATE, CAPACITY = abi.CLC_ERR_BAD_ARG, abi.CLC_ERR_STATE, abi.CLC_ERR_CAPACITY
        refused(BAD, view_a=dict(va.kw, d_desc=None))                                  # a null block
        refused(BAD, view_b=dict(vb.kw, n=-1))
        refused(BAD, view_a=dict(va.kw, d_kps=va.keep[1].data_ptr()))                  # both position forms
        refused(BAD, view_b={k: v for k, v in vb.kw.items() if k not in ("d_feat", "feat_stride")})      # neither
        refused(BAD, view_a=dict(va.kw, d_desc=va.kw["d_desc"] + 8))                   # misaligned rows
        refused(BAD, view_a=dict(va.kw, d_track=va.kw["d_track"] + 2))
        refused(BAD, view_b=dict(vb.kw, cam=(0.0, 320.0, 240.0, 0, 0, 0)))             # a non-positive focal
        refused(BAD, band=0.0)
        refused(BAD, band=float("inf"))
        refused(BAD, band=float("nan"))
        refused(BAD, max_distance=-1)
        refused(BAD, max_distance=513)
        refused(BAD, d_new_q=va.kw["d_track"] + 2)
        refused(CAPACITY, view_a=dict(va.kw, n=(1 << 22) + 1))
        refused(CAPACITY, view_b=dict(vb.kw, n=(1 << 22) + 1))
        with pytest.raises(CLCError) as e:
            ctx.extend_map_batch([dict(view_a=va.kw, view_b=vb.kw, **PAR)] * (abi.MAX_TRACK_PAIRS + 1))
        assert e.value.status == BAD
        with pytest.raises(CLCError) as e:                                             # the second job is refused: the first one did not run
            ctx.extend_map_batch([dict(view_a=va.kw, view_b=vb.kw, **PAR), dict(view_a=va.kw, view_b=vb.kw, **dict(PAR, band=-1.0))])
        assert e.value.status == BAD
        # nothing was enqueued: the lists and the map are as they were
        assert np.array_equal(va.tracks(), views[0]["track"]) and np.array_equal(vb.tracks(), views[1]["track"])
        _check_map(ctx, M, X, "after the refusals")
        # the context's state: no map, points without rows, rows without points, more rows than points
        bare = Context(device=0, detector=False, maxkp=256)
        try:
            def state(what):
                with pytest.raises(CLCError) as e:
                    bare.extend_map(va.kw, vb.kw, **PAR)
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
        finally:
            bare.close()
        nomat = Context(device=0, width=320, height=240, maxkp=256, matcher=False)      # a context without matcher options
        try:
            with pytest.raises(CLCError) as e:
                nomat.extend_map(va.kw, vb.kw, **PAR)
            assert e.value.status == STATE
        finally:
            nomat.close()
        # and the context still works
        got = ctx.extend_map(va.kw, vb.kw, **PAR)
        _same(got, mh.statement(views[0], views[1], mh.BAND, mh.THRESHOLD, mh.CAP, MAP_N, 2048), MAP_N, "after the refusals")
    finally:
        ctx.close()

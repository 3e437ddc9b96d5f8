"""The map replaced on the device at the old map's scale (include/coloc_hip.h: clc_map_align_dev, clc_map_update_batch_dev).

Descriptors: 512-bit rows are random; a "common" old row is a new row with at most 8 flipped bits.  Unrelated random rows lie about
256 +- 11 bits apart, so second - best > 60 holds exactly for the intended matches -- which every case ASSERTS on the CPU with the oracle
K2NN before it touches the GPU: the expected list is the oracle's, not an assumption.
Comparison rule: integers (match, counts, status) are compared EXACTLY with tests/map_update_host.py; the scale and every point are
compared BIT FOR BIT with the host build of inter_math.h / map_math.h (tests/host/map_update_lib.cpp)."""
import numpy as np
import pytest

import map_update_host as mu
import test_gpu_map_build as mb
import track_host
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

_ORACLE = []


def _oracle():
    if not _ORACLE:
        _ORACLE.append(Oracle())
    return _ORACLE[0]


def _flip(rows, rng, flips=8):
    d = rows.copy()
    for _ in range(flips):
        d[np.arange(len(d)), rng.integers(0, 64, len(d))] ^= (1 << rng.integers(0, 8, len(d))).astype(np.uint8)
    return d


def _points(rng, n):
    return np.stack([rng.uniform(-5, 5, n), rng.uniform(-3, 3, n), rng.uniform(6, 20, n)], 1)


def _case(n_old, n_new, q, t, seed, true_scale=2.5, block_rows=None, old_X=None, new_X=None, old_desc=None):
    """an old map of n_old rows and a new one of n_new: old row q[k] and new row t[k] are near-copies of one another, every other row is
    random; the new rows lie at `rows` of a block of block_rows (a permutation's head) or are the block.  old_desc given: the old map's
    rows as they are, the new rows copied from them.  The oracle confirms the intended matches."""
    rng = np.random.default_rng(seed)
    q, t = np.asarray(q, dtype=np.int64), np.asarray(t, dtype=np.int64)
    block = rng.integers(0, 256, (block_rows or n_new, 64), dtype=np.uint8)
    rows = rng.permutation(block_rows)[:n_new].astype(np.int32) if block_rows else np.arange(n_new, dtype=np.int32)
    intended = np.full(n_old, -1, dtype=np.int32)
    intended[q] = t
    if old_desc is None:
        old_desc = rng.integers(0, 256, (n_old, 64), dtype=np.uint8)
        if len(q):
            old_desc[q] = _flip(block[rows[t]], rng)
    else:
        block[rows[t]] = _flip(old_desc[q], rng)
    new_desc = np.ascontiguousarray(block[rows])
    if new_X is None:
        new_X = _points(rng, n_new)
    if old_X is None:
        old_X = _points(rng, n_old) * true_scale
        if len(q):
            old_X[q] = new_X[t] * true_scale + rng.normal(0, 0.01, (len(q), 3))
    got = _oracle().k2nn(old_desc, new_desc, 60) if n_old and n_new else intended
    assert np.array_equal(got, intended), int((got != intended).sum())
    c = dict(n_old=n_old, n_new=n_new, old_desc=old_desc, old_X=np.ascontiguousarray(old_X), block=block, rows=rows, new_desc=new_desc,
             new_X=np.ascontiguousarray(new_X), match=intended)
    c["want"] = mu.align(c["old_X"], c["new_X"], intended)
    return c


def _install_old(ctx, c):
    ctx.set_map(c["old_desc"])
    ctx.set_map_points(c["old_X"])


def _align(ctx, c, use_rows=True, install=True, **kw):
    """the call on device copies of the case's new map -> (result, the device tensors, kept alive)"""
    if use_rows:
        d_desc, d_rows = mb._dev(c["block"]), mb._dev(c["rows"])
    else:
        d_desc, d_rows = mb._dev(c["new_desc"]), None
    d_X = mb._dev(c["new_X"])
    r = ctx.map_align_dev(d_desc.data_ptr(), d_X.data_ptr(), c["n_new"], d_rows=None if d_rows is None else d_rows.data_ptr(), install=install, **kw)
    ctx.sync()
    assert np.array_equal(mb._bits(d_X.cpu().numpy()), mb._bits(c["new_X"]))           # d_X itself is not written
    return r, (d_desc, d_rows, d_X)


def _check(got, want, n_old, what):
    assert got["n_old"] == n_old, (what, got["n_old"])
    assert np.array_equal(got["match"], want["match"]), (what, int((got["match"] != want["match"]).sum()))
    assert (got["n_common"], got["n_terms"], got["status"]) == (want["n_common"], want["n_terms"], want["status"]), (what, got, want["n_common"], want["n_terms"], want["status"])
    assert np.array_equal(mb._bits(np.float64(got["scale"])), mb._bits(np.float64(want["scale"]))), (what, got["scale"], want["scale"])
    assert np.array_equal(mb._bits(got["X"]), mb._bits(want["X"])), (what, int((mb._bits(got["X"]) != mb._bits(want["X"])).sum()))


def _frame(desc, X, seed, n=500):
    """a frame that sees the first n landmarks of a map (desc rows, points X) from the origin: near-copies of the rows, the points'
    pixels -> (d_q, nq, d_feat, cam)"""
    rng = np.random.default_rng(seed)
    n = min(n, len(desc))
    cam = mb.F0 + track_host.DISTORTIONS[0]
    px = X[:n, :2] / X[:n, 2:3] * cam[0] + np.array(cam[1:3])
    feat = np.zeros((n, 4), dtype=np.float32)
    feat[:, :2] = mb._distort(px + rng.normal(0, 0.2, (n, 2)), cam)
    feat[:, 2] = 7.0
    return mb._dev(_flip(desc[:n], rng, 5)), n, mb._dev(feat), cam


def _answer(ctx, frame):
    d_q, nq, d_feat, cam = frame
    return mb._frame_against_map(ctx, d_q, nq, d_feat, cam)


def _serves_like_host_map(ctx, desc, X, what, seed=77):
    """the context answers a frame exactly as a second context given the rows and points through set_map + set_map_points"""
    ref = mb._ctx()
    try:
        ref.set_map(desc)
        ref.set_map_points(X)
        frame = _frame(desc, X, seed)
        a, b = _answer(ctx, frame), _answer(ref, frame)
        mb._same_frame(a, b, what)
        return a
    finally:
        ref.close()


def _spread_commons(n_old, n_new, n_common, seed):
    rng = np.random.default_rng(seed)
    q = np.sort(rng.choice(n_old, n_common, replace=False))
    t = rng.permutation(n_new)[:n_common]                       # shuffled new-row order
    return q, t


# ---- 1. hand-placed ----------------------------------------------------------------------------------------------------------------

def test_hand_placed():
    """6 old rows, 5 new.  Old row 1 is unmatched, new row 3 is unmatched, old rows 2 and 3 both match new row 0 (a guarded term).
    List: (0, 2) (2, 0) (3, 0) (4, 4) (5, 1).  Terms: |o2 - o0| / |n0 - n2| = 8 / 4 = 2; guarded; |o4 - o3| / |n4 - n0| = 36 / 12 = 3;
    |o5 - o4| / |n1 - n4| = 20 / 5 = 4.  Scale (2 + 3 + 4) / 3 = 3."""
    new_X = np.array([[0, 0, 0], [5, 0, 12], [0, 4, 0], [9, 9, 9], [0, 0, 12]], dtype=np.float64)
    old_X = np.array([[0, 8, 0], [7, 7, 7], [0, 0, 0], [1, 0, 0], [1, 0, 36], [21, 0, 36]], dtype=np.float64)
    c = _case(6, 5, [0, 2, 3, 4, 5], [2, 0, 0, 4, 1], 1, old_X=old_X, new_X=new_X)
    ctx = mb._ctx()
    try:
        _install_old(ctx, c)
        got, keep = _align(ctx, c, use_rows=False, install=False)
        assert got["match"].tolist() == [2, -1, 0, 0, 4, 1]
        assert (got["n_old"], got["n_common"], got["n_terms"], got["status"]) == (6, 5, 3, 0)
        assert got["scale"] == 3.0
        assert np.array_equal(got["X"], new_X * 3.0)
        _check(got, c["want"], 6, "hand")
    finally:
        ctx.close()


# ---- 2. across the passes ----------------------------------------------------------------------------------------------------------

_BIG = []


def _big_case():
    """2 500 old rows, 2 300 new rows at a permutation's head of a 3 000-row block, 1 800 commons in shuffled new-row order: three
    compaction passes over the old rows, two chunks of the sum"""
    if not _BIG:
        q, t = _spread_commons(2500, 2300, 1800, 21)
        c = _case(2500, 2300, q, t, 22, block_rows=3000)
        cq = c["want"]["cq"]
        assert c["want"]["n_common"] == 1800 and c["want"]["status"] == mu.OK
        # consecutive list entries in DIFFERENT passes of 1 024 old rows, at both boundaries
        cross = (cq[:-1] // 1024) != (cq[1:] // 1024)
        assert cross.sum() == 2 and set((cq[1:][cross] // 1024).tolist()) == {1, 2}
        # the terms straddle the 1 024-term chunks of the sum: terms 1 023 and 1 024 both exist and are kept
        assert c["want"]["n_terms"] == 1799 > 1024
        assert abs(c["want"]["scale"] / 2.5 - 1) < 0.01
        _BIG.append(c)
    return _BIG[0]


@pytest.mark.parametrize("use_rows", [True, False])
def test_across_the_passes(use_rows):
    c = _big_case()
    ctx = mb._ctx(maxkp=4000)
    try:
        _install_old(ctx, c)
        got, keep = _align(ctx, c, use_rows=use_rows, install=True)
        _check(got, c["want"], 2500, ("passes", use_rows))
        _serves_like_host_map(ctx, c["new_desc"], c["want"]["X"], ("passes, installed", use_rows))
    finally:
        ctx.close()


# ---- 3. no scale -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["zero", "one", "guarded"])
def test_no_scale(kind):
    n_old, n_new = 300, 200
    if kind == "zero":
        q, t = [], []
    elif kind == "one":
        q, t = [150], [60]
    else:
        q, t = np.arange(n_old), np.full(n_old, 17)              # all old rows near-copies of ONE new row: every term guarded
    c = _case(n_old, n_new, q, t, 31)
    want = c["want"]
    assert want["n_common"] == len(q) and want["n_terms"] == 0 and want["status"] == mu.NO_SCALE and want["scale"] == 1.0
    ctx = mb._ctx()
    try:
        _install_old(ctx, c)
        got, keep = _align(ctx, c, use_rows=False, install=True)
        _check(got, want, n_old, kind)
        assert got["scale"] == 1.0 and got["status"] == 1
        assert np.array_equal(mb._bits(got["X"]), mb._bits(c["new_X"]))
        # the installed points are d_X's bits: the context serves like one given them through set_map_points
        _serves_like_host_map(ctx, c["new_desc"], c["new_X"], kind)
    finally:
        ctx.close()


# ---- 4. / 5. install ---------------------------------------------------------------------------------------------------------------

_MID = []


def _mid_case():
    if not _MID:
        q, t = _spread_commons(700, 650, 500, 41)
        _MID.append(_case(700, 650, q, t, 42, block_rows=900))
    return _MID[0]


def test_report_only_leaves_the_map():
    c = _mid_case()
    ctx = mb._ctx()
    try:
        _install_old(ctx, c)
        frame = _frame(c["old_desc"], c["old_X"], 43)
        before = _answer(ctx, frame)
        assert before[1]["Rt"] is not None and (before[0] >= 0).sum() > 400
        got, keep = _align(ctx, c, install=False)
        _check(got, c["want"], 700, "report only")
        mb._same_frame(_answer(ctx, frame), before, "after a report-only call")
        got, keep = _align(ctx, c, install=False)                # and again: the staging buffers hold nothing the next call needs
        _check(got, c["want"], 700, "report only, again")
        mb._same_frame(_answer(ctx, frame), before, "after two")
    finally:
        ctx.close()


def test_installed_map_serves():
    c = _mid_case()
    ctx = mb._ctx()
    try:
        _install_old(ctx, c)
        got, keep = _align(ctx, c, install=True)
        _check(got, c["want"], 700, "install")
        a = _serves_like_host_map(ctx, c["new_desc"], c["want"]["X"], "installed")
        assert (a[0] >= 0).sum() > 400 and a[1]["Rt"] is not None and len(a[1]["inliers"]) > 200
    finally:
        ctx.close()


# ---- 6. twice in a row -------------------------------------------------------------------------------------------------------------

def test_twice_in_a_row():
    """A by set_map; B aligned to A; C aligned to B AS RESCALED; D aligned to C: the buffers have changed places three times"""
    rng = np.random.default_rng(51)
    sizes = [600, 550, 640, 500]
    qt = [_spread_commons(sizes[k], sizes[k + 1], 400, 52 + k) for k in range(3)]
    ab = _case(sizes[0], sizes[1], qt[0][0], qt[0][1], 61, true_scale=2.0)
    ctx = mb._ctx()
    try:
        _install_old(ctx, ab)
        got, keep = _align(ctx, ab, use_rows=False, install=True)
        _check(got, ab["want"], sizes[0], "B to A")
        prev_desc, prev_X = ab["new_desc"], ab["want"]["X"]
        for k in (1, 2):
            # this step's old map is the previous step's new map: its rows as gathered, its points AS RESCALED; the next map's points
            # are those at 1 / (0.4 k) of that scale
            new_X = _points(rng, sizes[k + 1])
            new_X[qt[k][1]] = prev_X[qt[k][0]] / (0.4 * k) + rng.normal(0, 0.004, (400, 3))
            c = _case(sizes[k], sizes[k + 1], qt[k][0], qt[k][1], 62 + k, old_X=prev_X, new_X=new_X, old_desc=prev_desc)
            got, keep = _align(ctx, c, use_rows=False, install=True)
            _check(got, c["want"], sizes[k], ("step", k))
            assert abs(got["scale"] / (0.4 * k) - 1) < 0.01
            prev_desc, prev_X = c["new_desc"], c["want"]["X"]
        _serves_like_host_map(ctx, prev_desc, prev_X, "after three installs")
    finally:
        ctx.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------

def test_errors_keep_the_previous_map():
    from coloc_amd import CLCError, abi
    torch = mb._torch()
    c = _mid_case()
    ctx, fresh, rows_only = mb._ctx(maxkp=1000), mb._ctx(maxkp=1000), mb._ctx(maxkp=1000)
    try:
        _install_old(ctx, c)
        frame = _frame(c["old_desc"], c["old_X"], 43)
        before = _answer(ctx, frame)
        d_desc = torch.zeros((1001, 64), dtype=torch.uint8, device="cuda")
        d_X = torch.ones((1001, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        for kw, status in ((dict(n_new=1001), abi.CLC_ERR_CAPACITY),
                           (dict(n_new=100, d_desc=d_desc.data_ptr() + 8), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=-1), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, d_X=None), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, d_desc=None), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, d_X=d_X.data_ptr() + 4), abi.CLC_ERR_BAD_ARG),
                           (dict(n_new=100, d_rows=d_X.data_ptr() + 2), abi.CLC_ERR_BAD_ARG)):
            args = dict(dict(d_desc=d_desc.data_ptr(), d_X=d_X.data_ptr(), install=True), **kw)
            with pytest.raises(CLCError) as e:
                ctx.map_align_dev(**args)
            assert e.value.status == status, kw
            mb._same_frame(_answer(ctx, frame), before, ("after", kw))
        # no previous map; a map without points
        rows_only.set_map(c["old_desc"])
        for other in (fresh, rows_only):
            with pytest.raises(CLCError) as e:
                other.map_align_dev(d_desc.data_ptr(), d_X.data_ptr(), 100)
            assert e.value.status == abi.CLC_ERR_STATE
        # the context works afterwards
        got, keep = _align(ctx, c, install=True)
        _check(got, c["want"], 700, "after the refusals")
    finally:
        for x in (ctx, fresh, rows_only):
            x.close()


def test_an_empty_new_map():
    c = _mid_case()
    ctx = mb._ctx()
    try:
        torch = mb._torch()
        _install_old(ctx, c)
        frame = _frame(c["old_desc"], c["old_X"], 43)
        before = _answer(ctx, frame)
        got = ctx.map_align_dev(None, None, 0, install=False)
        assert (got["n_old"], got["n_common"], got["n_terms"], got["status"], got["scale"]) == (700, 0, 0, 1, 1.0) and (got["match"] == -1).all()
        mb._same_frame(_answer(ctx, frame), before, "empty, report only")
        got = ctx.map_align_dev(None, None, 0, install=True)
        assert (got["n_old"], got["status"], got["scale"]) == (700, 1, 1.0)
        d_match = torch.full((frame[1],), -5, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.match_map_dev(frame[0].data_ptr(), frame[1], 60, d_match.data_ptr(), None)          # the empty map: nothing matches
        ctx.sync()
        assert (d_match.cpu().numpy() == -1).all()
    finally:
        ctx.close()


# ---- 8. after_stream ---------------------------------------------------------------------------------------------------------------

def test_after_stream_orders_the_call_behind_the_producer():
    """the new map's block, row list and points are written on a foreign torch stream behind a stretch of other work, straight before
    the call, with no host synchronisation: only the event the call records on after_stream puts its launches behind them"""
    torch = mb._torch()
    c = _big_case()
    ctx = mb._ctx(maxkp=4000)
    try:
        _install_old(ctx, c)
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
            got = ctx.map_align_dev(dst[0].data_ptr(), dst[2].data_ptr(), c["n_new"], d_rows=dst[1].data_ptr(), install=True,
                                    after_stream=torch.cuda.current_stream().cuda_stream)
        _check(got, c["want"], 2500, "after_stream")
        torch.cuda.synchronize()
    finally:
        ctx.close()


# ---- 9. the composition ------------------------------------------------------------------------------------------------------------

def _composition_scene(counts, seed):
    n = 300
    sc = mb._scene(3, n, seed, dist=[track_host.DISTORTIONS[0], track_host.DISTORTIONS[1], track_host.DISTORTIONS[2]], noise=0.3)
    desc = mb._descriptors(n, sc["point_of"], seed + 1)
    rng = np.random.default_rng(seed + 2)
    pair_cams = [(0, 1), (0, 2), (1, 2)]
    matches = []
    for k, (a, b) in enumerate(pair_cams):
        m = np.full(n, -1, dtype=np.int32)
        q = rng.choice(n, counts[k], replace=False)
        m[q] = sc["row_of"][b][sc["point_of"][a][q]]
        wrong = q[rng.random(len(q)) < 0.15]
        m[wrong] = rng.integers(0, n, len(wrong))
        matches.append(m)
    d_match, d_feat, d_desc = [mb._dev(m) for m in matches], [mb._dev(c["feat"]) for c in sc["cams"]], [mb._dev(d) for d in desc]
    jobs = [dict(d_match=d_match[k].data_ptr(), nq=n, nt=n, cam_a=sc["cams"][a]["cam"], cam_b=sc["cams"][b]["cam"], d_feat_a=d_feat[a].data_ptr(),
                 feat_stride_a=4, d_feat_b=d_feat[b].data_ptr(), feat_stride_b=4, img_wh=(mb.W, mb.H), seed=5 + k) for k, (a, b) in enumerate(pair_cams)]
    dc = [dict(cam=c["cam"], d_feat=d_feat[i].data_ptr(), feat_stride=4, d_desc=d_desc[i].data_ptr()) for i, c in enumerate(sc["cams"])]
    # the previous map: 200 rows, 150 of them near-copies of camera 0's rows (the lower camera of both pairs that can be the seed),
    # their points the world's at 2.5 x
    prev_rows = rng.choice(n, 150, replace=False)
    prev_desc = rng.integers(0, 256, (200, 64), dtype=np.uint8)
    where = np.sort(rng.choice(200, 150, replace=False))
    prev_desc[where] = _flip(desc[0][prev_rows], rng, 4)
    prev_X = _points(rng, 200) * 2.5
    prev_X[where] = sc["X"][sc["point_of"][0][prev_rows]] * 2.5
    return dict(n=n, sc=sc, desc=desc, pair_cams=pair_cams, jobs=jobs, dc=dc, prev_desc=prev_desc, prev_X=prev_X, keep=(d_match, d_feat, d_desc),
                d_desc=d_desc)


def test_update_equals_init_then_align():
    from coloc_amd import abi
    torch = mb._torch()
    s = _composition_scene((250, 220, 10), 81)
    n, sc = s["n"], s["sc"]
    set1, twins = [mb._ctx() for _ in range(3)], [mb._ctx() for _ in range(3)]
    try:
        origin_R, origin_C, scale = np.eye(3), np.array([0.3, -0.2, 0.1]), 3.0
        set1[0].set_map(s["prev_desc"])
        set1[0].set_map_points(s["prev_X"])
        # the twin set: init alone, then the align step on set 1 fed from the twin's map, report only
        tw, tw_filt = abi.map_init_batch_dev(twins, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], origin_R=origin_R, origin_C=origin_C, scale=scale)
        assert tw["seed_pair"] == 0 and tw["map_n"] > 100
        lower = s["pair_cams"][tw["seed_pair"]][0]
        d_rows, d_X = mb._dev(tw["map_row"]), mb._dev(tw["X"])
        al = set1[0].map_align_dev(s["d_desc"][lower].data_ptr(), d_X.data_ptr(), tw["map_n"], d_rows=d_rows.data_ptr(), install=False)
        # ... which is itself the host statement's, on the oracle's matches
        new_desc = s["desc"][lower][tw["map_row"]]
        want = mu.align(s["prev_X"], tw["X"], _oracle().k2nn(s["prev_desc"], new_desc, 60))
        _check(al, want, 200, "align on the twin's map")
        assert want["status"] == mu.OK and want["n_common"] > 50 and 0.5 < want["scale"] < 1.5       # 2.5 x the world against a baseline of 3
        got, filt = abi.map_update_batch_dev(set1, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], origin_R=origin_R, origin_C=origin_C, scale=scale)
        for k in range(3):
            assert filt[k]["n_pairs"] == tw_filt[k]["n_pairs"] and np.array_equal(filt[k]["inliers"], tw_filt[k]["inliers"])
        assert got["seed_pair"] == tw["seed_pair"] and got["entered"] == tw["entered"] == [True, True, False]
        assert got["n_tracks"] == tw["n_tracks"] and np.array_equal(got["track_feat"], tw["track_feat"])
        assert got["map_n"] == tw["map_n"] and np.array_equal(got["map_track"], tw["map_track"]) and np.array_equal(got["map_row"], tw["map_row"])
        ga = got["align"]
        assert np.array_equal(ga["match"], al["match"]) and (ga["n_old"], ga["n_common"], ga["n_terms"], ga["status"]) == (al["n_old"], al["n_common"], al["n_terms"], al["status"])
        assert np.array_equal(mb._bits(np.float64(ga["scale"])), mb._bits(np.float64(al["scale"])))
        assert np.array_equal(mb._bits(got["X"]), mb._bits(al["X"]))
        for key in ("Rt_seed_a", "Rt_seed_b"):
            assert np.array_equal(mb._bits(got[key]), mb._bits(mu.rescale_pose(tw[key], al["scale"]))), key
        a = _serves_like_host_map(set1[0], new_desc, want["X"], "update's map")
        assert (a[0] >= 0).sum() > 80
        torch.cuda.synchronize()
    finally:
        for c in set1 + twins:
            c.close()


def test_update_without_an_entering_pair_or_a_previous_map():
    from coloc_amd import CLCError, abi
    s = _composition_scene((10, 9, 8), 91)
    n = s["n"]
    set1 = [mb._ctx() for _ in range(3)]
    try:
        with pytest.raises(CLCError) as e:                                            # no previous map on ctxs[0]
            abi.map_update_batch_dev(set1, s["jobs"], [n] * 3, s["pair_cams"], s["dc"])
        assert e.value.status == abi.CLC_ERR_STATE
        set1[0].set_map(s["prev_desc"])
        set1[0].set_map_points(s["prev_X"])
        frame = _frame(s["prev_desc"], s["prev_X"], 92, n=200)
        before = _answer(set1[0], frame)
        got, filt = abi.map_update_batch_dev(set1, s["jobs"], [n] * 3, s["pair_cams"], s["dc"])
        assert got["seed_pair"] == -1 and got["map_n"] == -1 and got["entered"] == [False] * 3 and got["status"] == 0
        assert (got["align"]["status"], got["align"]["scale"], got["align"]["n_common"]) == (1, 1.0, 0)
        mb._same_frame(_answer(set1[0], frame), before, "no pair entered")
    finally:
        for c in set1:
            c.close()

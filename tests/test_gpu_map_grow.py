"""The map grown past the seed pair on the device (include/coloc_hip.h: clc_map_build_grow_dev, clc_map_init_grow_batch_dev,
clc_map_update_grow_batch_dev, clc_map_resect_build_dev).

Comparison rule: every discrete outcome (resection lists, masks, cameras, rows, counts, statuses) is compared EXACTLY with
tests/map_grow_host.py, the Python statement of the rules, fed the device's own resection poses; landmarks are compared BIT FOR BIT with
the g++ build of coloc_amd/csrc/map_math.h; a resection is compared bit for bit with clc_pnp_acransac on the host copy of its
correspondences.  The scene helpers are those of tests/test_gpu_map_build.py's kind, re-stated here."""
import itertools

import numpy as np
import pytest

import inter_geometry_host
import map_grow_host
import map_host
import map_update_host as mu
import track_host

pytestmark = pytest.mark.gpu

W, H = 1280, 720
F0 = (1000.0, 640.0, 360.0)
OK, NO_TRACKS, NO_POSE = map_grow_host.GROW_OK, map_grow_host.GROW_NO_TRACKS, map_grow_host.GROW_NO_POSE


def _torch():
    import torch
    return torch


def _dev(a):
    """a numpy array on the GPU, complete before anything another stream enqueues"""
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


def _dev_pairs(pairs, keep):
    out = []
    for p in pairs:
        q, t = np.asarray(p["q"], dtype=np.int32), np.asarray(p["t"], dtype=np.int32)
        d = dict(cam_a=p["cam_a"], cam_b=p["cam_b"], n=len(q))
        if len(q):
            tq, tt = _dev(q), _dev(t)
            keep += [tq, tt]
            d.update(d_q=tq.data_ptr(), d_t=tt.data_ptr())
        out.append(d)
    return out


def _dev_cams(cams, keep, desc):
    out = []
    for c, spec in enumerate(cams):
        t, td = _dev(np.asarray(spec["feat"], dtype=np.float32)), _dev(desc[c])
        keep += [t, td]
        out.append(dict(cam=spec["cam"], d_feat=t.data_ptr(), feat_stride=np.asarray(spec["feat"]).shape[1], d_desc=td.data_ptr()))
    return out


def _descriptors(n_points, rows_of, seed, flips=40):
    """one random 512-bit descriptor per world point; camera c's row r carries the descriptor of point rows_of[c][r] with up to `flips` bits
    flipped -- far enough apart that a row taken from the wrong camera's block is told from the right one (_rows_are)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_points, 64), dtype=np.uint8)
    out = []
    for pts in rows_of:
        d = base[pts].copy()
        for k in range(flips):
            d[np.arange(len(pts)), rng.integers(0, 64, len(pts))] ^= (1 << rng.integers(0, 8, len(pts))).astype(np.uint8)
        out.append(d)
    return out


def _distort(x, cam):
    f, pp, k = cam[0], np.array(cam[1:3]), cam[3:6]
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


def _small_rot(rng):
    a, b = rng.uniform(-0.06, 0.06), rng.uniform(-0.03, 0.03)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return Ry @ Rx


def _scene(n_cams, n_rows, seed, noise=0.2):
    """a world of n_rows points seen by n_cams cameras side by side (camera c's row r shows point point_of[c][r], a permutation): float
    feature blocks of the DISTORTED pixels, the cameras, their [R|t]"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-5, 5, n_rows), rng.uniform(-3, 3, n_rows), rng.uniform(8, 20, n_rows)], 1)
    cams, Rts, point_of = [], [], []
    for c in range(n_cams):
        cam = F0 + track_host.DISTORTIONS[c % 3]
        R = np.eye(3) if c == 0 else _small_rot(rng)
        Cc = np.array([0.8 * c, rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)]) if c else np.zeros(3)
        Rt = np.hstack([R, (-R @ Cc)[:, None]])
        perm = rng.permutation(n_rows)
        u = (X[perm] @ R.T + Rt[:, 3]) @ np.array([[cam[0], 0, cam[1]], [0, cam[0], cam[2]], [0, 0, 1.0]]).T
        px = u[:, :2] / u[:, 2:3] + rng.normal(0, noise, (n_rows, 2))
        feat = np.zeros((n_rows, 4), dtype=np.float32)
        feat[:, :2] = _distort(px, cam)
        feat[:, 2] = 7.0
        cams.append(dict(cam=cam, feat=feat))
        Rts.append(Rt)
        point_of.append(perm)
    return dict(X=X, cams=cams, Rt=Rts, point_of=point_of, row_of=[np.argsort(p) for p in point_of])


def _scene_pairs(sc, n_matches, seed, wrong=0.1, garbage=(), lone=()):
    """every camera pair a < b: n_matches random rows of a matched to the row of b that shows the same point, `wrong` of them to a random
    row instead.  A camera in `garbage` keeps ONE pair, with camera 0, whose every match is wrong (a derangement of the truth); a camera
    in `lone` has no match at all."""
    rng = np.random.default_rng(seed)
    n_cams, n_rows = len(sc["cams"]), len(sc["X"])
    pairs = []
    for a, b in itertools.combinations(range(n_cams), 2):
        q = rng.choice(n_rows, n_matches, replace=False)
        t = sc["row_of"][b][sc["point_of"][a][q]]
        bad = rng.random(n_matches) < wrong
        t = np.where(bad, rng.integers(0, n_rows, n_matches), t)
        if a in lone or b in lone or ((a in garbage or b in garbage) and a != 0):
            q, t = q[:0], t[:0]
        elif b in garbage:
            t = np.roll(t, 1)                                    # (every query gets another query's answer: one-to-one, all wrong)
        pairs.append(dict(cam_a=a, cam_b=b, q=q.astype(np.int32), t=t.astype(np.int32)))
    return pairs


def _reprojection_ok(sc, lst, I, px=3.0):
    """how many entries of a resection list agree with camera I's true pose (the correspondences a solve can stand on)"""
    if len(lst["track"]) == 0:
        return 0
    Rt, cam = sc["Rt"][I], sc["cams"][I]["cam"]
    u = lst["X"] @ Rt[:, :3].T + Rt[:, 3]
    p = u[:, :2] / u[:, 2:3] * cam[0] + np.array(cam[1:3])
    return int((np.linalg.norm(p - lst["x"], axis=1) < px).sum())


def _statement(rows, pairs, sc, seed_pair, got):
    """the Python statement fed the device's own poses"""
    g = got["grow"]
    a, b = pairs[seed_pair]["cam_a"], pairs[seed_pair]["cam_b"]
    return map_grow_host.grow_map(rows, pairs, sc["cams"], seed_pair, sc["Rt"][a], sc["Rt"][b], lambda I, lst: g["Rt"][I] if g["resected"][I] else None)


def _check_grown(got, want, what):
    g = got["grow"]
    assert got["n_tracks"] == len(want["track_feat"]) and np.array_equal(got["track_feat"], want["track_feat"]), what
    assert g["n_seed_rows"] == want["n_seed_rows"], (what, g["n_seed_rows"], want["n_seed_rows"])
    assert g["status"] == want["status"], (what, g["status"], want["status"])
    assert [int(n) for n in g["n_corr"]] == [len(want["lists"][c]["track"]) if c in want["lists"] else 0 for c in range(len(g["n_corr"]))], what
    assert got["map_n"] == len(want["map_track"]) and g["n_added"] == want["n_added"], (what, got["map_n"], len(want["map_track"]))
    for key in ("map_track", "map_row"):
        assert np.array_equal(got[key], want[key]), (what, key)
    assert np.array_equal(g["map_cam"], want["map_cam"]) and np.array_equal(g["map_obs"], want["map_obs"]), what
    assert np.array_equal(_bits(got["X"]), _bits(want["map_X"])), (what, int((_bits(got["X"]) != _bits(want["map_X"])).sum()))


def _build(ctx, sc, pairs, rows, seed_pair, desc, keep, seed=7, **kw):
    a, b = pairs[seed_pair]["cam_a"], pairs[seed_pair]["cam_b"]
    return ctx.map_build_grow_dev(rows, _dev_pairs(pairs, keep), _dev_cams(sc["cams"], keep, desc), seed_pair, sc["Rt"][a], sc["Rt"][b], seed=seed, **kw)


def _resect_on_device(ctx, rows, cams_dev, camera):
    torch = _torch()
    n = rows[camera]
    d_X, d_x = torch.full((3 * n,), -1.0, dtype=torch.float64, device="cuda"), torch.full((2 * n,), -1.0, dtype=torch.float64, device="cuda")
    d_t, d_r = torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_n = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.map_resect_build_dev(rows, cams_dev, camera, d_X.data_ptr(), d_x.data_ptr(), d_t.data_ptr(), d_r.data_ptr(), d_n.data_ptr(), None)
    ctx.sync()
    k = int(d_n.cpu()[0])
    assert 0 <= k <= n
    return dict(track=d_t.cpu().numpy()[:k], row=d_r.cpu().numpy()[:k], X=d_X.cpu().numpy().reshape(-1, 3)[:k], x=d_x.cpu().numpy().reshape(-1, 2)[:k])


def _same_list(got, want, what):
    assert np.array_equal(got["track"], want["track"]) and np.array_equal(got["row"], want["row"]), what
    assert np.array_equal(_bits(got["X"]), _bits(want["X"])) and np.array_equal(_bits(got["x"]), _bits(want["x"])), what


# ---- 1. the resect gather ----------------------------------------------------------------------------------------------------------

def test_resect_gather_on_a_hand_placed_table_and_a_scene():
    from coloc_amd import CLCError, abi
    from test_map_grow_host import hand_case
    ctx = _ctx()
    try:
        # the hand-placed tracks: every resection list has one to three entries, too few for a pose, so the state stays the seed's
        rows, pairs, cams, seed_pair, poses, row_of = hand_case()
        desc = [np.random.default_rng(3 + c).integers(0, 256, (r, 64), dtype=np.uint8) for c, r in enumerate(rows)]
        keep = []
        dc = _dev_cams(cams, keep, desc)
        got = ctx.map_build_grow_dev(rows, _dev_pairs(pairs, keep), dc, seed_pair, poses[1], poses[4])
        want = map_grow_host.grow_map(rows, pairs, cams, seed_pair, poses[1], poses[4], lambda I, lst: None)
        assert got["grow"]["status"] == [NO_POSE, OK, NO_POSE, NO_POSE, OK, NO_POSE, NO_POSE] == want["status"]
        _check_grown(got, want, "hand")
        for c in range(7):
            lst = map_grow_host.resect_list(want["track_feat"], want["state_X"], want["state_obs"], want["ud"], c)
            assert 1 <= len(lst["track"]) <= 3
            _same_list(_resect_on_device(ctx, rows, dc, c), lst, ("hand", c))
        for camera in (-1, 7):
            with pytest.raises(CLCError) as e:
                ctx.map_resect_build_dev(rows, dc, camera, 0, 0, 0, 0, 0, None)
            assert e.value.status == abi.CLC_ERR_BAD_ARG
        # a scene: the state after its last camera
        sc = _scene(4, 300, 11)
        pairs = _scene_pairs(sc, 170, 12, wrong=0.03)
        rows = [300] * 4
        desc = _descriptors(300, sc["point_of"], 13)
        dc = _dev_cams(sc["cams"], keep, desc)
        got = ctx.map_build_grow_dev(rows, _dev_pairs(pairs, keep), dc, 0, sc["Rt"][0], sc["Rt"][1], seed=7)
        want = _statement(rows, pairs, sc, 0, got)
        assert got["grow"]["resected"] == [False, False, True, True]
        for c in range(4):
            lst = map_grow_host.resect_list(want["track_feat"], want["state_X"], want["state_obs"], want["ud"], c)
            assert len(lst["track"]) > 100
            _same_list(_resect_on_device(ctx, rows, dc, c), lst, ("scene", c))
        # a plain build rewrites the block the table lies in: the state is gone
        ctx.map_build_dev(rows, _dev_pairs(pairs, keep), dc, 0, sc["Rt"][0], sc["Rt"][1])
        with pytest.raises(CLCError) as e:
            _resect_on_device(ctx, rows, dc, 2)
        assert e.value.status == abi.CLC_ERR_STATE
    finally:
        ctx.close()


# ---- 2., 3. the resections and the grown map ---------------------------------------------------------------------------------------

CASES = {
    # name: (cameras, rows, matches per pair, wrong, seed pair as cameras, garbage cameras, lone cameras, scene seed [, precision])
    # The garbage camera's case bounds the solve's threshold at 10 pixels (precision = its square): with the a-contrario threshold left
    # free the solve finds, in 81 correspondences that are ALL wrong, a "pose" that holds 68 of them at 348 pixels, a quarter of the image
    # -- clc_pnp_acransac's answer on the host copy as well.  The true cameras' solves end at 2 - 3 pixels.
    "4x300": (4, 300, 150, 0.0, (0, 1), (), (), 21),
    "4x300, seed (1, 2): camera 0 takes descriptors over": (4, 300, 170, 0.03, (1, 2), (), (), 22),
    "5x400, 10 % wrong": (5, 400, 200, 0.1, (0, 1), (), (), 23),
    "6x400: camera 2 all wrong, camera 4 without a track": (6, 400, 220, 0.1, (0, 1), (2,), (4,), 24, 100.0),
    "8x1500: more than one pass": (8, 1500, 600, 0.005, (1, 4), (), (), 25),
}


@pytest.mark.parametrize("name", list(CASES))
def test_grown_map_equals_the_statement_and_resections_equal_the_solve(name):
    n_cams, n, n_matches, wrong, seed_cams, garbage, lone, s = CASES[name][:8]
    precision = CASES[name][8] if len(CASES[name]) > 8 else float("inf")
    ctx, solver = _ctx(maxkp=6000), _ctx()
    try:
        sc = _scene(n_cams, n, s)
        pairs = _scene_pairs(sc, n_matches, s + 100, wrong=wrong, garbage=garbage, lone=lone)
        rows = [n] * n_cams
        seed_pair = [(p["cam_a"], p["cam_b"]) for p in pairs].index(seed_cams)
        desc = _descriptors(n, sc["point_of"], s + 200, flips=6)
        # the statement alone, on the true poses: every intended camera has correspondences a solve can stand on
        truth = map_grow_host.grow_map(rows, pairs, sc["cams"], seed_pair, sc["Rt"][seed_cams[0]], sc["Rt"][seed_cams[1]],
                                       lambda I, lst: None if I in garbage else sc["Rt"][I])
        intended = [c for c in range(n_cams) if c not in seed_cams + garbage + lone]
        for c in intended:
            assert _reprojection_ok(sc, truth["lists"][c], c) > 60, (name, c)
        for c in garbage:
            assert len(truth["lists"][c]["track"]) > 60 and _reprojection_ok(sc, truth["lists"][c], c) < 6, (name, c)
        keep = []
        got = _build(ctx, sc, pairs, rows, seed_pair, desc, keep, seed=7, precision=precision)
        g = got["grow"]
        assert g["status"] == [NO_POSE if c in garbage else (NO_TRACKS if c in lone else OK) for c in range(n_cams)], (name, g["status"])
        assert g["resected"] == [c in intended for c in range(n_cams)]
        want = _statement(rows, pairs, sc, seed_pair, got)
        _check_grown(got, want, name)
        assert want["n_added"] > 20 and len(want["map_track"]) > want["n_seed_rows"]
        new = ~np.isin(want["map_track"], want["seed_tracks"][want["seed_ok"]])
        assert new.any() and new[:-1][~new[1:]].any()                 # new landmarks interleave with the seed's
        if seed_cams[0] > 0:
            assert (want["map_cam"] == 0).sum() > 50 and (want["map_cam"] == seed_cams[0]).any()
        if len(want["track_feat"]) > 1024:
            assert (want["map_track"] < 1024).any() and (want["map_track"] >= 1024).any() and len(want["map_track"]) > 1024
        # the seed cameras report their seed poses; a camera that failed reports zeros
        for c, Rt in zip(seed_cams, (sc["Rt"][seed_cams[0]], sc["Rt"][seed_cams[1]])):
            assert np.array_equal(_bits(g["Rt"][c]), _bits(np.ascontiguousarray(Rt)))
        for c in garbage + lone:
            assert not g["Rt"][c].any() and g["n_inliers"][c] <= 7
        # 2. every resection is clc_pnp_acransac's on the host copy of the same correspondences, seed + k
        for k, c in enumerate(want["order"]):
            lst = want["lists"][c]
            if len(lst["track"]) == 0:
                continue
            cam = sc["cams"][c]["cam"]
            ref = solver.pnp_acransac(lst["X"], lst["x"], np.array([[cam[0], 0, cam[1]], [0, cam[0], cam[2]], [0, 0, 1.0]]), max_iteration=256, seed=7 + k,
                                      precision=precision)
            assert g["n_inliers"][c] == len(ref["inliers"]), (name, c)
            assert np.array_equal(_bits(np.float64(g["error_max"][c])), _bits(np.float64(ref["error_max"]))), (name, c)
            if ref["Rt"] is None:
                assert not g["Rt"][c].any()
            else:
                assert np.array_equal(_bits(g["Rt"][c]), _bits(ref["Rt"])), (name, c)
            if c in intended:
                assert len(ref["inliers"]) > 40 and np.abs(ref["Rt"] - sc["Rt"][c]).max() < 0.1
        # the same build again: nothing depends on scheduling
        again = _build(ctx, sc, pairs, rows, seed_pair, desc, keep, seed=7, precision=precision)
        _check_grown(again, want, name + ", again")
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(again["grow"]["Rt"], g["Rt"]))
    finally:
        ctx.close()
        solver.close()


# ---- 4. the installed map ----------------------------------------------------------------------------------------------------------

def _frame_against_map(ctx, d_q, nq, d_feat, cam, seed=3, threshold=60):
    torch = _torch()
    d_match = torch.full((nq,), -5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.match_map_dev(d_q.data_ptr(), nq, threshold, d_match.data_ptr(), None)
    r = ctx.track_localize_dev(d_match=d_match.data_ptr(), nq=nq, cam=cam, d_feat=d_feat.data_ptr(), feat_stride=4, seed=seed)
    ctx.sync()
    return d_match.cpu().numpy(), r


def _same_frame(a, b, what):
    (ma, ra), (mb, rb) = a, b
    assert np.array_equal(ma, mb), what
    assert ra["n_tracks"] == rb["n_tracks"] and np.array_equal(ra["track_query"], rb["track_query"]) and np.array_equal(ra["track_map"], rb["track_map"]), what
    assert np.array_equal(ra["inliers"], rb["inliers"]) and (ra["Rt"] is None) == (rb["Rt"] is None), what
    if ra["Rt"] is not None:
        assert np.array_equal(_bits(ra["Rt"]), _bits(rb["Rt"])) and np.array_equal(_bits(ra["cov"]), _bits(rb["cov"])), what


def _probe(ctx, rows):
    torch = _torch()
    d_q = _dev(rows)
    d_match = torch.full((len(rows),), -5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.match_map_dev(d_q.data_ptr(), len(rows), 180, d_match.data_ptr(), None)
    ctx.sync()
    return d_match.cpu().numpy()


def _rows_are(ctx, rows, what):
    """The context's map rows are `rows`: the library hands out no pointer to its map, so the rows are read through the matcher.  Row i
    of `rows` is matched under a threshold of 180: with the right row in place its distance is 0 and the gap to any other row (random
    512-bit rows: > 200 bits) passes; a row from ANOTHER camera's block (some 75 bits away, _descriptors' flips) or of another point
    does not.  (Two tracks of one world point leave two near rows and no match in either map: hence the comparison with a context
    that holds `rows` through clc_set_map, and `most` for the identity: with 55 - 75 % of the rows matched per pair up to a tenth of the
    world points end up in two tracks.)"""
    ref = _ctx(maxkp=max(len(rows), 64))
    try:
        ref.set_map(rows)
        want = _probe(ref, rows)
    finally:
        ref.close()
    got = _probe(ctx, rows)
    assert np.array_equal(got, want), (what, int((got != want).sum()))
    assert (want == np.arange(len(rows))).mean() > 0.8 and ((want == np.arange(len(rows))) | (want == -1)).all(), what


def test_installed_map_has_the_rows_and_serves_like_the_host_assembled_copy():
    ctx, ref = _ctx(), _ctx()
    try:
        sc = _scene(4, 600, 31)
        pairs = _scene_pairs(sc, 330, 32, wrong=0.03)
        rows = [600] * 4
        seed_pair = [(p["cam_a"], p["cam_b"]) for p in pairs].index((1, 2))
        desc = _descriptors(600, sc["point_of"], 33)
        keep = []
        got = _build(ctx, sc, pairs, rows, seed_pair, desc, keep)
        g = got["grow"]
        assert g["resected"] == [True, False, False, True] and len(set(g["map_cam"].tolist())) >= 3
        host_rows = np.stack([desc[c][r] for c, r in zip(g["map_cam"], got["map_row"])])
        _rows_are(ctx, host_rows, "grown map")
        # (the probe tells a row of the wrong camera: the seed's lower camera's rows in place of camera 0's fail it)
        moved = g["map_cam"] == 0
        wrong_rows = host_rows.copy()
        table = got["track_feat"]
        wrong_rows[moved] = desc[1][table[got["map_track"][moved], 1]]
        assert moved.sum() > 100
        ref.set_map(wrong_rows)
        assert (_probe(ref, host_rows)[moved] == -1).all()
        ref.set_map(host_rows)
        ref.set_map_points(got["X"])
        # camera 0's frame against both, and camera 3's: it localises where the grow resected it
        d_q, d_f = _dev(desc[0]), _dev(sc["cams"][0]["feat"])
        _same_frame(_frame_against_map(ctx, d_q, 600, d_f, sc["cams"][0]["cam"]), _frame_against_map(ref, d_q, 600, d_f, sc["cams"][0]["cam"]), "grown map, camera 0")
        d_q, d_f = _dev(desc[3]), _dev(sc["cams"][3]["feat"])
        a = _frame_against_map(ctx, d_q, 600, d_f, sc["cams"][3]["cam"])
        b = _frame_against_map(ref, d_q, 600, d_f, sc["cams"][3]["cam"])
        _same_frame(a, b, "grown map, camera 3")
        assert (a[0] >= 0).sum() > 200 and a[1]["Rt"] is not None and np.abs(a[1]["Rt"] - sc["Rt"][3]).max() < 0.1
    finally:
        ctx.close()
        ref.close()


# ---- 5. the unchanged paths and the compositions -----------------------------------------------------------------------------------

def test_two_cameras_leave_nothing_to_resect():
    ctx, plain = _ctx(), _ctx()
    try:
        sc = _scene(2, 700, 41)
        pairs = _scene_pairs(sc, 500, 42)
        desc = _descriptors(700, sc["point_of"], 43)
        keep = []
        dp, dc = _dev_pairs(pairs, keep), _dev_cams(sc["cams"], keep, desc)
        a = plain.map_build_dev([700, 700], dp, dc, 0, sc["Rt"][0], sc["Rt"][1])
        b = ctx.map_build_grow_dev([700, 700], dp, dc, 0, sc["Rt"][0], sc["Rt"][1])
        assert a["map_n"] == b["map_n"] > 300 and a["n_tracks"] == b["n_tracks"]
        for key in ("track_feat", "map_track", "map_row"):
            assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(_bits(a["X"]), _bits(b["X"]))
        g = b["grow"]
        assert g["status"] == [OK, OK] and g["resected"] == [False, False] and g["n_added"] == 0 and g["n_seed_rows"] == a["map_n"]
        assert (g["map_cam"] == 0).all() and (g["map_obs"] == 3).all()
        d_q, d_f = _dev(desc[1]), _dev(sc["cams"][1]["feat"])
        _same_frame(_frame_against_map(ctx, d_q, 700, d_f, sc["cams"][1]["cam"]), _frame_against_map(plain, d_q, 700, d_f, sc["cams"][1]["cam"]), "two cameras")
    finally:
        ctx.close()
        plain.close()


def _composition_scene(counts, seed, n=400):
    sc = _scene(3, n, seed, noise=0.3)
    desc = _descriptors(n, sc["point_of"], seed + 1, flips=6)
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
    d_match, d_feat, d_desc = [_dev(m) for m in matches], [_dev(c["feat"]) for c in sc["cams"]], [_dev(d) for d in desc]
    jobs = [dict(d_match=d_match[k].data_ptr(), nq=n, nt=n, cam_a=sc["cams"][a]["cam"], cam_b=sc["cams"][b]["cam"], d_feat_a=d_feat[a].data_ptr(),
                 feat_stride_a=4, d_feat_b=d_feat[b].data_ptr(), feat_stride_b=4, img_wh=(W, H), seed=5 + k) for k, (a, b) in enumerate(pair_cams)]
    dc = [dict(cam=c["cam"], d_feat=d_feat[i].data_ptr(), feat_stride=4, d_desc=d_desc[i].data_ptr()) for i, c in enumerate(sc["cams"])]
    return dict(n=n, sc=sc, desc=desc, pair_cams=pair_cams, jobs=jobs, dc=dc, keep=(d_match, d_feat, d_desc), rng=rng)


def _same_grown(a, b, what):
    assert a["map_n"] == b["map_n"] and a["n_tracks"] == b["n_tracks"], what
    for key in ("track_feat", "map_track", "map_row"):
        assert np.array_equal(a[key], b[key]), (what, key)
    assert np.array_equal(_bits(a["X"]), _bits(b["X"])), what
    ga, gb = a["grow"], b["grow"]
    for key in ("resected", "status", "n_corr", "n_inliers", "n_seed_rows", "n_added"):
        assert ga[key] == gb[key], (what, key)
    assert np.array_equal(ga["map_cam"], gb["map_cam"]) and np.array_equal(ga["map_obs"], gb["map_obs"]), what
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(ga["Rt"], gb["Rt"])), what


def test_init_grow_equals_filter_selection_and_build_grow():
    from coloc_amd import abi
    s = _composition_scene((300, 260, 10), 51)
    n, sc = s["n"], s["sc"]
    ctxs, refs, other, plain = [_ctx() for _ in range(3)], [_ctx() for _ in range(3)], _ctx(), [_ctx() for _ in range(3)]
    try:
        origin_R, origin_C, scale = np.eye(3), np.array([0.3, -0.2, 0.1]), 0.8
        got, filt = abi.map_init_grow_batch_dev(ctxs, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], origin_R=origin_R, origin_C=origin_C, scale=scale, seed=11)
        # the same by hand
        ref_filt = abi.pair_filter_batch_dev(refs, "E", s["jobs"])
        K = np.array([[F0[0], 0, F0[1]], [0, F0[0], F0[2]], [0, 0, 1.0]])
        entered, votes = [], []
        for k, r in enumerate(ref_filt):
            assert r["n_pairs"] == filt[k]["n_pairs"] and np.array_equal(r["inliers"], filt[k]["inliers"])
            v = None
            if len(r["inliers"]) >= 13:
                v = inter_geometry_host.relative(np.ascontiguousarray(r["x1"]), np.ascontiguousarray(r["x2"]), K, np.ascontiguousarray(r["M"]),
                                                 np.ascontiguousarray(r["inliers"], dtype=np.int32))
                v = v if v["stage"] == 0 else None
            entered.append(v is not None)
            votes.append(v)
        assert entered == [True, True, False] and got["entered"] == entered and got["seed_pair"] == 0
        Rt_a, Rt_b = abi.seed_poses(origin_R, origin_C, votes[0]["R"], map_host.pose_center(votes[0]["R"], votes[0]["t"]), scale)
        assert np.array_equal(_bits(got["Rt_seed_a"]), _bits(Rt_a)) and np.array_equal(_bits(got["Rt_seed_b"]), _bits(Rt_b))
        host_pairs = [dict(cam_a=a, cam_b=b, q=r["pair_q"][r["inliers"]], t=r["pair_t"][r["inliers"]]) for (a, b), r, e in zip(s["pair_cams"], ref_filt, entered) if e]
        keep = []
        built = other.map_build_grow_dev([n] * 3, _dev_pairs(host_pairs, keep), s["dc"], 0, Rt_a, Rt_b, seed=11)
        _same_grown(got, built, "filter + selection + build_grow")
        want = map_grow_host.grow_map([n] * 3, host_pairs, sc["cams"], 0, Rt_a, Rt_b, lambda I, lst: got["grow"]["Rt"][I] if got["grow"]["resected"][I] else None)
        _check_grown(got, want, "init_grow")
        assert got["grow"]["resected"] == [False, False, True] and got["grow"]["n_added"] > 10
        # the plain composition is what it was: the seed pair's map
        base, _ = abi.map_init_batch_dev(plain, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], origin_R=origin_R, origin_C=origin_C, scale=scale)
        seed_map = map_host.build_map([n] * 3, host_pairs, sc["cams"], 0, Rt_a, Rt_b)
        assert base["map_n"] == len(seed_map["map_track"]) == got["grow"]["n_seed_rows"] and np.array_equal(base["map_track"], seed_map["map_track"])
        assert np.array_equal(_bits(base["X"]), _bits(seed_map["X"]))
        _torch().cuda.synchronize()
    finally:
        for c in ctxs + refs + plain + [other]:
            c.close()


def test_update_grow_installs_the_grown_map_at_the_old_scale():
    import oracle_lib
    from coloc_amd import CLCError, abi
    s = _composition_scene((300, 260, 10), 61)
    n, sc, rng = s["n"], s["sc"], s["rng"]
    set1, twins = [_ctx() for _ in range(3)], [_ctx() for _ in range(3)]
    small = []
    try:
        origin_R, origin_C, scale = np.eye(3), np.array([0.3, -0.2, 0.1]), 3.0
        # the previous map: 200 rows, 150 of them near-copies of camera 0's rows, their points the world's at 2.5 x
        prev_rows = rng.choice(n, 150, replace=False)
        prev_desc = rng.integers(0, 256, (200, 64), dtype=np.uint8)
        where = np.sort(rng.choice(200, 150, replace=False))
        prev_desc[where] = s["desc"][0][prev_rows]
        prev_X = np.stack([rng.uniform(-5, 5, 200), rng.uniform(-3, 3, 200), rng.uniform(8, 20, 200)], 1) * 2.5
        prev_X[where] = sc["X"][sc["point_of"][0][prev_rows]] * 2.5
        set1[0].set_map(prev_desc)
        set1[0].set_map_points(prev_X)
        tw, _ = abi.map_init_grow_batch_dev(twins, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], origin_R=origin_R, origin_C=origin_C, scale=scale, seed=11)
        tg = tw["grow"]
        assert tw["seed_pair"] == 0 and tg["resected"] == [False, False, True] and tg["n_added"] > 10
        new_desc = np.stack([s["desc"][c][r] for c, r in zip(tg["map_cam"], tw["map_row"])])
        want = mu.align(prev_X, tw["X"], oracle_lib.Oracle().k2nn(prev_desc, new_desc, 60))
        assert want["status"] == mu.OK and want["n_common"] > 50
        got, _ = abi.map_update_grow_batch_dev(set1, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], origin_R=origin_R, origin_C=origin_C, scale=scale, seed=11)
        gg, ga = got["grow"], got["align"]
        assert got["map_n"] == tw["map_n"] and np.array_equal(got["map_track"], tw["map_track"]) and np.array_equal(got["map_row"], tw["map_row"])
        assert np.array_equal(gg["map_cam"], tg["map_cam"]) and np.array_equal(gg["map_obs"], tg["map_obs"]) and gg["status"] == tg["status"]
        assert np.array_equal(ga["match"], want["match"]) and (ga["n_old"], ga["n_common"], ga["n_terms"], ga["status"]) == (200, want["n_common"], want["n_terms"], want["status"])
        assert np.array_equal(_bits(np.float64(ga["scale"])), _bits(np.float64(want["scale"])))
        assert np.array_equal(_bits(got["X"]), _bits(want["X"]))
        for key in ("Rt_seed_a", "Rt_seed_b"):
            assert np.array_equal(_bits(got[key]), _bits(mu.rescale_pose(tw[key], want["scale"]))), key
        for c in range(3):
            assert np.array_equal(_bits(gg["Rt"][c]), _bits(mu.rescale_pose(tg["Rt"][c], want["scale"]))), c
        assert abs(want["scale"] - 1.0) > 1e-3
        # the installed map is the grown one, rescaled
        ref = _ctx()
        small.append(ref)
        ref.set_map(new_desc)
        ref.set_map_points(want["X"])
        _rows_are(set1[0], new_desc, "update_grow's map")
        d_q, d_f = _dev(s["desc"][2]), _dev(sc["cams"][2]["feat"])
        _same_frame(_frame_against_map(set1[0], d_q, n, d_f, sc["cams"][2]["cam"]), _frame_against_map(ref, d_q, n, d_f, sc["cams"][2]["cam"]), "update_grow's map")
        # a map that holds the seed pair's rows but not the grown map's: refused, the previous map still serves
        maxkp = (tg["n_seed_rows"] + tw["map_n"]) // 2
        assert 200 <= tg["n_seed_rows"] <= maxkp < tw["map_n"]
        tight = [_ctx(maxkp=maxkp) for _ in range(3)]
        small += tight
        tight[0].set_map(prev_desc)
        tight[0].set_map_points(prev_X)
        ref.set_map(prev_desc)
        ref.set_map_points(prev_X)
        with pytest.raises(CLCError) as e:
            abi.map_update_grow_batch_dev(tight, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], origin_R=origin_R, origin_C=origin_C, scale=scale, seed=11)
        assert e.value.status == abi.CLC_ERR_CAPACITY
        _rows_are(tight[0], prev_desc, "after the refusal")
        plain, _ = abi.map_update_batch_dev(tight, s["jobs"], [n] * 3, s["pair_cams"], s["dc"], origin_R=origin_R, origin_C=origin_C, scale=scale)
        assert plain["map_n"] == tg["n_seed_rows"]                # (the seed pair's map fits)
        _torch().cuda.synchronize()
    finally:
        for c in set1 + twins + small:
            c.close()


def test_a_camera_without_its_descriptor_block_is_refused():
    from coloc_amd import CLCError, abi
    ctx = _ctx()
    try:
        sc = _scene(3, 100, 71)
        pairs = _scene_pairs(sc, 60, 72)
        desc = _descriptors(100, sc["point_of"], 73)
        keep = []
        dp, dc = _dev_pairs(pairs, keep), _dev_cams(sc["cams"], keep, desc)
        no_block = [dc[0], dc[1], {k: v for k, v in dc[2].items() if k != "d_desc"}]
        with pytest.raises(CLCError) as e:
            ctx.map_build_grow_dev([100] * 3, dp, no_block, 0, sc["Rt"][0], sc["Rt"][1])
        assert e.value.status == abi.CLC_ERR_BAD_ARG
        assert ctx.map_build_dev([100] * 3, dp, no_block, 0, sc["Rt"][0], sc["Rt"][1])["map_n"] > 20       # (the plain build reads the lower seed camera's only)
        assert ctx.map_build_grow_dev([100] * 3, dp, dc, 0, sc["Rt"][0], sc["Rt"][1])["grow"]["resected"] == [False, False, True]
    finally:
        ctx.close()


# ---- 6. after_stream ---------------------------------------------------------------------------------------------------------------

def test_after_stream_orders_the_grown_build_behind_the_producer():
    """the edge lists, the features and the descriptors are written on torch's current stream behind a stretch of other work; only the
    event the call records on after_stream puts the launches behind it.  No torch.cuda.synchronize() in between."""
    torch = _torch()
    ctx = _ctx()
    try:
        sc = _scene(4, 400, 91)
        pairs = _scene_pairs(sc, 220, 92, wrong=0.05)
        rows = [400] * 4
        desc = _descriptors(400, sc["point_of"], 93)
        src = dict(q=[_dev(p["q"]) for p in pairs], t=[_dev(p["t"]) for p in pairs], feat=[_dev(c["feat"]) for c in sc["cams"]], desc=[_dev(d) for d in desc])
        dst = {k: [torch.zeros_like(v) for v in vs] for k, vs in src.items()}
        a = torch.randn(2048, 2048, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(20):
                a = (a @ a) * 1e-3
            for k in src:
                for d, s in zip(dst[k], src[k]):
                    d.copy_(s)
            dp = [dict(cam_a=p["cam_a"], cam_b=p["cam_b"], n=220, d_q=dst["q"][i].data_ptr(), d_t=dst["t"][i].data_ptr()) for i, p in enumerate(pairs)]
            dc = [dict(cam=c["cam"], d_feat=dst["feat"][i].data_ptr(), feat_stride=4, d_desc=dst["desc"][i].data_ptr()) for i, c in enumerate(sc["cams"])]
            got = ctx.map_build_grow_dev(rows, dp, dc, 1, sc["Rt"][0], sc["Rt"][2], after_stream=torch.cuda.current_stream().cuda_stream, seed=7)
        assert pairs[1]["cam_a"] == 0 and pairs[1]["cam_b"] == 2
        want = _statement(rows, pairs, sc, 1, got)
        _check_grown(got, want, "after_stream")
        assert got["grow"]["resected"] == [False, True, False, True] and want["n_added"] > 20
        _rows_are(ctx, np.stack([desc[c][r] for c, r in zip(got["grow"]["map_cam"], got["map_row"])]), "after_stream")
        torch.cuda.synchronize()
    finally:
        ctx.close()

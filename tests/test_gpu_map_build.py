"""The map built on the device (include/coloc_hip.h: clc_tracks_build_dev, clc_map_build_dev, clc_map_init_batch_dev).

Comparison rule: integers (track table, track ids, rows, counts) are compared EXACTLY with tests/map_host.py, the Python statement of the
rules; doubles are compared BIT FOR BIT with the host build of coloc_amd/csrc/map_math.h (tests/host/map_math_lib.cpp) fed the
undistorted pixels of tests/track_host.py, which has get_ud_pixel's bits (tests/test_track_abi.py)."""
import itertools

import numpy as np
import pytest

import inter_geometry_host
import map_host
import synth
import track_host

pytestmark = pytest.mark.gpu

W, H = 1280, 720
F0 = (1000.0, 640.0, 360.0)
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])


def _torch():
    import torch
    return torch


def _dev(a):
    """a numpy array (structured ones as bytes) on the GPU, complete before anything another stream enqueues"""
    torch = _torch()
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1) if a.dtype.names else a).cuda()
    torch.cuda.synchronize()
    return t


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _ctx(maxkp=4000):
    from coloc_amd import Context
    return Context(device=0, width=W, height=H, maxkp=maxkp, match_thresh=60)


def _dev_pairs(pairs, keep):
    """host pairs (map_host's form: cam_a, cam_b, q, t [, count, index]) -> the binding's pairs over device copies"""
    out = []
    for p in pairs:
        q, t = np.asarray(p["q"], dtype=np.int32), np.asarray(p["t"], dtype=np.int32)
        d = dict(cam_a=p["cam_a"], cam_b=p["cam_b"], n=len(q))
        if len(q):
            tq, tt = _dev(q), _dev(t)
            keep += [tq, tt]
            d.update(d_q=tq.data_ptr(), d_t=tt.data_ptr())
        if p.get("index") is not None:
            ti = _dev(np.asarray(p["index"], dtype=np.int32))
            keep.append(ti)
            d.update(d_index=ti.data_ptr(), n=len(p["index"]), n_list=len(q))
        if p.get("count") is not None:
            tc = _dev(np.array([p["count"], 12345], dtype=np.int32))
            keep.append(tc)
            d.update(d_n=tc.data_ptr())
        out.append(d)
    return out


def _tracks_on_device(ctx, rows, pairs):
    from coloc_amd import abi
    torch = _torch()
    keep = []
    dp = _dev_pairs(pairs, keep)
    cap = abi.tracks_capacity(rows, dp)
    d_table = torch.full((max(cap, 1) * len(rows),), -7, dtype=torch.int32, device="cuda")
    d_n = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.tracks_build_dev(rows, dp, d_table.data_ptr(), d_n.data_ptr(), None)
    ctx.sync()
    n = int(d_n.cpu()[0])
    table = d_table.cpu().numpy().reshape(-1, len(rows))
    assert 0 <= n <= cap and (cap == 0 or (table[n:cap] == -1).all())          # the room past the tracks is written too
    return table[:n].copy()


def _dev_cams(cams, keep, desc=None):
    out = []
    for c, spec in enumerate(cams):
        d = dict(cam=spec["cam"])
        if spec.get("kps") is not None:
            t = _dev(spec["kps"])
            d.update(d_kps=t.data_ptr())
        else:
            t = _dev(np.asarray(spec["feat"], dtype=np.float32))
            d.update(d_feat=t.data_ptr(), feat_stride=np.asarray(spec["feat"]).shape[1])
        keep.append(t)
        if desc is not None:
            td = _dev(desc[c])
            keep.append(td)
            d.update(d_desc=td.data_ptr())
        out.append(d)
    return out


def _check_map(got, want, what):
    assert got["n_tracks"] == len(want["track_feat"]), (what, got["n_tracks"], len(want["track_feat"]))
    assert np.array_equal(got["track_feat"], want["track_feat"]), what
    assert got["map_n"] == len(want["map_track"]), (what, got["map_n"], len(want["map_track"]))
    assert np.array_equal(got["map_track"], want["map_track"]) and np.array_equal(got["map_row"], want["map_row"]), what
    assert np.array_equal(_bits(got["X"]), _bits(want["X"])), (what, int((_bits(got["X"]) != _bits(want["X"])).sum()))


def _descriptors(n_points, rows_of, seed):
    """one random 512-bit descriptor per world point; camera c's row r carries the descriptor of point rows_of[c][r] with a few bits
    flipped"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_points, 64), dtype=np.uint8)
    out = []
    for pts in rows_of:
        d = base[pts].copy()
        for k in range(6):
            d[np.arange(len(pts)), rng.integers(0, 64, len(pts))] ^= (1 << rng.integers(0, 8, len(pts))).astype(np.uint8)
        out.append(d)
    return out


def _distort(x, cam):
    f, pp, k = cam[0], np.array(cam[1:3]), cam[3:6]
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


def _scene(n_cams, n_rows, seed, dist=None, noise=0.2):
    """a world of n_rows points seen by n_cams cameras side by side (camera c's row r shows point point_of[c][r], a permutation): float
    feature blocks of the DISTORTED pixels, the cameras, their [R|t]"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-5, 5, n_rows), rng.uniform(-3, 3, n_rows), rng.uniform(8, 20, n_rows)], 1)
    cams, Rts, point_of = [], [], []
    for c in range(n_cams):
        cam = F0 + (track_host.DISTORTIONS[c % 3] if dist is None else dist[c])
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


def _small_rot(rng):
    a, b = rng.uniform(-0.06, 0.06), rng.uniform(-0.03, 0.03)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return Ry @ Rx


def _scene_pairs(sc, n_matches, seed, wrong=0.1):
    """every camera pair a < b: n_matches random rows of a matched to the row of b that shows the same point -- `wrong` of them to a
    random row instead (K2NN is not one-to-one: conflicts, direct and transitive)"""
    rng = np.random.default_rng(seed)
    n_cams, n_rows = len(sc["cams"]), len(sc["X"])
    pairs = []
    for a, b in itertools.combinations(range(n_cams), 2):
        q = rng.choice(n_rows, n_matches, replace=False)
        t = sc["row_of"][b][sc["point_of"][a][q]]
        bad = rng.random(n_matches) < wrong
        t = np.where(bad, rng.integers(0, n_rows, n_matches), t)
        pairs.append(dict(cam_a=a, cam_b=b, q=q.astype(np.int32), t=t.astype(np.int32)))
    return pairs


# ---- tracks ------------------------------------------------------------------------------------------------------------------------

def _hand_pairs():
    """3 cameras x 300 rows (A, B, C = 0, 1, 2).  Every edge list is fed in DESCENDING order, so the larger roots are hooked first and a
    chain needs several hook steps to reach its smallest node."""
    ab, bc, ac = [], [], []
    # a chain of 3 through all cameras, the smallest node last; another that lacks camera A (no seed camera 0)
    ab.append((250, 260)); bc.append((260, 270))
    bc.append((40, 41))
    # a long zig-zag path A-B-C-A-B-... : 30 nodes in ONE component (many hook steps), dropped whole: it holds 10 rows of every camera
    for k in range(10):
        ab.append((100 + k, 100 + k)); bc.append((100 + k, 100 + k))
        if k:
            ac.append((100 + k, 100 + k - 1))
    # duplicate edges
    ab += [(7, 8), (7, 8), (7, 8)]
    # a direct conflict: two queries name one train
    ab += [(20, 30), (21, 30)]
    # a transitive conflict: A5-B7, B7-C2, C2-A9
    ab.append((5, 7)); bc.append((7, 2)); ac.append((9, 2))
    # plain pairs, one per pair of cameras, and rows out of range
    ab.append((299, 0)); bc.append((299, 299)); ac.append((0, 298)); ab.append((300, 5)); ac.append((3, -1))
    mk = lambda a, b, es: dict(cam_a=a, cam_b=b, q=[e[0] for e in sorted(es, reverse=True)], t=[e[1] for e in sorted(es, reverse=True)])
    return [mk(0, 1, ab), mk(1, 2, bc), mk(0, 2, ac),
            dict(cam_a=0, cam_b=2, q=[], t=[]),                                     # an empty pair
            dict(cam_a=0, cam_b=1, q=[150, 151], t=[150, 150], count=0)]            # and one whose device count says so


def test_hand_placed_tracks():
    ctx = _ctx()
    try:
        rows, pairs = [300, 300, 300], _hand_pairs()
        want = map_host.build_tracks(rows, pairs)
        got = _tracks_on_device(ctx, rows, pairs)
        assert np.array_equal(got, want), (got, want)
        have = [tuple(r) for r in got.tolist()]
        assert (250, 260, 270) in have and (-1, 40, 41) in have and (7, 8, -1) in have and (299, 0, -1) in have and (0, -1, 298) in have
        flat = {(c, r) for row in got for c, r in enumerate(row) if r >= 0}
        assert not any((c, 100 + k) in flat for c in range(3) for k in range(10))             # the zig-zag component
        assert not flat & {(0, 20), (0, 21), (1, 30), (0, 5), (1, 7), (2, 2), (0, 9), (0, 150), (0, 151)}      # conflicts; the counted-out pair
        assert have == sorted(have, key=lambda r: next((c, v) for c, v in enumerate(r) if v >= 0))             # ids in (camera, row) order
        # the same edges through an index list (a filter's inlier list over its pair lists), out-of-range indices ignored
        idx_pairs = []
        for p in pairs[:3]:
            n = len(p["q"])
            pad = np.concatenate([np.asarray(p["q"]), [11, 12]]), np.concatenate([np.asarray(p["t"]), [13, 13]])
            idx_pairs.append(dict(cam_a=p["cam_a"], cam_b=p["cam_b"], q=pad[0], t=pad[1], index=list(range(n - 1, -1, -1)) + [-1, n + 2, 1 << 20]))
        assert np.array_equal(map_host.build_tracks(rows, idx_pairs), want)
        assert np.array_equal(_tracks_on_device(ctx, rows, idx_pairs), want)
    finally:
        ctx.close()


def test_hand_placed_map_skips_tracks_without_a_seed_camera():
    ctx = _ctx()
    try:
        rows, pairs = [300, 300, 300], _hand_pairs()
        sc = _scene(3, 300, 31)
        desc = _descriptors(300, sc["point_of"], 32)
        keep = []
        got = ctx.map_build_dev(rows, _dev_pairs(pairs, keep), _dev_cams(sc["cams"], keep, desc), 0, sc["Rt"][0], sc["Rt"][1])
        want = map_host.build_map(rows, pairs, sc["cams"], 0, sc["Rt"][0], sc["Rt"][1])
        _check_map(got, want, "hand")
        lacking = [k for k, r in enumerate(want["track_feat"].tolist()) if r[0] < 0 or r[1] < 0]
        assert lacking and not set(lacking) & set(want["seed_tracks"].tolist())
    finally:
        ctx.close()


def test_eight_cameras_twice():
    """8 x 1 500 rows (not a multiple of 64), 1 100 matches per pair, 28 pairs: several edge workgroups per pair, 12 passes of the
    export's compaction and two of the seed's, with survivors in more than one of each; twice: nothing depends on scheduling"""
    ctx = _ctx(maxkp=4000)
    try:
        sc = _scene(8, 1500, 41)
        pairs = _scene_pairs(sc, 1100, 42, wrong=0.005)
        rows = [1500] * 8
        want = map_host.build_tracks(rows, pairs)
        first_node = np.array([next(1500 * c + r for c, r in enumerate(row) if r >= 0) for row in want.tolist()])
        assert len(want) > 1024 and len(set((first_node // 1024).tolist())) >= 2
        all_edges = sum(len(p["q"]) for p in pairs)
        assert 2 * len(want) < all_edges                       # (conflicts and longer tracks: the filter had work)
        got1 = _tracks_on_device(ctx, rows, pairs)
        got2 = _tracks_on_device(ctx, rows, pairs)
        assert np.array_equal(got1, want) and np.array_equal(got2, got1)
        desc = _descriptors(1500, sc["point_of"], 43)
        keep = []
        dp, dc = _dev_pairs(pairs, keep), _dev_cams(sc["cams"], keep, desc)
        seed = 9                                               # some pair in the middle: cameras (1, 4)
        a, b = pairs[seed]["cam_a"], pairs[seed]["cam_b"]
        wantm = map_host.build_map(rows, pairs, sc["cams"], seed, sc["Rt"][a], sc["Rt"][b])
        assert len(wantm["seed_tracks"]) > 300 and (wantm["map_track"] < 1024).any() and (wantm["map_track"] >= 1024).any()
        m1 = ctx.map_build_dev(rows, dp, dc, seed, sc["Rt"][a], sc["Rt"][b])
        m2 = ctx.map_build_dev(rows, dp, dc, seed, sc["Rt"][a], sc["Rt"][b])
        _check_map(m1, wantm, "8 cameras")
        _check_map(m2, wantm, "8 cameras, again")
        # the landmarks are the world's points where the track is a true one
        pt = sc["point_of"][a][wantm["map_row"]]
        err = np.linalg.norm(wantm["X"] - sc["X"][pt], axis=1)
        assert np.median(err) < 0.5
    finally:
        ctx.close()


# ---- the seed triangulation --------------------------------------------------------------------------------------------------------

def _acceptance_case(dist_a, dist_b, back):
    """two cameras, 64 + 6 points placed by hand, every point one track.  back: camera B stands at z = 40 and looks back at camera A."""
    rng = np.random.default_rng(5)
    cam_a, cam_b = F0 + dist_a, F0 + dist_b
    if back:
        Rb, Cb = np.diag([-1.0, 1.0, -1.0]), np.array([0.5, 0.0, 40.0])
    else:
        Rb, Cb = np.eye(3), np.array([2.0, 0.0, 0.0])
    Rtb = np.hstack([Rb, (-Rb @ Cb)[:, None]])
    n = 64
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(8, 30, n)], 1)
    special = np.array([[0.3, 0.2, -6.0],      # behind A
                        [1.0, -0.4, 99.9], [1.0, -0.4, 100.1],          # |Z| just below / just above 100
                        [0.2, 0.1, 55.0],       # beyond B when B looks back: behind B only
                        [-0.4, 0.3, -99.9], [-0.4, 0.3, -100.1]])
    X = np.vstack([X, special])
    feats = []
    for cam, Rt in ((cam_a, I34), (cam_b, Rtb)):
        u = (X @ Rt[:, :3].T + Rt[:, 3]) @ np.array([[cam[0], 0, cam[1]], [0, cam[0], cam[2]], [0, 0, 1.0]]).T
        f = np.zeros((len(X), 4), dtype=np.float32)
        f[:, :2] = _distort(u[:, :2] / u[:, 2:3], cam)
        feats.append(f)
    rows = [len(X), len(X)]
    perm = rng.permutation(len(X))                               # camera B's row of camera A's row r
    fb = np.zeros_like(feats[1])
    fb[perm] = feats[1]
    pairs = [dict(cam_a=0, cam_b=1, q=np.arange(len(X), dtype=np.int32), t=perm.astype(np.int32))]
    return X, rows, pairs, [dict(cam=cam_a, feat=feats[0]), dict(cam=cam_b, feat=fb)], Rtb


@pytest.mark.parametrize("back", [False, True])
@pytest.mark.parametrize("da,db", [(0, 0), (1, 2), (2, 1)])
def test_acceptance_rule(da, db, back):
    ctx = _ctx()
    try:
        X, rows, pairs, cams, Rtb = _acceptance_case(track_host.DISTORTIONS[da], track_host.DISTORTIONS[db], back)
        desc = _descriptors(len(X), [np.arange(len(X))] * 2, 6)
        keep = []
        got = ctx.map_build_dev(rows, _dev_pairs(pairs, keep), _dev_cams(cams, keep, desc), 0, I34, Rtb)
        want = map_host.build_map(rows, pairs, cams, 0, I34, Rtb)
        _check_map(got, want, ("acceptance", da, db, back))
        ok = want["seed_ok"]                                     # per track = per row of camera A
        assert len(ok) == 70 and ok[:64].all()
        assert np.abs(want["seed_X"][[64, 65, 66, 67, 68, 69]] - X[64:]).max() < 0.02          # the hand-placed points came back where they were put
        if not back:
            # B beside A, both looking along +z: behind A is behind both
            assert ok[64:].tolist() == [False, True, False, True, False, False]
        else:
            # B looks back from z = 40: z < 0 is behind A only, z > 40 behind B only -- kept unless |Z| > 100
            assert ok[64:].tolist() == [True, True, False, True, True, False]
    finally:
        ctx.close()


def test_one_side_keypoints_one_side_features():
    ctx = _ctx()
    try:
        n = 700
        rng = np.random.default_rng(8)
        kps = synth.random_keypoints(n, W, H, seed=81)
        kps["scale"][:64] = np.arange(64) % 8
        feat = np.zeros((n, 2), dtype=np.float32)
        feat[:] = track_host.feature_positions(synth.random_keypoints(n, W, H, seed=82)) + rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32)
        Rtb = np.hstack([_small_rot(rng), np.array([[-1.0], [0.05], [0.02]])])
        q = rng.choice(n, 500, replace=False).astype(np.int32)
        pairs = [dict(cam_a=0, cam_b=1, q=q, t=rng.permutation(n)[:500].astype(np.int32))]
        desc = _descriptors(n, [np.arange(n)] * 2, 83)
        for spec in ([dict(cam=F0 + track_host.DISTORTIONS[1], kps=kps), dict(cam=F0 + track_host.DISTORTIONS[2], feat=feat)],
                     [dict(cam=F0 + track_host.DISTORTIONS[2], feat=feat), dict(cam=F0 + track_host.DISTORTIONS[1], kps=kps)]):
            keep = []
            got = ctx.map_build_dev([n, n], _dev_pairs(pairs, keep), _dev_cams(spec, keep, desc), 0, I34, Rtb)
            want = map_host.build_map([n, n], pairs, spec, 0, I34, Rtb)
            assert len(want["seed_tracks"]) == 500 and 0 < len(want["map_track"]) < 500          # random rays: both outcomes occur
            _check_map(got, want, "kps | feat")
    finally:
        ctx.close()


# ---- the installed map -------------------------------------------------------------------------------------------------------------

def _frame_against_map(ctx, d_q, nq, d_feat, cam, seed=3):
    """match_map_dev + track_localize_dev of one frame on ctx -> (match, localisation result)"""
    torch = _torch()
    d_match = torch.full((nq,), -5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.match_map_dev(d_q.data_ptr(), nq, 60, d_match.data_ptr(), None)
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


def test_installed_map_serves_matching_and_localisation():
    """after map_build_dev the context matches and localises exactly like one given the host-gathered map through set_map +
    set_map_points"""
    ctx, ref = _ctx(), _ctx()
    try:
        sc = _scene(3, 900, 51)
        pairs = _scene_pairs(sc, 700, 52)
        rows = [900] * 3
        desc = _descriptors(900, sc["point_of"], 53)
        keep = []
        got = ctx.map_build_dev(rows, _dev_pairs(pairs, keep), _dev_cams(sc["cams"], keep, desc), 0, sc["Rt"][0], sc["Rt"][1])
        want = map_host.build_map(rows, pairs, sc["cams"], 0, sc["Rt"][0], sc["Rt"][1])
        _check_map(got, want, "installed")
        assert got["map_n"] > 300
        ref.set_map(desc[0][want["map_row"]])
        ref.set_map_points(want["X"])
        # camera 2's frame against the map
        d_q, d_f = _dev(desc[2]), _dev(sc["cams"][2]["feat"])
        a = _frame_against_map(ctx, d_q, 900, d_f, sc["cams"][2]["cam"])
        b = _frame_against_map(ref, d_q, 900, d_f, sc["cams"][2]["cam"])
        _same_frame(a, b, "installed map")
        assert (a[0] >= 0).sum() > 200 and a[1]["Rt"] is not None and len(a[1]["inliers"]) > 100
        assert np.abs(a[1]["Rt"] - sc["Rt"][2]).max() < 0.1                       # camera 2's pose
    finally:
        ctx.close()
        ref.close()


def test_capacity_keeps_the_previous_map_and_an_empty_map():
    from coloc_amd import CLCError, abi
    ctx, ref = _ctx(maxkp=900), _ctx(maxkp=900)
    try:
        sc = _scene(2, 1200, 61)
        desc = _descriptors(1200, sc["point_of"], 62)
        q = np.arange(1200, dtype=np.int32)
        t = sc["row_of"][1][sc["point_of"][0][q]].astype(np.int32)
        keep = []
        dc = _dev_cams(sc["cams"], keep, desc)
        small = [dict(cam_a=0, cam_b=1, q=q[:500], t=t[:500])]
        got = ctx.map_build_dev([1200, 1200], _dev_pairs(small, keep), dc, 0, sc["Rt"][0], sc["Rt"][1])
        want = map_host.build_map([1200, 1200], small, sc["cams"], 0, sc["Rt"][0], sc["Rt"][1])
        _check_map(got, want, "small")
        assert 400 < got["map_n"] <= 500
        ref.set_map(desc[0][want["map_row"]])
        ref.set_map_points(want["X"])
        d_q, d_f = _dev(desc[1][:900]), _dev(sc["cams"][1]["feat"][:900])
        before = _frame_against_map(ctx, d_q, 900, d_f, sc["cams"][1]["cam"])
        # 1 200 landmarks do not fit 900 rows: refused, and the previous map keeps working
        big = [dict(cam_a=0, cam_b=1, q=q, t=t)]
        assert len(map_host.build_map([1200, 1200], big, sc["cams"], 0, sc["Rt"][0], sc["Rt"][1])["map_track"]) > 900
        with pytest.raises(CLCError) as e:
            ctx.map_build_dev([1200, 1200], _dev_pairs(big, keep), dc, 0, sc["Rt"][0], sc["Rt"][1])
        assert e.value.status == abi.CLC_ERR_CAPACITY
        after = _frame_against_map(ctx, d_q, 900, d_f, sc["cams"][1]["cam"])
        _same_frame(after, before, "after the refusal")
        _same_frame(after, _frame_against_map(ref, d_q, 900, d_f, sc["cams"][1]["cam"]), "against the host-gathered map")
        assert after[1]["Rt"] is not None
        # no edge at all: no track, no landmark, an empty map
        none = [dict(cam_a=0, cam_b=1, q=[], t=[])]
        got = ctx.map_build_dev([1200, 1200], _dev_pairs(none, keep), dc, 0, sc["Rt"][0], sc["Rt"][1])
        assert got["n_tracks"] == 0 and got["map_n"] == 0 and len(got["X"]) == 0
        # 64 queries that all name one train row: one component, dropped whole
        clash = [dict(cam_a=0, cam_b=1, q=q[:64], t=np.full(64, 7, dtype=np.int32))]
        got = ctx.map_build_dev([1200, 1200], _dev_pairs(clash, keep), dc, 0, sc["Rt"][0], sc["Rt"][1])
        assert got["n_tracks"] == 0 and got["map_n"] == 0
        # tracks, but every landmark behind both cameras (the poses turned round): no map either
        turned = np.hstack([np.diag([-1.0, 1.0, -1.0]), np.zeros((3, 1))])
        got = ctx.map_build_dev([1200, 1200], _dev_pairs(small, keep), dc, 0, turned @ np.vstack([sc["Rt"][0], [0, 0, 0, 1.0]]), turned @ np.vstack([sc["Rt"][1], [0, 0, 0, 1.0]]))
        assert got["n_tracks"] == 500 and got["map_n"] == 0
        torch = _torch()
        d_match = torch.full((900,), -5, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.match_map_dev(d_q.data_ptr(), 900, 60, d_match.data_ptr(), None)
        ctx.sync()
        assert (d_match.cpu().numpy() == -1).all()
    finally:
        ctx.close()
        ref.close()


def test_bad_arguments():
    from coloc_amd import CLCError, abi
    ctx = _ctx()
    light = None
    try:
        from coloc_amd import Context
        light = Context(device=0, detector=False, matcher=False)
        sc = _scene(2, 100, 71)
        desc = _descriptors(100, sc["point_of"], 72)
        keep = []
        dc = _dev_cams(sc["cams"], keep, desc)
        q = np.arange(50, dtype=np.int32)
        dp = _dev_pairs([dict(cam_a=0, cam_b=1, q=q, t=q)], keep)
        good = dict(rows=[100, 100], pairs=dp, cams=dc, seed_pair=0, Rt_seed_a=I34, Rt_seed_b=I34)
        bad = [dict(good, rows=[100], cams=dc[:1]),                                              # fewer than two cameras
               dict(good, pairs=[dict(dp[0], cam_a=1, cam_b=1)]), dict(good, pairs=[dict(dp[0], cam_a=1, cam_b=0)]),      # cam_a >= cam_b
               dict(good, pairs=[dict(dp[0], cam_b=2)]),                                         # a camera that is not there
               dict(good, pairs=[dict(dp[0], d_q=dp[0]["d_q"] + 2)]), dict(good, pairs=[dict(dp[0], d_index=dp[0]["d_t"] + 1, n_list=50)]),     # misaligned
               dict(good, cams=[dict(dc[0], d_desc=dc[0]["d_desc"] + 8), dc[1]]), dict(good, cams=[dc[0], dict(dc[1], d_feat=dc[1]["d_feat"] + 2)]),
               dict(good, cams=[dict(dc[0], d_kps=dc[0]["d_feat"]), dc[1]]),                      # both
               dict(good, cams=[dc[0], dict(cam=dc[1]["cam"], d_desc=dc[1]["d_desc"])]),          # neither
               dict(good, seed_pair=1), dict(good, seed_pair=-1),
               dict(good, pairs=[dict(dp[0], n=-1)])]
        for b in bad:
            with pytest.raises(CLCError) as e:
                ctx.map_build_dev(**b)
            assert e.value.status == abi.CLC_ERR_BAD_ARG, b
        torch = _torch()
        d_tab, d_n = torch.zeros(200, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
        for rows, pairs, tab, n in (([100], dp, d_tab.data_ptr(), d_n.data_ptr()), ([100, 100], [dict(dp[0], cam_a=1, cam_b=0)], d_tab.data_ptr(), d_n.data_ptr()),
                                    ([100, 100], dp, d_tab.data_ptr(), None), ([100, 100], dp, None, d_n.data_ptr()), ([100, 100], dp, d_tab.data_ptr() + 2, d_n.data_ptr())):
            with pytest.raises(CLCError) as e:
                ctx.tracks_build_dev(rows, pairs, tab, n, None)
            assert e.value.status == abi.CLC_ERR_BAD_ARG
        with pytest.raises(CLCError) as e:                                                        # no matcher: nowhere to install a map
            light.map_build_dev(**good)
        assert e.value.status == abi.CLC_ERR_STATE
        light.tracks_build_dev([100, 100], dp, d_tab.data_ptr(), d_n.data_ptr(), None)             # the tracks alone need none
        light.sync()
        assert int(d_n.cpu()[0]) == 50
        got = ctx.map_build_dev(**good)                                                           # the context is usable afterwards
        assert got["n_tracks"] == 50
    finally:
        ctx.close()
        if light is not None:
            light.close()


def test_after_stream_orders_the_build_behind_the_producer():
    """the edge lists, the features and the descriptors are written on torch's current stream behind a stretch of other work; the
    context's stream is non-blocking, so only the event the call records on after_stream puts the launches behind it.  No
    torch.cuda.synchronize() in between."""
    torch = _torch()
    ctx = _ctx()
    try:
        sc = _scene(3, 600, 91)
        pairs = _scene_pairs(sc, 450, 92)
        rows = [600] * 3
        desc = _descriptors(600, sc["point_of"], 93)
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
            dp = [dict(cam_a=p["cam_a"], cam_b=p["cam_b"], n=450, d_q=dst["q"][i].data_ptr(), d_t=dst["t"][i].data_ptr()) for i, p in enumerate(pairs)]
            dc = [dict(cam=c["cam"], d_feat=dst["feat"][i].data_ptr(), feat_stride=4, d_desc=dst["desc"][i].data_ptr()) for i, c in enumerate(sc["cams"])]
            got = ctx.map_build_dev(rows, dp, dc, 1, sc["Rt"][0], sc["Rt"][2], after_stream=torch.cuda.current_stream().cuda_stream)
        want = map_host.build_map(rows, pairs, sc["cams"], 1, sc["Rt"][0], sc["Rt"][2])
        assert pairs[1]["cam_a"] == 0 and pairs[1]["cam_b"] == 2 and len(want["map_track"]) > 200
        _check_map(got, want, "after_stream")
        torch.cuda.synchronize()
    finally:
        ctx.close()


def test_map_serves_other_streams_as_soon_as_the_call_returns():
    """A context's stream is non-blocking, and a streaming host matches against the map on a stream of its own.  Straight after
    map_build_dev returns, with NO host synchronisation, a foreign stream (1) overwrites the seed camera's descriptor block -- the next
    frame described into it -- and (2) runs match_map_dev.  The map must already be complete and the block no longer read: the result
    is that of a context given the host-gathered map through set_map."""
    torch = _torch()
    ctx, ref = _ctx(maxkp=8000), _ctx(maxkp=8000)
    try:
        n = 8000
        sc = _scene(2, n, 111)
        desc = _descriptors(n, sc["point_of"], 112)
        q = np.arange(n, dtype=np.int32)
        pairs = [dict(cam_a=0, cam_b=1, q=q, t=sc["row_of"][1][sc["point_of"][0][q]].astype(np.int32))]
        want = map_host.build_map([n, n], pairs, sc["cams"], 0, sc["Rt"][0], sc["Rt"][1])
        assert len(want["map_track"]) > 7000
        ref.set_map(desc[0][want["map_row"]])
        keep = []
        dp = _dev_pairs(pairs, keep)
        d_feat, d_desc = [_dev(c["feat"]) for c in sc["cams"]], [_dev(d) for d in desc]
        dc = [dict(cam=c["cam"], d_feat=d_feat[i].data_ptr(), feat_stride=4, d_desc=d_desc[i].data_ptr()) for i, c in enumerate(sc["cams"])]
        d_q = _dev(desc[1])
        d_match, d_ref = (torch.full((n,), -5, dtype=torch.int32, device="cuda") for _ in range(2))
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        for rep in range(3):                                     # (the second and third builds replace a map that is in use)
            d_desc[0].copy_(torch.from_numpy(desc[0]))
            d_match.fill_(-5)
            torch.cuda.synchronize()
            got = ctx.map_build_dev([n, n], dp, dc, 0, sc["Rt"][0], sc["Rt"][1])
            with torch.cuda.stream(side):
                d_desc[0].zero_()
                ctx.match_map_dev(d_q.data_ptr(), n, 60, d_match.data_ptr(), side.cuda_stream)
            side.synchronize()
            _check_map(got, want, ("foreign stream", rep))
            ref.match_map_dev(d_q.data_ptr(), n, 60, d_ref.data_ptr(), None)
            ref.sync()
            m = d_match.cpu().numpy()
            assert np.array_equal(m, d_ref.cpu().numpy()), (rep, int((m != d_ref.cpu().numpy()).sum()))
            assert (m >= 0).sum() > 7000
    finally:
        ctx.close()
        ref.close()


# ---- the composition ---------------------------------------------------------------------------------------------------------------

def test_map_init_equals_filter_selection_and_build():
    """clc_map_init_batch_dev on a 3-camera scene against clc_pair_filter_batch_dev + the host's selection (13 inliers, the chirality
    vote of the host build of inter_geometry.cpp, the seed rule, seed_poses) + clc_map_build_dev on the inliers' edges.  Pair (1, 2) has
    ten matches: below 13 inliers, left out of the tracks."""
    from coloc_amd import abi
    torch = _torch()
    ctxs = [_ctx() for _ in range(3)]
    refs = [_ctx() for _ in range(3)]
    other = _ctx()
    try:
        n = 800
        sc = _scene(3, n, 101, dist=[track_host.DISTORTIONS[0], track_host.DISTORTIONS[1], track_host.DISTORTIONS[2]], noise=0.3)
        desc = _descriptors(n, sc["point_of"], 102)
        rng = np.random.default_rng(103)
        pair_cams = [(0, 1), (0, 2), (1, 2)]
        matches = []
        for k, (a, b) in enumerate(pair_cams):
            m = np.full(n, -1, dtype=np.int32)
            q = rng.choice(n, (500, 420, 10)[k], replace=False)
            m[q] = sc["row_of"][b][sc["point_of"][a][q]]
            wrong = q[rng.random(len(q)) < 0.2]
            m[wrong] = rng.integers(0, n, len(wrong))
            matches.append(m)
        d_match, d_feat = [_dev(m) for m in matches], [_dev(c["feat"]) for c in sc["cams"]]
        d_desc = [_dev(d) for d in desc]
        jobs = [dict(d_match=d_match[k].data_ptr(), nq=n, nt=n, cam_a=sc["cams"][a]["cam"], cam_b=sc["cams"][b]["cam"], d_feat_a=d_feat[a].data_ptr(),
                     feat_stride_a=4, d_feat_b=d_feat[b].data_ptr(), feat_stride_b=4, img_wh=(W, H), seed=5 + k) for k, (a, b) in enumerate(pair_cams)]
        dc = [dict(cam=c["cam"], d_feat=d_feat[i].data_ptr(), feat_stride=4, d_desc=d_desc[i].data_ptr()) for i, c in enumerate(sc["cams"])]
        origin_R, origin_C, scale = np.eye(3), np.array([0.3, -0.2, 0.1]), 0.8
        got, filt = abi.map_init_batch_dev(ctxs, jobs, [n] * 3, pair_cams, dc, origin_R=origin_R, origin_C=origin_C, scale=scale)
        # the same by hand
        ref_filt = abi.pair_filter_batch_dev(refs, "E", jobs)
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
        assert entered == [True, True, False] and got["entered"] == entered
        assert len(ref_filt[2]["inliers"]) < 13
        counts = [len(r["inliers"]) if e else 0 for r, e in zip(ref_filt, entered)]
        seed = int(np.argmax(counts))                                # (argmax: the first of equals)
        assert got["seed_pair"] == seed == 0
        Rt_a, Rt_b = abi.seed_poses(origin_R, origin_C, votes[seed]["R"], map_host.pose_center(votes[seed]["R"], votes[seed]["t"]), scale)
        assert np.array_equal(_bits(got["Rt_seed_a"]), _bits(Rt_a)) and np.array_equal(_bits(got["Rt_seed_b"]), _bits(Rt_b))
        host_pairs = [dict(cam_a=a, cam_b=b, q=r["pair_q"][r["inliers"]], t=r["pair_t"][r["inliers"]]) for (a, b), r, e in zip(pair_cams, ref_filt, entered) if e]
        want = map_host.build_map([n] * 3, host_pairs, sc["cams"], 0, Rt_a, Rt_b)
        _check_map(got, want, "map_init")
        keep = []
        built = other.map_build_dev([n] * 3, _dev_pairs(host_pairs, keep), dc, 0, Rt_a, Rt_b)
        _check_map(built, want, "filter + selection + build")
        assert got["map_n"] > 150
        # pair (1, 2)'s matches joined nothing: no track holds cameras 1 and 2 without camera 0
        assert not ((got["track_feat"][:, 0] < 0)).any()
        # and both contexts now serve the same map
        d_q = _dev(desc[2])
        a = _frame_against_map(ctxs[0], d_q, n, d_feat[2], sc["cams"][2]["cam"])
        b = _frame_against_map(other, d_q, n, d_feat[2], sc["cams"][2]["cam"])
        _same_frame(a, b, "map_init's map")
        assert (a[0] >= 0).sum() > 100
        torch.cuda.synchronize()
    finally:
        for c in ctxs + refs + [other]:
            c.close()

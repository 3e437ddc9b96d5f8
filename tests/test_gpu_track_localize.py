"""Localizer::setupTracks on the device and the pose solve that starts from it (include/coloc_hip.h: clc_set_map_points,
clc_track_build_dev, clc_track_localize_dev, clc_track_localize_batch_dev).

Every comparison is EXACT (bit patterns): the track kernel runs the IEEE operations of tests/track_host.py (the numpy restatement of
Localizer.hpp:59-75 and Pinhole_Intrinsic_Radial_K3::get_ud_pixel, held to the host member's bits in tests/test_track_abi.py) in the same
order, and the solve behind it is the one clc_pnp_acransac / clc_pnp_localize_ac run on the host-gathered copy of the same tracks."""
import numpy as np
import pytest

import synth
import track_host

pytestmark = pytest.mark.gpu

W, H = 1280, 720
CAM0 = (1000.0, 640.0, 360.0)


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


def _light_ctx():
    from coloc_amd import Context
    return Context(device=0, detector=False, matcher=False)


def _random_match(rng, nq, map_n, mode="mixed"):
    if mode == "none":
        return np.full(nq, -1, dtype=np.int32)
    m = rng.integers(0, map_n, nq).astype(np.int32)
    if mode == "all":
        return m
    u = rng.random(nq)
    m[u < 0.25] = -1
    m[(u >= 0.25) & (u < 0.33)] = map_n + rng.integers(0, 1000, nq)[(u >= 0.25) & (u < 0.33)]      # past the map: "no match"
    m[(u >= 0.33) & (u < 0.40)] = -2 - rng.integers(0, 1 << 20, nq)[(u >= 0.33) & (u < 0.40)]     # negative other than -1
    return m


def _build_on_device(ctx, match, count, cam, kps=None, feat=None, stride=4):
    """clc_track_build_dev on fresh device buffers -> (N, query, map, X, x)"""
    torch = _torch()
    nq = len(match)
    d_match = _dev(match)
    d_X = torch.full((3 * max(nq, 1),), np.nan, dtype=torch.float64, device="cuda")
    d_x = torch.full((2 * max(nq, 1),), np.nan, dtype=torch.float64, device="cuda")
    d_q = torch.full((max(nq, 1),), -9, dtype=torch.int32, device="cuda")
    d_m = torch.full((max(nq, 1),), -9, dtype=torch.int32, device="cuda")
    d_n = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    d_cnt = None if count is None else _dev(np.array([count, count + 17], dtype=np.uint32).view(np.int32))
    d_kps = None if kps is None else _dev(kps)
    d_feat = None if feat is None else _dev(feat)
    torch.cuda.synchronize()
    ctx.track_build_dev(d_X.data_ptr(), d_x.data_ptr(), d_q.data_ptr(), d_m.data_ptr(), d_n.data_ptr(), None,
                        d_match=d_match.data_ptr(), nq=nq, cam=cam, d_kps=None if d_kps is None else d_kps.data_ptr(),
                        d_feat=None if d_feat is None else d_feat.data_ptr(), feat_stride=stride,
                        d_count=None if d_cnt is None else d_cnt.data_ptr())
    ctx.sync()
    N = int(d_n.cpu()[0])
    return N, d_q.cpu().numpy()[:N], d_m.cpu().numpy()[:N], d_X.cpu().numpy()[:3 * N].reshape(-1, 3), d_x.cpu().numpy()[:2 * N].reshape(-1, 2)


def _check_tracks(got, want, what):
    N, q, m, X, x = got
    wq, wm, wX, wx = want
    assert N == len(wq), (what, N, len(wq))
    assert np.array_equal(q, wq) and np.array_equal(m, wm), what
    assert np.array_equal(_bits(X), _bits(wX)), what
    assert np.array_equal(_bits(x), _bits(wx)), (what, int((_bits(x) != _bits(wx)).sum()))


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 1000, 10000])
def test_tracks_equal_the_host_rule(nq):
    ctx = _light_ctx()
    try:
        rng = np.random.default_rng(100 + nq)
        map_n = 3000
        map_X = rng.uniform(-5, 5, (map_n, 3)) + [0, 0, 12]
        ctx.set_map_points(map_X)
        kps = synth.random_keypoints(nq, W, H, seed=nq)
        kps["scale"][:min(nq, 64)] = np.arange(min(nq, 64)) % 8            # all 8 levels wherever there is room for them
        if nq >= 64:
            assert len(np.unique(kps["scale"])) == 8
        feat = np.zeros((nq, 4), dtype=np.float32)
        feat[:, :2] = np.stack([rng.uniform(0, W, nq), rng.uniform(0, H, nq)], 1)
        feat[:, 2:] = 7.0
        for k in track_host.DISTORTIONS:
            cam = CAM0 + k
            for mode in ("mixed", "none", "all"):
                match = _random_match(rng, nq, map_n, mode)
                if mode != "none":
                    # a keypoint exactly on the principal point, matched
                    j = nq // 2
                    kps[j] = (640, 360, 0, 0.0, 0)
                    feat[j, :2] = (640.0, 360.0)
                    match[j] = 7
                for count in (None, nq, max(nq - 1 - nq // 3, 0), nq + 5):
                    what = (nq, k, mode, count)
                    _check_tracks(_build_on_device(ctx, match, count, cam, kps=kps), track_host.build_tracks(match, map_X, cam, kps=kps, count=count), what + ("kps",))
                    _check_tracks(_build_on_device(ctx, match, count, cam, feat=feat), track_host.build_tracks(match, map_X, cam, feat=feat, count=count), what + ("feat",))
            if nq >= 1000:
                got = _build_on_device(ctx, match, None, cam, kps=kps)
                on_pp = np.nonzero(got[1] == nq // 2)[0]
                assert len(on_pp) == 1 and got[4][on_pp[0]].tolist() == [640.0, 360.0]          # r2 == 0: the pixel itself
    finally:
        ctx.close()


def test_tracks_feature_stride_two():
    """d_feat with a stride of its own (a packed x, y block)"""
    ctx = _light_ctx()
    try:
        rng = np.random.default_rng(5)
        map_X = rng.uniform(-5, 5, (500, 3))
        ctx.set_map_points(map_X)
        match = _random_match(rng, 700, 500)
        feat = np.stack([rng.uniform(0, W, 700), rng.uniform(0, H, 700)], 1).astype(np.float32)
        cam = CAM0 + track_host.DISTORTIONS[2]
        _check_tracks(_build_on_device(ctx, match, None, cam, feat=feat, stride=2), track_host.build_tracks(match, map_X, cam, feat=feat), "stride 2")
    finally:
        ctx.close()


def _distort(x, cam):
    f, pp, k = cam[0], np.array(cam[1:3]), cam[3:6]
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


def _scattered_scene(n, seed, cam, map_n=None, map_off=0, map_X=None):
    """synth.pnp_scene (30 % outliers, its defaults) scattered into a d_match / feature / map-point layout: n tracks among 1.6 n queries;
    -> (match, feat (nq, 4) float32, map_X)"""
    sc = synth.pnp_scene(n, seed=seed)
    assert np.array_equal(sc["K"], np.array([[cam[0], 0, cam[1]], [0, cam[0], cam[2]], [0, 0, 1.0]]))
    rng = np.random.default_rng(seed + 1)
    nq = int(1.6 * n) + 3
    if map_X is None:
        map_n = int(1.3 * n) + 5
        map_X = rng.uniform(-5, 5, (map_n, 3)) + [0, 0, 12]
        rows = rng.choice(map_n, n, replace=False)
    else:
        rows = map_off + rng.permutation(n)
    map_X[rows] = sc["X"]
    qs = np.sort(rng.choice(nq, n, replace=False))
    match = np.full(nq, -1, dtype=np.int32)
    match[qs] = rows
    feat = np.zeros((nq, 4), dtype=np.float32)
    feat[:, :2] = np.stack([rng.uniform(0, W, nq), rng.uniform(0, H, nq)], 1)
    feat[qs, :2] = _distort(sc["x"], cam)                        # the detector sees distorted pixels, stored as floats
    return match, feat, map_X


def _host_path(ctx, match, feat, map_X, cam, seed, refine, kps=None):
    """today's path: the host-gathered copy of the tracks through clc_pnp_acransac / clc_pnp_localize_ac (iterations: the one-job batch)"""
    from coloc_amd import abi
    q, m, X, x = track_host.build_tracks(match, map_X, cam, feat=feat, kps=kps)
    K = np.array([[cam[0], 0, cam[1]], [0, cam[0], cam[2]], [0, 0, 1.0]])
    r = ctx.pnp_acransac(X, x, K, seed=seed, refine=refine)
    if refine:
        rb = abi.pnp_localize_batch([ctx], [(X, x, K)], seeds=[seed], refine=True)[0]
        assert np.array_equal(rb["inliers"], r["inliers"])
        r["iterations"] = rb["iterations"]
    r.update(track_query=q, track_map=m, n_tracks=len(q))
    return r


def _same_pose(got, want, refine, what):
    assert got["n_tracks"] == want["n_tracks"], what
    assert np.array_equal(got["track_query"], want["track_query"]) and np.array_equal(got["track_map"], want["track_map"]), what
    assert np.array_equal(got["inliers"], want["inliers"]), what          # order included
    assert np.array_equal(got["mask"], want["mask"]), what
    assert (got["Rt"] is None) == (want["Rt"] is None), what
    if want["Rt"] is not None:
        assert np.array_equal(_bits(got["Rt"]), _bits(want["Rt"])), what
    assert got["error_max"] == want["error_max"] and got["iterations"] == want["iterations"], (what, got["iterations"], want["iterations"])
    if refine and want["Rt"] is not None:
        assert np.array_equal(_bits(got["cov"]), _bits(want["cov"])), what
        assert got["rmse"] == want["rmse"], what


@pytest.mark.parametrize("n", [200, 1000, 5000])
@pytest.mark.parametrize("refine", [True, False])
def test_pose_equals_the_host_gathered_solve(n, refine):
    ctx = _light_ctx()
    try:
        cam = CAM0 + track_host.DISTORTIONS[1]
        match, feat, map_X = _scattered_scene(n, 4000 + n, cam)
        ctx.set_map_points(map_X)
        d_match, d_feat = _dev(match), _dev(feat)
        for seed in (1, 7):
            got = ctx.track_localize_dev(d_match=d_match.data_ptr(), nq=len(match), cam=cam, d_feat=d_feat.data_ptr(), feat_stride=4,
                                         seed=seed, refine=refine)
            want = _host_path(ctx, match, feat, map_X, cam, seed, refine)
            assert want["Rt"] is not None and len(want["inliers"]) > 0.5 * n
            _same_pose(got, want, refine, (n, refine, seed))
    finally:
        ctx.close()


@pytest.mark.parametrize("n_jobs", [1, 3, 8])
def test_batch_equals_the_single_calls(n_jobs):
    """one shared map, one camera frame per job; 8 jobs run in lockstep, fewer interleaved (acr_lockstep)"""
    from coloc_amd import abi
    ctxs = [_light_ctx() for _ in range(n_jobs)]
    single = _light_ctx()
    try:
        cam = CAM0 + track_host.DISTORTIONS[2]
        sizes = [300 + 90 * j for j in range(n_jobs)]
        map_X = np.random.default_rng(3).uniform(-5, 5, (sum(sizes) + 50, 3)) + [0, 0, 12]
        frames, off = [], 0
        for j, n in enumerate(sizes):
            match, feat, _ = _scattered_scene(n, 900 + j, cam, map_off=off, map_X=map_X)
            frames.append((match, feat))
            off += n
        ctxs[0].set_map_points(map_X)
        single.set_map_points(map_X)
        dev = [(_dev(m), _dev(f)) for m, f in frames]
        jobs = [dict(d_match=dm.data_ptr(), nq=len(frames[j][0]), cam=cam, d_feat=df.data_ptr(), feat_stride=4, seed=11 + j, refine=True)
                for j, (dm, df) in enumerate(dev)]
        for rep in range(2):                                    # (a second frame through the same contexts and track blocks)
            got = abi.track_localize_batch_dev(ctxs, jobs)
            for j in range(n_jobs):
                one = single.track_localize_dev(**jobs[j])
                assert one["Rt"] is not None
                _same_pose(got[j], one, True, (n_jobs, j, rep))
                _same_pose(got[j], _host_path(single, frames[j][0], frames[j][1], map_X, cam, 11 + j, True), True, (n_jobs, j, rep, "host"))
    finally:
        for c in ctxs + [single]:
            c.close()


def test_real_front_end_without_a_host_trip():
    """rendered plane -> clc_detect_dev -> clc_describe_detected_dev -> clc_match_map_dev -> clc_track_localize_dev with the detector's own
    count, nothing copied in between, against today's host path on the same frame (download, numpy gather, pnp_acransac)"""
    torch = _torch()
    from coloc_amd import Context
    w, h, cap, ppu = 640, 480, 6000, 100.0
    K = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1.0]])
    cam = (520.0, 320.0, 240.0, 0.0, 0.0, 0.0)
    tex = synth.plane_texture()
    ctx = Context(device=0, width=w, height=h, maxkp=cap, match_thresh=60)
    try:
        Ra, ta = synth.look_at_plane_pose((7.0, 7.0), 5.2)
        Rb, tb = synth.look_at_plane_pose((7.25, 6.85), 5.0, yaw=0.05, tilt=(0.03, -0.02))
        kps_a, desc_a, _ = ctx.detect_and_describe(synth.render_plane(tex, ppu, K, Ra, ta, w, h), capacity=cap)
        Xmap = synth.backproject_to_plane(track_host.feature_positions(kps_a).astype(np.float64), K, Ra, ta)
        ctx.set_map(desc_a)
        ctx.set_map_points(Xmap)
        img = _dev(synth.render_plane(tex, ppu, K, Rb, tb, w, h))
        d_match = torch.full((cap,), -5, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        d_kps, d_cnt, d_desc = ctx.detect_buffers()
        ctx.pyramid_build_dev(img.data_ptr(), w, h, w, None)
        ctx.detect_dev(None)
        ctx.describe_detected_dev(None, None)
        ctx.match_map_dev(d_desc, cap, 60, d_match.data_ptr(), None)          # the PLANNED size: the count stays on the device
        got = ctx.track_localize_dev(d_match=d_match.data_ptr(), nq=cap, cam=cam, d_kps=d_kps, d_count=d_cnt, seed=3, refine=True)
        # today's path on the same frame
        ctx.sync()
        kps = ctx.detect(capacity=cap)[0]                        # the same pyramid through the host entry: the same keypoints
        n = len(kps)
        match = d_match.cpu().numpy()[:n]
        assert n > 800 and (match >= 0).sum() > 150
        want = _host_path(ctx, match, None, Xmap, cam, 3, True, kps=kps)
        assert want["Rt"] is not None
        _same_pose(got, want, True, "front end")
        R_est, t_est = got["Rt"][:, :3], got["Rt"][:, 3]
        assert np.linalg.norm(-R_est.T @ t_est + Rb.T @ tb) < 0.1
    finally:
        ctx.close()


def test_after_stream_orders_the_call_behind_the_producer():
    """d_match is written on torch's current stream behind a stretch of other work; the context's stream is non-blocking, so only the
    event the call records on after_stream puts the track launch behind it.  No torch.cuda.synchronize() before the call."""
    torch = _torch()
    ctx = _light_ctx()
    try:
        cam = CAM0 + track_host.DISTORTIONS[1]
        match, feat, map_X = _scattered_scene(1000, 5000, cam)
        ctx.set_map_points(map_X)
        d_src, d_feat = _dev(match), _dev(feat)
        d_match = torch.full((len(match),), -1, dtype=torch.int32, device="cuda")
        a = torch.randn(2048, 2048, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(20):
                a = (a @ a) * 1e-3
            d_match.copy_(d_src)
            got = ctx.track_localize_dev(d_match=d_match.data_ptr(), nq=len(match), cam=cam, d_feat=d_feat.data_ptr(), seed=1, refine=True,
                                         after_stream=torch.cuda.current_stream().cuda_stream)
        want = _host_path(ctx, match, feat, map_X, cam, 1, True)
        assert want["n_tracks"] == 1000
        _same_pose(got, want, True, "after_stream")
        torch.cuda.synchronize()
    finally:
        ctx.close()


def test_edges():
    from coloc_amd import CLCError, abi
    ctx = _light_ctx()
    try:
        cam = CAM0 + (0.0, 0.0, 0.0)
        match = np.full(50, -1, dtype=np.int32)
        match[[3, 17, 40]] = [0, 1, 2]
        feat = np.random.default_rng(0).uniform(0, 700, (50, 4)).astype(np.float32)
        d_match, d_feat = _dev(match), _dev(feat)
        job = dict(d_match=d_match.data_ptr(), nq=50, cam=cam, d_feat=d_feat.data_ptr())
        with pytest.raises(CLCError) as e:                      # no map points yet
            ctx.track_localize_dev(**job)
        assert e.value.status == abi.CLC_ERR_STATE
        ctx.set_map_points(np.arange(30, dtype=np.float64).reshape(10, 3))
        r = ctx.track_localize_dev(**job)                       # N = 3 <= 3: OK, no model
        assert r["n_tracks"] == 3 and len(r["inliers"]) == 0 and r["Rt"] is None and r["status"] == abi.CLC_OK
        assert r["track_query"].tolist() == [3, 17, 40] and r["track_map"].tolist() == [0, 1, 2]
        for bad in (dict(job, d_feat=None), dict(job, d_kps=d_feat.data_ptr())):      # neither / both 2-D forms
            with pytest.raises(CLCError) as e:
                ctx.track_localize_dev(**bad)
            assert e.value.status == abi.CLC_ERR_BAD_ARG
        ctx.set_map_points(np.zeros((0, 3)))                    # cleared
        with pytest.raises(CLCError) as e:
            ctx.track_localize_dev(**job)
        assert e.value.status == abi.CLC_ERR_STATE
        # the context is usable afterwards
        cam2 = CAM0 + track_host.DISTORTIONS[1]
        match2, feat2, map_X = _scattered_scene(300, 77, cam2)
        ctx.set_map_points(map_X)
        d_m2, d_f2 = _dev(match2), _dev(feat2)
        got = ctx.track_localize_dev(d_match=d_m2.data_ptr(), nq=len(match2), cam=cam2, d_feat=d_f2.data_ptr(), seed=2)
        _same_pose(got, _host_path(ctx, match2, feat2, map_X, cam2, 2, True), True, "after the edges")
    finally:
        ctx.close()


def test_fewer_map_points_than_map_rows_is_a_state_error():
    from coloc_amd import CLCError, Context, abi
    ctx = Context(device=0, width=64, height=64, maxkp=256, detector=False)
    try:
        ctx.set_map(np.zeros((100, 64), dtype=np.uint8))
        ctx.set_map_points(np.zeros((60, 3)))
        d_match, d_feat = _dev(np.zeros(8, dtype=np.int32)), _dev(np.zeros((8, 4), dtype=np.float32))
        with pytest.raises(CLCError) as e:
            ctx.track_localize_dev(d_match=d_match.data_ptr(), nq=8, cam=CAM0 + (0.0, 0.0, 0.0), d_feat=d_feat.data_ptr())
        assert e.value.status == abi.CLC_ERR_STATE
    finally:
        ctx.close()

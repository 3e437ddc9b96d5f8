"""The gather of RobustMatcher::computeRelativePose on the device and the two-view filter that starts from it (include/coloc_hip.h:
clc_pair_build_dev, clc_pair_filter_dev, clc_pair_filter_batch_dev).

Every comparison is EXACT (bit patterns, no tolerance): the pair kernel runs the IEEE operations of tests/pair_host.py (the numpy
restatement of RobustMatcher.hpp:393-398 over Pinhole_Intrinsic_Radial_K3::get_ud_pixel, held to the host member's bits in
tests/test_pair_host.py) in the same order, and the solve behind it is the one clc_two_view_acransac runs on the host-gathered copy of
the same correspondences."""
import numpy as np
import pytest

import pair_host
import synth
import track_host
import twoview_host

pytestmark = pytest.mark.gpu

W, H = 1280, 720
F0 = tuple(float(v) for v in (twoview_host.K_DEFAULT[0, 0], twoview_host.K_DEFAULT[0, 2], twoview_host.K_DEFAULT[1, 2]))
SAMPLE = {"E": 5, "F": 7, "H": 4}


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


def _random_match(rng, nq, nt, mode="mixed"):
    if mode == "none":
        return np.full(nq, -1, dtype=np.int32)
    m = rng.integers(0, nt, nq).astype(np.int32)
    if mode == "all":
        return m
    u = rng.random(nq)
    m[u < 0.25] = -1
    m[(u >= 0.25) & (u < 0.33)] = nt + rng.integers(0, 1000, nq)[(u >= 0.25) & (u < 0.33)]          # past camera B's rows: "no match"
    m[(u >= 0.33) & (u < 0.40)] = -2 - rng.integers(0, 1 << 20, nq)[(u >= 0.33) & (u < 0.40)]        # negative other than -1
    return m


def _build_on_device(ctx, match, nt, camA, camB, kpsA=None, featA=None, strideA=4, kpsB=None, featB=None, strideB=4, countA=None, countB=None):
    """clc_pair_build_dev on fresh device buffers -> (N, pair_q, pair_t, x1, x2)"""
    torch = _torch()
    nq = len(match)
    d_match = _dev(match)
    d_x1 = torch.full((2 * max(nq, 1),), np.nan, dtype=torch.float64, device="cuda")
    d_x2 = torch.full((2 * max(nq, 1),), np.nan, dtype=torch.float64, device="cuda")
    d_q = torch.full((max(nq, 1),), -9, dtype=torch.int32, device="cuda")
    d_t = torch.full((max(nq, 1),), -9, dtype=torch.int32, device="cuda")
    d_n = torch.full((4,), -9, dtype=torch.int32, device="cuda")
    cnt = lambda c: None if c is None else _dev(np.array([c, c + 17], dtype=np.uint32).view(np.int32))
    d_ca, d_cb = cnt(countA), cnt(countB)
    dev = {k: (None if v is None else _dev(v)) for k, v in dict(kpsA=kpsA, featA=featA, kpsB=kpsB, featB=featB).items()}
    ptr = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    ctx.pair_build_dev(d_x1.data_ptr(), d_x2.data_ptr(), d_q.data_ptr(), d_t.data_ptr(), d_n.data_ptr(), None,
                       d_match=d_match.data_ptr(), nq=nq, nt=nt, cam_a=camA, cam_b=camB, d_kps_a=ptr(dev["kpsA"]), d_feat_a=ptr(dev["featA"]),
                       feat_stride_a=strideA, d_kps_b=ptr(dev["kpsB"]), d_feat_b=ptr(dev["featB"]), feat_stride_b=strideB,
                       d_count_a=ptr(d_ca), d_count_b=ptr(d_cb))
    ctx.sync()
    N = int(d_n.cpu()[0])
    return N, d_q.cpu().numpy()[:N], d_t.cpu().numpy()[:N], d_x1.cpu().numpy()[:2 * N].reshape(-1, 2), d_x2.cpu().numpy()[:2 * N].reshape(-1, 2)


def _check_pairs(got, want, what):
    N, q, t, x1, x2 = got
    wq, wt, w1, w2 = want
    assert N == len(wq), (what, N, len(wq))
    assert np.array_equal(q, wq) and np.array_equal(t, wt), what
    assert np.array_equal(_bits(x1), _bits(w1)), (what, int((_bits(x1) != _bits(w1)).sum()))
    assert np.array_equal(_bits(x2), _bits(w2)), (what, int((_bits(x2) != _bits(w2)).sum()))


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 1000, 10000])
def test_pairs_equal_the_host_rule(nq):
    """d_kps and d_feat forms mixed per camera, feat_stride 2 and 4, with and without the count words, all three distortion sets, a
    different one per camera, matches of every kind (none, all, -1 / out of range / other negatives), r2 == 0 on both sides"""
    ctx = _light_ctx()
    try:
        rng = np.random.default_rng(200 + nq)
        nt = max(1, (3 * nq) // 4 + 2)
        kpsA, kpsB = synth.random_keypoints(nq, W, H, seed=nq), synth.random_keypoints(nt, W, H, seed=nq + 1)
        kpsA["scale"][:min(nq, 64)] = np.arange(min(nq, 64)) % 8            # all 8 levels wherever there is room for them
        kpsB["scale"][:min(nt, 64)] = (3 + np.arange(min(nt, 64))) % 8
        if nq >= 64:
            assert len(np.unique(kpsA["scale"])) == 8
        featA4 = np.full((nq, 4), 7.0, dtype=np.float32)
        featA4[:, :2] = np.stack([rng.uniform(0, W, nq), rng.uniform(0, H, nq)], 1)
        featB2 = np.stack([rng.uniform(0, W, nt), rng.uniform(0, H, nt)], 1).astype(np.float32)
        featA2, featB4 = np.ascontiguousarray(featA4[:, :2]), np.full((nt, 4), 7.0, dtype=np.float32)
        featB4[:, :2] = featB2
        for da in range(3):
            camA = (1000.0, 640.0, 360.0) + track_host.DISTORTIONS[da]
            camB = (900.0, 650.0, 350.0) + track_host.DISTORTIONS[(da + 1) % 3]
            for mode in ("mixed", "none", "all"):
                match = _random_match(rng, nq, nt, mode)
                if mode != "none":
                    # a pair exactly on the two principal points
                    j, jt = nq // 2, nt // 2
                    kpsA[j] = (640, 360, 0, 0.0, 0); featA4[j, :2] = featA2[j] = (640.0, 360.0)
                    kpsB[jt] = (650, 350, 0, 0.0, 0); featB4[jt, :2] = featB2[jt] = (650.0, 350.0)
                    match[j] = jt
                sides = [("kk", dict(kpsA=kpsA, kpsB=kpsB), {}),
                         ("kf", dict(kpsA=kpsA, featB=featB2), dict(strideB=2)),
                         ("fk", dict(featA=featA4, kpsB=kpsB), dict(strideA=4)),
                         ("ff", dict(featA=featA2, featB=featB4), dict(strideA=2, strideB=4))]
                for countA, countB in ((None, None), (nq, nt), (max(nq - 1 - nq // 3, 0), max(nt - 1 - nt // 4, 0)), (nq + 5, None), (None, nt + 5)):
                    for name, side, strides in sides:
                        got = _build_on_device(ctx, match, nt, camA, camB, countA=countA, countB=countB, **side, **strides)
                        want = pair_host.build_pairs(match, nt, camA, camB, countA=countA, countB=countB, **side)
                        _check_pairs(got, want, (nq, da, mode, countA, countB, name))
                if mode == "all" and nq >= 1000:
                    got = _build_on_device(ctx, match, nt, camA, camB, kpsA=kpsA, featB=featB2, strideB=2)
                    k = np.nonzero(got[1] == nq // 2)[0]
                    assert len(k) == 1 and got[3][k[0]].tolist() == [640.0, 360.0] and got[4][k[0]].tolist() == [650.0, 350.0]    # r2 == 0
    finally:
        ctx.close()


def _distort(x, cam):
    f, pp, k = cam[0], np.array(cam[1:3]), cam[3:6]
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


def _scattered_pair(model, n, seed, camA, camB):
    """twoview_host.scene (about 30 % outliers, a plane for 'H') scattered into a d_match / two feature blocks layout: n correspondences
    among 1.6 n query rows of camera A and 1.3 n rows of camera B; -> (match, featA (nq, 4), featB (nt, 2))"""
    sc = twoview_host.scene(n, seed, planar=(model == "H"))
    rng = np.random.default_rng(seed + 1)
    nq, nt = int(1.6 * n) + 3, int(1.3 * n) + 5
    qs = np.sort(rng.choice(nq, n, replace=False))
    rows = rng.choice(nt, n, replace=False)
    match = np.full(nq, -1, dtype=np.int32)
    match[qs] = rows
    featA = np.zeros((nq, 4), dtype=np.float32)
    featA[:, :2] = np.stack([rng.uniform(0, W, nq), rng.uniform(0, H, nq)], 1)
    featA[qs, :2] = _distort(sc["x1"], camA)                     # the detector sees distorted pixels, stored as floats
    featB = np.stack([rng.uniform(0, W, nt), rng.uniform(0, H, nt)], 1).astype(np.float32)
    featB[rows] = _distort(sc["x2"], camB)
    return match, featA, featB


def _K(cam):
    return np.array([[cam[0], 0, cam[1]], [0, cam[0], cam[2]], [0, 0, 1.0]])


def _host_path(ctx, model, pairs, camA, camB, seed, wh=(W, H)):
    """today's path: the host-gathered copy of the correspondences through clc_two_view_acransac"""
    q, t, x1, x2 = pairs
    r = ctx.two_view_acransac(model, x1, x2, wh, K1=_K(camA), K2=_K(camB), seed=seed)
    r.update(pair_q=q, pair_t=t, x1=x1, x2=x2, n_pairs=len(q))
    return r


def _same_filter(got, want, what):
    assert got["n_pairs"] == want["n_pairs"], what
    assert np.array_equal(got["pair_q"], want["pair_q"]) and np.array_equal(got["pair_t"], want["pair_t"]), what
    assert np.array_equal(_bits(got["x1"]), _bits(want["x1"])) and np.array_equal(_bits(got["x2"]), _bits(want["x2"])), what
    assert np.array_equal(got["inliers"], want["inliers"]), what          # order included
    assert np.array_equal(got["mask"], want["mask"]), what
    for k in ("M", "F"):
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)
    assert got["error_max"] == want["error_max"] and got["min_nfa"] == want["min_nfa"], (what, got["error_max"], want["error_max"])
    assert got["iterations"] == want["iterations"], (what, got["iterations"], want["iterations"])


def _job(match, featA, featB, camA, camB, d_match, d_fa, d_fb, seed, **more):
    return dict(d_match=d_match.data_ptr(), nq=len(match), nt=len(featB), cam_a=camA, cam_b=camB, d_feat_a=d_fa.data_ptr(), feat_stride_a=4,
                d_feat_b=d_fb.data_ptr(), feat_stride_b=2, img_wh=(W, H), seed=seed, **more)


@pytest.mark.parametrize("n", [200, 1000, 5000])
@pytest.mark.parametrize("model", ["E", "F", "H"])
def test_filter_equals_the_host_gathered_solve(model, n):
    ctx = _light_ctx()
    try:
        camA, camB = F0 + track_host.DISTORTIONS[1], F0 + track_host.DISTORTIONS[2]
        match, featA, featB = _scattered_pair(model, n, 6000 + n, camA, camB)
        d_match, d_fa, d_fb = _dev(match), _dev(featA), _dev(featB)
        pairs = pair_host.build_pairs(match, len(featB), camA, camB, featA=featA, featB=featB)
        assert len(pairs[0]) == n
        for seed in (1, 7):
            got = ctx.pair_filter_dev(model, **_job(match, featA, featB, camA, camB, d_match, d_fa, d_fb, seed))
            want = _host_path(ctx, model, pairs, camA, camB, seed)
            assert want["M"] is not None and len(want["inliers"]) > 0.5 * n
            _same_filter(got, want, (model, n, seed))
    finally:
        ctx.close()


@pytest.mark.parametrize("n_jobs", [1, 3, 8])
def test_batch_equals_the_single_calls(n_jobs):
    """8 jobs run in lockstep, fewer interleaved for 'F' / 'H'; 'E' in lockstep from 4 (acr_lockstep)"""
    from coloc_amd import abi
    ctxs = [_light_ctx() for _ in range(n_jobs)]
    single = _light_ctx()
    try:
        camA, camB = F0 + track_host.DISTORTIONS[2], F0 + track_host.DISTORTIONS[1]
        for model in ("E", "F", "H"):
            scenes = [_scattered_pair(model, 300 + 90 * j, 700 + j, camA, camB) for j in range(n_jobs)]
            dev = [tuple(_dev(a) for a in s) for s in scenes]
            jobs = [_job(*scenes[j], camA, camB, *dev[j], 11 + j) for j in range(n_jobs)]
            for rep in range(2):                                    # (a second pair through the same contexts and pair blocks)
                got = abi.pair_filter_batch_dev(ctxs, model, jobs)
                for j in range(n_jobs):
                    one = single.pair_filter_dev(model, **jobs[j])
                    assert one["M"] is not None
                    _same_filter(got[j], one, (model, n_jobs, j, rep))
                    pairs = pair_host.build_pairs(scenes[j][0], len(scenes[j][2]), camA, camB, featA=scenes[j][1], featB=scenes[j][2])
                    _same_filter(got[j], _host_path(single, model, pairs, camA, camB, 11 + j), (model, n_jobs, j, rep, "host"))
    finally:
        for c in ctxs + [single]:
            c.close()


def test_real_front_end_without_a_host_trip():
    """two rendered views -> clc_detect_dev -> clc_describe_detected_dev (a context per camera) -> clc_match_2nn_dev at the PLANNED sizes ->
    clc_pair_filter_dev with the detectors' own count words, nothing copied in between; against today's host path on the same frames
    (download, numpy gather, two_view_acransac).  The scene is a plane: models 'E' and 'H'."""
    torch = _torch()
    from coloc_amd import Context
    w, h, cap, ppu = 640, 480, 6000, 100.0
    K = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1.0]])
    camA, camB = (520.0, 320.0, 240.0, 0.0, 0.0, 0.0), (520.0, 320.0, 240.0, -0.05, 0.01, 0.0)
    tex = synth.plane_texture()
    ca = Context(device=0, width=w, height=h, maxkp=cap, match_thresh=60)
    cb = Context(device=0, width=w, height=h, maxkp=cap, match_thresh=60)
    try:
        Ra, ta = synth.look_at_plane_pose((7.0, 7.0), 5.2)
        Rb, tb = synth.look_at_plane_pose((7.25, 6.85), 5.0, yaw=0.05, tilt=(0.03, -0.02))
        imgs = [_dev(synth.render_plane(tex, ppu, K, R, t, w, h)) for R, t in ((Ra, ta), (Rb, tb))]
        d_match = torch.full((cap,), -5, dtype=torch.int32, device="cuda")
        # camera B's descriptor rows past its count must not hold stale bits a query could match
        desc_b = torch.zeros((cap, 64), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bufs = []
        for c, img, d_desc in ((cb, imgs[1], desc_b.data_ptr()), (ca, imgs[0], None)):
            c.pyramid_build_dev(img.data_ptr(), w, h, w, None)
            c.detect_dev(None)
            c.describe_detected_dev(d_desc, None)
            bufs.append(c.detect_buffers())
        cb.sync()                                                # (camera B ran on its own context's stream; no data comes back)
        (kb, cntb, _), (ka, cnta, desc_a) = bufs
        ca.match_2nn_dev(desc_a, cap, desc_b.data_ptr(), cap, 60, d_match.data_ptr(), None)
        got = {m: ca.pair_filter_dev(m, d_match=d_match.data_ptr(), nq=cap, nt=cap, cam_a=camA, cam_b=camB, d_kps_a=ka, d_kps_b=kb,
                                     d_count_a=cnta, d_count_b=cntb, img_wh=(w, h), seed=3) for m in ("E", "H")}
        # today's path on the same frames
        ca.sync()
        kps_a, kps_b = ca.detect(capacity=cap)[0], cb.detect(capacity=cap)[0]      # the same pyramids through the host entry
        match = d_match.cpu().numpy()
        pairs = pair_host.build_pairs(match, cap, camA, camB, kpsA=kps_a, kpsB=kps_b, countA=len(kps_a),
                                      countB=len(kps_b))
        assert len(kps_a) > 800 and len(kps_b) > 800 and len(pairs[0]) > 150
        for m in ("E", "H"):
            want = _host_path(ca, m, pairs, camA, camB, 3, wh=(w, h))
            assert want["M"] is not None and len(want["inliers"]) > 60
            _same_filter(got[m], want, ("front end", m))
    finally:
        ca.close()
        cb.close()


def test_after_stream_orders_the_call_behind_the_producer():
    """d_match is written on torch's current stream behind a stretch of other work; the context's stream is non-blocking, so only the
    event the call records on after_stream puts the pair launch behind it.  No torch.cuda.synchronize() before the call."""
    torch = _torch()
    ctx = _light_ctx()
    try:
        camA, camB = F0 + track_host.DISTORTIONS[1], F0 + track_host.DISTORTIONS[0]
        match, featA, featB = _scattered_pair("E", 1000, 5100, camA, camB)
        d_src, d_fa, d_fb = _dev(match), _dev(featA), _dev(featB)
        d_match = torch.full((len(match),), -1, dtype=torch.int32, device="cuda")
        a = torch.randn(2048, 2048, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(20):
                a = (a @ a) * 1e-3
            d_match.copy_(d_src)
            got = ctx.pair_filter_dev("E", **_job(match, featA, featB, camA, camB, d_match, d_fa, d_fb, 1,
                                                   after_stream=torch.cuda.current_stream().cuda_stream))
        pairs = pair_host.build_pairs(match, len(featB), camA, camB, featA=featA, featB=featB)
        want = _host_path(ctx, "E", pairs, camA, camB, 1)
        assert want["n_pairs"] == 1000
        _same_filter(got, want, "after_stream")
        torch.cuda.synchronize()
    finally:
        ctx.close()


def test_edges():
    from coloc_amd import CLCError, abi
    ctx = _light_ctx()
    try:
        cam = F0 + (0.0, 0.0, 0.0)
        rng = np.random.default_rng(0)
        featA, featB = rng.uniform(0, 700, (50, 4)).astype(np.float32), rng.uniform(0, 700, (40, 2)).astype(np.float32)
        d_fa, d_fb = _dev(featA), _dev(featB)
        base = dict(nq=50, nt=40, cam_a=cam, cam_b=cam, d_feat_a=d_fa.data_ptr(), d_feat_b=d_fb.data_ptr(), feat_stride_b=2, img_wh=(W, H))
        none = _dev(np.full(50, -1, dtype=np.int32))
        for model in "EFH":
            r = ctx.pair_filter_dev(model, d_match=none.data_ptr(), **base)                 # 0 matches
            assert r["n_pairs"] == 0 and len(r["inliers"]) == 0 and r["M"] is None and r["status"] == abi.CLC_OK
            r = ctx.pair_filter_dev(model, d_match=none.data_ptr(), **dict(base, nq=0))     # no queries at all
            assert r["n_pairs"] == 0 and r["M"] is None and r["status"] == abi.CLC_OK
            m = np.full(50, -1, dtype=np.int32)
            rows = np.sort(rng.choice(50, SAMPLE[model], replace=False))
            m[rows] = np.arange(SAMPLE[model])
            d_m = _dev(m)
            r = ctx.pair_filter_dev(model, d_match=d_m.data_ptr(), **base)                  # N == sample size: OK, no model
            assert r["n_pairs"] == SAMPLE[model] and len(r["inliers"]) == 0 and r["M"] is None and r["status"] == abi.CLC_OK
            assert r["pair_q"].tolist() == rows.tolist() and r["pair_t"].tolist() == list(range(SAMPLE[model]))
            assert np.array_equal(_bits(r["x1"]), _bits(pair_host.build_pairs(m, 40, cam, cam, featA=featA, featB=featB)[2]))
        d_m = _dev(np.arange(50, dtype=np.int32) % 40)
        job = dict(base, d_match=d_m.data_ptr())
        bad = [dict(job, d_feat_a=None), dict(job, d_kps_a=d_fa.data_ptr()), dict(job, d_feat_b=None), dict(job, d_kps_b=d_fb.data_ptr()),   # neither / both
               dict(job, d_match=d_m.data_ptr() + 2), dict(job, d_feat_b=d_fb.data_ptr() + 1), dict(job, d_count_a=d_fa.data_ptr() + 2),       # misaligned
               dict(job, cam_a=(0.0,) + cam[1:]), dict(job, cam_b=(-3.0,) + cam[1:]), dict(job, nt=-1)]
        for b in bad:
            with pytest.raises(CLCError) as e:
                ctx.pair_filter_dev("E", **b)
            assert e.value.status == abi.CLC_ERR_BAD_ARG
        with pytest.raises(CLCError) as e:                                                   # an unknown model
            ctx.pair_filter_dev("X", **job)
        assert e.value.status == abi.CLC_ERR_BAD_ARG
        # more correspondences than a solve takes: refused, nothing written past the block
        nbig = 17000
        big_a, big_b = _dev(rng.uniform(0, 700, (nbig, 2)).astype(np.float32)), _dev(rng.uniform(0, 700, (nbig, 2)).astype(np.float32))
        d_big = _dev(np.arange(nbig, dtype=np.int32))
        with pytest.raises(CLCError) as e:
            ctx.pair_filter_dev("F", d_match=d_big.data_ptr(), nq=nbig, nt=nbig, cam_a=cam, cam_b=cam, d_feat_a=big_a.data_ptr(), feat_stride_a=2,
                                d_feat_b=big_b.data_ptr(), feat_stride_b=2, img_wh=(W, H))
        assert e.value.status == abi.CLC_ERR_CAPACITY
        # the context is usable afterwards
        camA, camB = F0 + track_host.DISTORTIONS[1], F0 + track_host.DISTORTIONS[2]
        match, fa, fb = _scattered_pair("F", 300, 77, camA, camB)
        dm, dfa, dfb = _dev(match), _dev(fa), _dev(fb)
        got = ctx.pair_filter_dev("F", **_job(match, fa, fb, camA, camB, dm, dfa, dfb, 2))
        _same_filter(got, _host_path(ctx, "F", pair_host.build_pairs(match, len(fb), camA, camB, featA=fa, featB=fb), camA, camB, 2), "after the edges")
    finally:
        ctx.close()

"""A tracked frame's pose from the prediction (include/coloc_hip.h: clc_track_prior_dev, clc_track_prior_batch_dev,
clc_pnp_refine_prior; THE RULE there).

  the host-array entry on the case table (tests/pose_prior_cases.py) against the 50-digit reference (tests/pose_prior_mp.py): mask,
  rounds_run, converged, result, n_inliers equal; the pose by rule b, cov and rmse by rules c and d of tests/test_gpu_pose_edges.py as they
  stand; two calls equal bits; N = 3 and "every point behind the prior" give FEW with the prior's bits and a zero covariance
  the device path equals the host-array entry BIT FOR BIT on the host-gathered copy of the same tracks (track_host.build_tracks)
  batch, after_stream, the rendered chain, a wrong prior, errors and edges
With -s the tests print what they measured.
"""
import functools

import numpy as np
import pytest
from mpmath import mp

import pose_mp as pm
import pose_prior_cases as pc
import pose_prior_host as ph
import synth
import track_host
from test_pose_prior_reference import rule_b
from test_gpu_pose_edges import _np_normal_matrix
from test_gpu_track_localize import _bits, _dev, _distort, _light_ctx, _torch

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
W, H = 1280, 720
CAM0 = (1000.0, 640.0, 360.0)
OK, FEW = 0, 1


def _K(cam):
    return np.array([[cam[0], 0, cam[1]], [0, cam[0], cam[2]], [0, 0, 1.0]])


def _params(Rt):
    return pm.log_so3(Rt[:, :3]) + pm.vec(Rt[:, 3])


def _same_bits(a, b, what):
    for k in ("Rt", "cov", "mask"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)
    for k in ("n_inliers", "iterations", "rounds_run", "converged", "result"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert _bits(np.array([a["rmse"]]))[0] == _bits(np.array([b["rmse"]]))[0], (what, "rmse")


def _mask_consistent(r, X, x, K, gate, what):
    """every track outside the 5 % band around the gate (and not next to the principal plane), recomputed in numpy at the returned pose, is
    classified as the mask says"""
    Xc = X @ r["Rt"][:, :3].T + r["Rt"][:, 3]
    uvw = Xc @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        sq = ((x - uvw[:, :2] / uvw[:, 2:3]) ** 2).sum(1)
    g2 = gate * gate
    clear = (np.abs(Xc[:, 2]) >= 1e-6) & ~((sq >= 0.95 * g2) & (sq <= 1.05 * g2))
    want = (Xc[:, 2] > 0) & (sq <= g2)
    assert np.array_equal(r["mask"][clear], want[clear]), (what, np.flatnonzero(clear & (r["mask"] != want)))
    assert r["n_inliers"] == int(r["mask"].sum()), what
    return int(clear.sum())


# ---- the host-array entry on the case table --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", pc.IDS)
def test_case_table_against_the_reference(gpu_ctx, cid):
    c = pc.build(cid)
    ref = pc.reference(cid)
    X, x, K = c["X"], c["x"], c["K"]
    got = gpu_ctx.pnp_refine_prior(X, x, K, c["Rt_prior"], pc.GATE, huber_a=pc.HUBER)
    again = gpu_ctx.pnp_refine_prior(X, x, K, c["Rt_prior"], pc.GATE, huber_a=pc.HUBER)
    _same_bits(got, again, cid)
    rec = ["%s: rounds %d, converged %d, result %d, inliers %d, iterations %d" % (cid, got["rounds_run"], got["converged"], got["result"],
                                                                                 got["n_inliers"], got["iterations"])]
    assert np.isfinite(got["Rt"]).all() and np.isfinite(got["cov"]).all() and np.isfinite(got["rmse"]), rec
    assert np.array_equal(got["mask"], ref["mask"]), (rec, np.flatnonzero(got["mask"] != ref["mask"]))
    assert (got["rounds_run"], got["converged"], got["result"], got["n_inliers"]) == \
        (ref["rounds_run"], ref["converged"], ref["result"], ref["n_inliers"]), rec
    assert 0 <= got["iterations"] <= 50 * max(got["rounds_run"], 1), rec
    if ref["rounds_run"] == 0:
        assert got["result"] == FEW and np.array_equal(_bits(got["Rt"]), _bits(c["Rt_prior"])) and not got["cov"].any(), rec
        print("\n" + " | ".join(rec))
        return
    p = _params(got["Rt"])
    a = pc.HUBER
    mask_b = ref["mask"] if ref["converged"] else ref["masks"][-2]
    A, cost = rule_b(p, X, x, K, a, mask_b, rec)
    if not np.array_equal(mask_b, ref["mask"]):
        A, _, cost = pm.normal_equations(p, X, x, K, a, mask=ref["mask"])
    n_in = ref["n_inliers"]
    if got["result"] == OK:
        # c: the covariance at the returned pose over the returned mask (angles far from pi here: one chart)
        Ainv, Af = pm.to_float(mp.inverse(A)), pm.to_float(A)
        Dh = 1.0 / np.sqrt(np.diag(Af))
        cond = float(np.linalg.cond(Af * Dh[:, None] * Dh[None, :]))
        bound = 256.0 * cond * EPS * np.abs(Ainv).max()
        m = ref["mask"]
        err_np = np.abs(np.linalg.inv(_np_normal_matrix(pm.to_float(p), X[m], x[m], K, a)) - Ainv).max()
        err_gpu = np.abs(got["cov"] - Ainv).max()
        rec.append("c: |cov - A^-1| %.2e (numpy %.2e) <= %.2e, cond %.2e" % (err_gpu, err_np, bound, cond))
        assert err_np <= bound / 4, rec
        assert err_gpu <= bound, rec
        assert np.abs(got["cov"] - got["cov"].T).max() <= 2 * bound, rec
    else:
        assert not got["cov"].any(), rec
    if n_in > 0:
        # d: rmse
        rmse_ref = float(mp.sqrt(cost / (2 * n_in)))
        rec.append("d: rmse %.12g vs %.12g" % (got["rmse"], rmse_ref))
        assert abs(got["rmse"] - rmse_ref) <= 1e-9 * rmse_ref + 64 * EPS * np.abs(x).max(), rec
    print("\n" + " | ".join(rec))


# ---- the two entries of the one Levenberg-Marquardt pass (csrc/pose_lm.h) --------------------------------------------------------------

AGREE_NS = (4, 513, 600)        # the least the prior runs on; the first size at which a thread owns two tracks; an active Huber tail
AGREE_GATE, AGREE_HUBER = 1e4, 16.0


@functools.lru_cache(maxsize=None)
def _agree_scene(n):
    """synth.pnp_scene without outliers (points 4 - 20 units in front, 0.5 px noise), the start its pose turned by a degree and shifted
    by two centimetres; at N = 600 seven observations are moved 40 .. 70 px away, past huber_a -> X, x, K, start"""
    s = synth.pnp_scene(n, seed=4300 + n, outlier_frac=0.0)
    x = s["x"].copy()
    if n == 600:
        rng = np.random.default_rng(n)
        ang = rng.uniform(0, 2 * np.pi, 7)
        x[rng.choice(n, 7, replace=False)] += rng.uniform(40, 70, (7, 1)) * np.stack([np.cos(ang), np.sin(ang)], 1)
    start = np.concatenate([pc._rot(np.radians(1.0), pc._axis(n + 1)) @ s["R"], (s["t"] + 0.02 * pc._axis(n + 2))[:, None]], 1)
    return s["X"], x, s["K"], start


@pytest.mark.parametrize("n", AGREE_NS)
def test_prior_with_every_track_in_equals_the_refine(gpu_ctx, n):
    """Where their rules coincide, clc_pnp_refine_prior performs the Levenberg-Marquardt clc_pnp_refine performs without a mask, on the
    same X, x, K, start, huber_a and max_iter.  The conditions: every point in front of the camera at the start (the first mask is all
    of them), a gate no residual reaches at any pose the minimisation visits (every track is "in", so the mask is stable after round 1:
    converged, no FINAL pass), rounds = 1, N >= 4 and min_inliers <= N.  Then iterations and n_inliers == N are equal, and Rt, cov and
    rmse agree within the bounds each entry is held to against the 50-digit reference (rules b, c, d of tests/test_gpu_pose_edges.py and
    tests/test_pose_prior_reference.py, the same for both entries; A for rule c in float64 numpy, which its bound allows a quarter).
    The seeds give equal iterations on the library before the pass was stated once as well (profiles/pose_lm_once.txt)."""
    X, x, K, start = _agree_scene(n)
    assert ((X @ start[:, :3].T + start[:, 3])[:, 2] > 0).all()
    Rt, cov, rmse, it = gpu_ctx.pnp_refine(X, x, K, start, huber_a=AGREE_HUBER, max_iter=50)
    got = gpu_ctx.pnp_refine_prior(X, x, K, start, AGREE_GATE, huber_a=AGREE_HUBER, rounds=1, max_iter=50, min_inliers=4)
    uvw = (X @ Rt[:, :3].T + Rt[:, 3]) @ K.T
    sq = ((x - uvw[:, :2] / uvw[:, 2:3]) ** 2).sum(1)
    assert sq.max() < AGREE_GATE ** 2 and int((sq > AGREE_HUBER ** 2).sum()) == (7 if n == 600 else 0)
    p, q = pm.to_float(_params(Rt)), pm.to_float(_params(got["Rt"]))
    A = _np_normal_matrix(p, X, x, K, AGREE_HUBER)
    Ainv = np.linalg.inv(A)
    Dh = 1.0 / np.sqrt(np.diag(A))
    bound = 256.0 * float(np.linalg.cond(A * Dh[:, None] * Dh[None, :])) * EPS * np.abs(Ainv).max()
    rec = "N %d: iterations %d / %d, inliers %d, rounds %d, converged %d, result %d; |p - q| %.2e <= 1e-5; |cov - cov'| %.2e <= %.2e; rmse %.12g / %.12g" % (
        n, it, got["iterations"], got["n_inliers"], got["rounds_run"], got["converged"], got["result"], np.abs(p - q).max(),
        np.abs(cov - got["cov"]).max(), bound, rmse, got["rmse"])
    print("\n" + rec)
    assert it > 0 and got["iterations"] == it, rec
    assert got["n_inliers"] == n and got["mask"].all() and (got["rounds_run"], got["converged"], got["result"]) == (1, 1, OK), rec
    assert np.abs(p - q).max() <= 1e-5, rec
    assert np.abs(cov - got["cov"]).max() <= bound, rec
    assert abs(rmse - got["rmse"]) <= 1e-9 * rmse + 64 * EPS * np.abs(x).max(), rec


# ---- the device path ---------------------------------------------------------------------------------------------------------------------

def _frame(nq, seed, cam, map_n=None, share_matched=0.7, share_out=0.15, noise=0.8):
    """a frame of nq features of which a share is matched to landmarks seen under a true pose; a share of those matches is wrong.
    -> dict(match, feat (nq, 4) float32, kps, map_X, Rt_true)"""
    rng = np.random.default_rng(seed)
    map_n = map_n or (2 * nq + 40)
    R = pc._rot(0.4, pc._axis(seed))
    t = np.array([0.3, -0.2, 0.5])
    z = rng.uniform(4, 20, map_n)
    Xc = np.stack([rng.uniform(-0.5, 0.5, map_n) * z, rng.uniform(-0.3, 0.3, map_n) * z, z], 1)
    map_X = (Xc - t) @ R
    match = np.full(nq, -1, dtype=np.int32)
    n = max(int(round(share_matched * nq)), 1)
    qs = np.sort(rng.choice(nq, n, replace=False))
    rows = rng.choice(map_n, n, replace=False)
    match[qs] = rows
    uvw = Xc[rows] @ _K(cam).T
    px = uvw[:, :2] / uvw[:, 2:3] + rng.uniform(-noise, noise, (n, 2))
    wrong = rng.random(n) < share_out
    px[wrong] += rng.uniform(15, 90, (int(wrong.sum()), 2)) * rng.choice([-1.0, 1.0], (int(wrong.sum()), 2))
    feat = np.zeros((nq, 4), dtype=np.float32)
    feat[:, :2] = np.stack([rng.uniform(0, W, nq), rng.uniform(0, H, nq)], 1)
    feat[qs, :2] = _distort(px, cam)
    feat[:, 2:] = 3.0
    kps = np.zeros(nq, dtype=synth.KP_DTYPE)
    kps["x"], kps["y"] = np.rint(feat[:, 0]).astype(np.int32), np.rint(feat[:, 1]).astype(np.int32)      # level 0: the pixel itself
    return dict(match=match, feat=feat, kps=kps, map_X=map_X, Rt_true=np.concatenate([R, t[:, None]], 1))


def _host_entry(ctx, fr, cam, prior, gate, kps=False, stride=4, count=None, **step):
    feat = None if kps else (fr["feat"] if stride == 4 else np.ascontiguousarray(fr["feat"][:, :2]))
    q, m, X, x = track_host.build_tracks(fr["match"], fr["map_X"], cam, kps=fr["kps"] if kps else None, feat=feat, count=count)
    r = ctx.pnp_refine_prior(X, x, _K(cam), prior, gate, **step)
    r.update(track_query=q, track_map=m, n_tracks=len(q), X=X, x=x)
    return r


def _same_as_host(got, want, what):
    assert got["n_tracks"] == want["n_tracks"], (what, got["n_tracks"], want["n_tracks"])
    assert np.array_equal(got["track_query"], want["track_query"]) and np.array_equal(got["track_map"], want["track_map"]), what
    assert got["status"] == 0, what
    _same_bits(got, want, what)


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 1000])
def test_device_path_equals_the_host_array_entry(nq):
    ctx = _light_ctx()
    try:
        gate = 3.0
        seen = set()
        for k, dist in enumerate(track_host.DISTORTIONS):
            cam = CAM0 + dist
            fr = _frame(nq, 300 + 7 * nq + k, cam)
            ctx.set_map_points(fr["map_X"])
            prior = pc.perturbed(fr["Rt_true"], nq + k)
            d_match, d_feat, d_kps = _dev(fr["match"]), _dev(fr["feat"]), _dev(fr["kps"])
            d_feat2 = _dev(np.ascontiguousarray(fr["feat"][:, :2]))
            below = max(nq - 1 - nq // 3, 0)
            d_cnt = _dev(np.array([below, below + 17], dtype=np.uint32).view(np.int32))
            base = dict(d_match=d_match.data_ptr(), nq=nq, cam=cam, Rt_prior=prior, gate=gate)
            variants = [("kps", dict(d_kps=d_kps.data_ptr()), dict(kps=True)),
                        ("feat4", dict(d_feat=d_feat.data_ptr(), feat_stride=4), dict()),
                        ("feat2", dict(d_feat=d_feat2.data_ptr(), feat_stride=2), dict(stride=2)),
                        ("count", dict(d_feat=d_feat.data_ptr(), d_count=d_cnt.data_ptr()), dict(count=below))]
            for name, dev_kw, host_kw in variants:
                got = ctx.track_prior_dev(**base, **dev_kw)
                want = _host_entry(ctx, fr, cam, prior, gate, **host_kw)
                _same_as_host(got, want, (nq, dist, name))
                seen.add(got["result"])
                if got["result"] == OK:
                    _mask_consistent(got, want["X"], want["x"], _K(cam), gate, (nq, dist, name))
                    assert np.abs(got["Rt"] - fr["Rt_true"]).max() < 0.05, (nq, dist, name)
            # other step arguments travel too
            got = ctx.track_prior_dev(**base, d_feat=d_feat.data_ptr(), huber_a=2.0, rounds=2, max_iter=3, min_inliers=5)
            _same_as_host(got, _host_entry(ctx, fr, cam, prior, gate, huber_a=2.0, rounds=2, max_iter=3, min_inliers=5), (nq, dist, "step"))
            assert got["rounds_run"] <= 2 and got["iterations"] <= 6
        assert (OK in seen) == (nq >= 63), (nq, seen)
    finally:
        ctx.close()


def test_batch_equals_the_single_calls():
    from coloc_amd import abi
    ctxs = [_light_ctx() for _ in range(3)]
    single = _light_ctx()
    try:
        assert abi.track_prior_batch_dev([], []) == []
        cam = CAM0 + track_host.DISTORTIONS[2]
        map_n = 2500
        frames = [_frame(nq, 800 + j, cam, map_n=map_n) for j, nq in enumerate((700, 130, 1000))]
        # one shared map: every frame's landmarks are its own scene's, so the frames get a third of the rows each
        map_X = frames[0]["map_X"].copy()
        Rt_true = frames[0]["Rt_true"]
        for fr in frames[1:]:
            fr["map_X"] = map_X
            rows = fr["match"][fr["match"] >= 0]
            fr["match"][fr["match"] >= 0] = np.random.default_rng(9).permutation(map_n)[:len(rows)]
        # frames 1 and 2 now carry matches that fit no pose: frame 1 keeps its 130 features as a FEW job, frame 2 is re-made on the shared map
        uvw = (map_X @ Rt_true[:, :3].T + Rt_true[:, 3]) @ _K(cam).T
        px = uvw[:, :2] / uvw[:, 2:3]
        f2 = frames[2]
        acc = np.flatnonzero(f2["match"] >= 0)
        f2["feat"][acc, :2] = _distort(px[f2["match"][acc]] + np.random.default_rng(10).uniform(-0.8, 0.8, (len(acc), 2)), cam)
        for c in ctxs + [single]:
            c.set_map_points(map_X)
        dev = [(_dev(fr["match"]), _dev(fr["feat"])) for fr in frames]
        priors = [pc.perturbed(Rt_true, 40 + j) for j in range(3)]
        jobs = [dict(d_match=dm.data_ptr(), nq=len(frames[j]["match"]), cam=cam, d_feat=df.data_ptr(), Rt_prior=priors[j], gate=3.0 + j)
                for j, (dm, df) in enumerate(dev)]
        for n_jobs in (1, 3):
            for rep in range(2):
                got = abi.track_prior_batch_dev(ctxs[:n_jobs], jobs[:n_jobs])
                for j in range(n_jobs):
                    one = single.track_prior_dev(**jobs[j])
                    _same_as_host(got[j], one, (n_jobs, j, rep))
                    _same_as_host(got[j], _host_entry(single, frames[j], cam, priors[j], 3.0 + j), (n_jobs, j, rep, "host"))
        assert [g["result"] for g in got] == [OK, FEW, OK], [(g["result"], g["n_inliers"], g["n_tracks"]) for g in got]
    finally:
        for c in ctxs + [single]:
            c.close()


def test_after_stream_orders_the_call_behind_the_producer():
    """d_match is written on torch's current stream behind a stretch of other work; only the event the call records on after_stream puts the
    track launch behind it.  No torch.cuda.synchronize() before the call."""
    torch = _torch()
    ctx = _light_ctx()
    try:
        cam = CAM0 + track_host.DISTORTIONS[1]
        fr = _frame(1000, 5000, cam)
        ctx.set_map_points(fr["map_X"])
        prior = pc.perturbed(fr["Rt_true"], 5)
        d_src, d_feat = _dev(fr["match"]), _dev(fr["feat"])
        d_match = torch.full((1000,), -1, dtype=torch.int32, device="cuda")
        a = torch.randn(2048, 2048, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(20):
                a = (a @ a) * 1e-3
            d_match.copy_(d_src)
            got = ctx.track_prior_dev(d_match=d_match.data_ptr(), nq=1000, cam=cam, d_feat=d_feat.data_ptr(), Rt_prior=prior, gate=3.0,
                                      after_stream=torch.cuda.current_stream().cuda_stream)
        want = _host_entry(ctx, fr, cam, prior, 3.0)
        assert want["n_tracks"] == 700 and want["result"] == OK
        _same_as_host(got, want, "after_stream")
        torch.cuda.synchronize()
    finally:
        ctx.close()


def test_chain_on_rendered_frames():
    """a map from two rendered views, a third view through the plain match -> clc_track_localize_dev -> the guided re-match under its
    pose; then clc_track_prior_dev on the guided d_match with the first solve's pose as the prior and its error_max as the gate.  What the
    scene yields is printed beside the a-contrario solve's, not fixed in advance."""
    torch = _torch()
    from coloc_amd import Context, abi
    w, h, cap, ppu = 640, 480, 2048, 100.0
    K = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1.0]])
    cams = [(520.0, 320.0, 240.0, 0.0, 0.0, 0.0), (520.0, 320.0, 240.0, -0.05, 0.01, 0.0), (520.0, 320.0, 240.0, 0.0, 0.0, 0.0)]
    tex = synth.plane_texture()
    ctxs = [Context(device=0, width=w, height=h, maxkp=cap, match_thresh=60, fast_thresh=60) for _ in range(3)]
    try:
        poses = [synth.look_at_plane_pose((7.0, 7.0), 5.2), synth.look_at_plane_pose((7.25, 6.85), 5.0, yaw=0.05, tilt=(0.03, -0.02)),
                 synth.look_at_plane_pose((7.1, 6.95), 5.1, yaw=0.02, tilt=(0.01, -0.01))]
        imgs = [_dev(synth.render_plane(tex, ppu, K, R, t, w, h)) for R, t in poses]
        desc = [torch.zeros((cap, 64), dtype=torch.uint8, device="cuda") for _ in range(3)]
        d_pair, d_plain, d_guided = (torch.full((cap,), -5, dtype=torch.int32, device="cuda") for _ in range(3))
        torch.cuda.synchronize()
        bufs = []
        for c, img, d in zip(ctxs, imgs, desc):
            c.pyramid_build_dev(img.data_ptr(), w, h, w, None)
            c.detect_dev(None)
            c.describe_detected_dev(d.data_ptr(), None)
            c.sync()
            bufs.append(c.detect_buffers())
        (ka, cnta, _), (kb, cntb, _), (kc, cntc, _) = bufs
        ctx = ctxs[0]
        ctx.match_2nn_dev(desc[0].data_ptr(), cap, desc[1].data_ptr(), cap, 60, d_pair.data_ptr(), None)
        ctx.sync()
        pair = dict(d_match=d_pair.data_ptr(), nq=cap, nt=cap, cam_a=cams[0], cam_b=cams[1], d_kps_a=ka, d_kps_b=kb, d_count_a=cnta, d_count_b=cntb,
                    img_wh=(w, h), seed=3)
        dc = [dict(cam=cams[i], d_kps=k, d_desc=desc[i].data_ptr()) for i, k in enumerate((ka, kb))]
        got, filt = abi.map_init_batch_dev([ctx], [pair], [cap, cap], [(0, 1)], dc)
        assert got["entered"] == [True] and got["map_n"] > 100
        frame = dict(nq=cap, cam=cams[2], d_kps=kc, d_count=cntc)
        ctx.match_map_dev(desc[2].data_ptr(), cap, 60, d_plain.data_ptr(), None)
        first = ctx.track_localize_dev(d_match=d_plain.data_ptr(), seed=7, **frame)
        assert first["Rt"] is not None and len(first["inliers"]) > 30
        P, gate = first["Rt"], float(first["error_max"])                   # the precision AC-RANSAC found, in pixels
        ctx.match_map_guided_dev(d_q=desc[2].data_ptr(), Rt=P, radius=4.0, threshold=60, d_match=d_guided.data_ptr(), **frame)
        second = ctx.track_localize_dev(d_match=d_guided.data_ptr(), seed=7, **frame)
        prior = ctx.track_prior_dev(d_match=d_guided.data_ptr(), Rt_prior=P, gate=gate, **frame)
        ctx.sync()
        kps_c = ctxs[2].detect(capacity=cap)[0]
        nc = len(kps_c)
        padded = np.concatenate([kps_c, np.zeros(cap - nc, dtype=kps_c.dtype)])
        tq, tm, X, x = track_host.build_tracks(d_guided.cpu().numpy(), got["X"], cams[2], kps=padded, count=nc)
        stmt = ph.solve(X, x, K, P, gate)
        print("\nchain: guided match gives %d tracks; a-contrario solve on them: %d inliers (error_max %.3f px, rmse %.3f after refinement); "
              "from the prediction (gate %.3f px): result %d, %d inliers, %d rounds, %d iterations, converged %d, rmse %.3f; the float64 "
              "statement's masks round by round %s" % (second["n_tracks"], len(second["inliers"]), second["error_max"], second["rmse"], gate,
                                                        prior["result"], prior["n_inliers"], prior["rounds_run"], prior["iterations"],
                                                        prior["converged"], prior["rmse"], [int(m.sum()) for m in stmt["masks"]]))
        assert prior["result"] == OK and prior["status"] == 0
        assert prior["n_tracks"] == len(tq) and np.array_equal(prior["track_query"], tq) and np.array_equal(prior["track_map"], tm)
        clear = _mask_consistent(prior, X, x, K, gate, "chain")
        rec = []
        rule_b(_params(prior["Rt"]), X, x, K, 16.0, prior["mask"], rec)
        print("chain: %d tracks outside the band; %s" % (clear, rec[0]))
    finally:
        for c in ctxs:
            c.close()


def test_a_wrong_prior_is_few_or_consistent():
    ctx = _light_ctx()
    try:
        cam = CAM0 + track_host.DISTORTIONS[1]
        fr = _frame(1000, 6100, cam)
        ctx.set_map_points(fr["map_X"])
        c, s = np.cos(0.35), np.sin(0.35)
        prior = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ fr["Rt_true"]           # the camera turned 0.35 rad about its optical axis
        d_match, d_feat = _dev(fr["match"]), _dev(fr["feat"])
        got = ctx.track_prior_dev(d_match=d_match.data_ptr(), nq=1000, cam=cam, d_feat=d_feat.data_ptr(), Rt_prior=prior, gate=3.0)
        assert got["status"] == 0 and got["result"] in (OK, FEW)
        assert np.isfinite(got["Rt"]).all() and np.isfinite(got["cov"]).all() and np.isfinite(got["rmse"])
        q, m, X, x = track_host.build_tracks(fr["match"], fr["map_X"], cam, feat=fr["feat"])
        _mask_consistent(got, X, x, _K(cam), 3.0, "wrong prior")
        print("\nwrong prior (0.35 rad about the optical axis): result %d, %d of %d tracks in, %d rounds, %d iterations, converged %d"
              % (got["result"], got["n_inliers"], got["n_tracks"], got["rounds_run"], got["iterations"], got["converged"]))
        if got["result"] == OK:
            # the pose minimises over the last mask a round ran on: the final mask where it is stable, else the one before it, which the
            # float64 statement names
            rec = []
            mask_b = got["mask"] if got["converged"] else ph.solve(X, x, _K(cam), prior, 3.0)["masks"][-2]
            rule_b(_params(got["Rt"]), X, x, _K(cam), 16.0, mask_b, rec)
        else:
            assert not got["cov"].any()
    finally:
        ctx.close()


def test_errors_and_edges():
    from coloc_amd import CLCError, abi
    ctx = _light_ctx()
    try:
        cam = CAM0 + (0.0, 0.0, 0.0)
        fr = _frame(300, 77, cam)
        prior = pc.perturbed(fr["Rt_true"], 3)
        d_match, d_feat = _dev(fr["match"]), _dev(fr["feat"])
        job = dict(d_match=d_match.data_ptr(), nq=300, cam=cam, d_feat=d_feat.data_ptr(), Rt_prior=prior, gate=3.0)

        def refused(status, **kw):
            with pytest.raises(CLCError) as e:
                ctx.track_prior_dev(**dict(job, **kw))
            assert e.value.status == status, (kw, e.value.status)

        refused(abi.CLC_ERR_STATE)                              # no map points yet
        ctx.set_map_points(fr["map_X"])
        good = ctx.track_prior_dev(**job)
        assert good["result"] == OK
        bad_prior = prior.copy(); bad_prior[1, 2] = np.nan
        inf_prior = prior.copy(); inf_prior[0, 3] = np.inf
        for kw in (dict(Rt_prior=bad_prior), dict(Rt_prior=inf_prior), dict(gate=0.0), dict(gate=-1.0), dict(gate=np.nan), dict(gate=np.inf),
                   dict(gate=1e200), dict(gate=1e-200), dict(rounds=-1), dict(rounds=9), dict(max_iter=-1), dict(d_feat=None),
                   dict(d_kps=d_feat.data_ptr()), dict(cam=(0.0,) + cam[1:]), dict(cam=(-5.0,) + cam[1:])):
            refused(abi.CLC_ERR_BAD_ARG, **kw)
        lib = abi.load_library()
        assert lib.clc_track_prior_dev(None, None) == abi.CLC_ERR_BAD_ARG and lib.clc_track_prior_dev(ctx.h, None) == abi.CLC_ERR_BAD_ARG
        assert lib.clc_track_prior_batch_dev(None, None, -1) == abi.CLC_ERR_BAD_ARG
        assert lib.clc_track_prior_batch_dev(None, None, 9) == abi.CLC_ERR_BAD_ARG
        assert lib.clc_track_prior_batch_dev(None, None, 1) == abi.CLC_ERR_BAD_ARG
        # the host-array entry's own checks
        q, m, X, x = track_host.build_tracks(fr["match"], fr["map_X"], cam, feat=fr["feat"])
        for kw in (dict(gate=0.0), dict(rounds=9), dict(max_iter=-2)):
            with pytest.raises(CLCError) as e:
                ctx.pnp_refine_prior(X, x, _K(cam), prior, **dict(dict(gate=3.0), **kw))
            assert e.value.status == abi.CLC_ERR_BAD_ARG
        with pytest.raises(CLCError) as e:
            ctx.pnp_refine_prior(X, x, 2.0 * _K(cam), prior, 3.0)
        assert e.value.status == abi.CLC_ERR_BAD_ARG
        with pytest.raises(CLCError) as e:
            ctx.pnp_refine_prior(np.zeros((16385, 3)), np.zeros((16385, 2)), _K(cam), prior, 3.0)
        assert e.value.status == abi.CLC_ERR_CAPACITY
        # nq == 0, and no accepted query: CLC_OK, FEW, the prior's bits
        none = _dev(np.full(300, -1, dtype=np.int32))
        for r in (ctx.track_prior_dev(**dict(job, nq=0)), ctx.track_prior_dev(**dict(job, d_match=none.data_ptr())),
                  ctx.pnp_refine_prior(np.zeros((0, 3)), np.zeros((0, 2)), _K(cam), prior, 3.0)):
            assert r["result"] == FEW and r["n_inliers"] == 0 and r.get("n_tracks", 0) == 0 and r["rounds_run"] == 0
            assert np.array_equal(_bits(r["Rt"]), _bits(prior)) and not r["cov"].any()
        # more tracks than a solve takes: CLC_ERR_CAPACITY after the wait
        many = _dev(np.zeros(16390, dtype=np.int32))
        many_feat = _dev(np.tile(fr["feat"][:1], (16390, 1)))
        refused(abi.CLC_ERR_CAPACITY, d_match=many.data_ptr(), nq=16390, d_feat=many_feat.data_ptr())
        ctx.set_map_points(np.zeros((0, 3)))                    # cleared
        refused(abi.CLC_ERR_STATE)
        # the context still serves both solves
        ctx.set_map_points(fr["map_X"])
        after = ctx.track_prior_dev(**job)
        _same_bits(after, good, "after the errors")
        loc = ctx.track_localize_dev(d_match=d_match.data_ptr(), nq=300, cam=cam, d_feat=d_feat.data_ptr(), seed=2)
        assert loc["Rt"] is not None and np.abs(loc["Rt"] - fr["Rt_true"]).max() < 0.05 and loc["n_tracks"] == good["n_tracks"]
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
            ctx.track_prior_dev(d_match=d_match.data_ptr(), nq=8, cam=CAM0 + (0.0, 0.0, 0.0), d_feat=d_feat.data_ptr(), Rt_prior=np.eye(4)[:3], gate=3.0)
        assert e.value.status == abi.CLC_ERR_STATE
    finally:
        ctx.close()

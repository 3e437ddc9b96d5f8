"""The map match guided by a predicted pose on the device (include/coloc_hip.h: clc_match_map_guided_dev, clc_match_map_guided_batch_dev)
against the host statement (tests/proj_host.py).  Every comparison is EXACT: d_match, d_best, d_second, d_qpos and d_proj equal the
statement bit for bit.

One sweep workgroup holds 128 queries and its 8 waves cut a split, so the shapes straddle 128 queries, and the map runs from fewer rows
than waves (1, 2, 7) through one split (33) to several splits (513, 1500); what the plan really does is asserted, not assumed.  The
classes (queries with 0, 1 and >= 2 candidates, queries whose unrestricted best row lies outside the radius, ties for the minimum inside
it, exact copies on landmarks without a projection) are asserted on the statement before the device is looked at, wherever the shape
leaves room for all of them (nq >= 127 and nm >= 33)."""
import os
import subprocess

import numpy as np
import pytest

import guided_host as gh
import proj_host as ph
import synth
import track_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM_K = (520.0, 320.0, 240.0, -0.05, 0.01, 0.002)


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1) if a.dtype.names else a).cuda()
    torch.cuda.synchronize()
    return t


def _ctx(monkeypatch, formulation="popcount", maxkp=2048, M=None, X=None):
    from coloc_amd import Context
    monkeypatch.setenv("CLC_K2NN_FORMULATION", formulation)
    ctx = Context(device=0, detector=False, maxkp=maxkp)
    if M is not None:
        ctx.set_map(M)
        ctx.set_map_points(X)
    return ctx


def _pose(ax=0.0, ay=0.0, az=0.0, C=(0.0, 0.0, 0.0)):
    """[R|t], t = -R C with each row ((R0 C0 + R1 C1) + R2 C2) negated: the order Pose3::translation() and the policy member use"""
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    t = np.array([-((R[i, 0] * C[0] + R[i, 1] * C[1]) + R[i, 2] * C[2]) for i in range(3)])
    return np.column_stack([R, t])


class _Job:
    """one job's device buffers (inputs uploaded, outputs poisoned) and its keyword dict; nm = the rows of the context's map"""

    def __init__(self, Q, nm, Rt, radius, thr, cam, kps=None, feat=None, count=None, stride=2):
        torch = _torch()
        nq = len(Q)
        self.nq, self.nm = nq, nm
        self.keep = [_dev(Q if nq else np.zeros((1, 64), np.uint8))]
        self.match = torch.full((max(nq, 1),), -7, dtype=torch.int32, device="cuda")
        self.best = torch.full((max(nq, 1),), 7, dtype=torch.int16, device="cuda")
        self.second = torch.full((max(nq, 1),), 7, dtype=torch.int16, device="cuda")
        self.qpos = torch.full((2 * max(nq, 1),), 5.0, dtype=torch.float32, device="cuda")
        self.proj = torch.full((2 * max(nm, 1),), 5.0, dtype=torch.float32, device="cuda")
        side = {}
        if kps is not None:
            d = _dev(kps if len(kps) else np.zeros(1, dtype=kps.dtype))
            side["d_kps"] = d.data_ptr()
        else:
            f = np.full((max(len(feat), 1), stride), 7.0, dtype=np.float32)
            f[:len(feat), :2] = feat
            d = _dev(f)
            side["d_feat"], side["feat_stride"] = d.data_ptr(), stride
        self.keep.append(d)
        if count is not None:
            d = _dev(np.array([count, count + 17], dtype=np.uint32).view(np.int32))
            self.keep.append(d)
            side["d_count"] = d.data_ptr()
        torch.cuda.synchronize()
        self.kw = dict(d_q=self.keep[0].data_ptr(), nq=nq, cam=cam, Rt=Rt, radius=radius, threshold=thr, d_match=self.match.data_ptr(),
                       d_best=self.best.data_ptr(), d_second=self.second.data_ptr(), d_qpos=self.qpos.data_ptr(), d_proj=self.proj.data_ptr(), **side)

    def result(self):
        nq, nm = self.nq, self.nm
        return dict(match=self.match.cpu().numpy()[:nq], best=self.best.cpu().numpy()[:nq].view(np.uint16),
                    second=self.second.cpu().numpy()[:nq].view(np.uint16), qpos=self.qpos.cpu().numpy()[:2 * nq].reshape(-1, 2),
                    proj=self.proj.cpu().numpy()[:2 * nm].reshape(-1, 2))


def _same(got, st, what):
    assert np.array_equal(got["match"], st["match"]), (what, "match", int((got["match"] != st["match"]).sum()))
    assert np.array_equal(got["best"], st["best"]), (what, "best")
    assert np.array_equal(got["second"], st["second"]), (what, "second")
    assert gh.same_bits(got["qpos"], st["qpos"]), (what, "qpos")
    assert gh.same_bits(got["proj"], st["proj"]), (what, "proj")


def _run(ctx, *args, **kw):
    job = _Job(*args, **kw)
    ctx.match_map_guided_dev(**job.kw)
    ctx.sync()
    return job.result()


NMS = [1, 2, 7, 33, 513, 1500]


@pytest.mark.parametrize("nq", [1, 127, 128, 129, 300])
def test_shapes_equal_the_statement(monkeypatch, nq):
    ctx = _ctx(monkeypatch)
    try:
        for nm in NMS:
            Q, M, qpos, X = ph.make_case(nq, nm, 1000 * nq + nm)
            st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
            c = ph.classes(st, Q, M, 20)
            print("nq %d nm %d classes %s" % (nq, nm, c))
            if nq >= 127 and nm >= 33:
                assert ph.all_classes_occur(c), c
            plan = ctx.k2nn_plan_query(nq, nm)                         # a popcount context: the plan the guided sweep runs
            assert plan["queries_per_block"] == 128 and plan["qblocks"] == (nq + 127) // 128
            if nm == 1500:
                assert plan["splits"] >= 2, plan
            if nm <= 33:
                assert plan["splits"] == 1, plan
            ctx.set_map(M)
            ctx.set_map_points(X)
            _same(_run(ctx, Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos), st, (nq, nm))
    finally:
        ctx.close()


def test_the_3_4_5_edge_and_landmarks_without_a_projection(monkeypatch):
    """dx = 3, dy = 4, radius = 5 is a candidate, dy = 4.5 is not; a landmark behind the camera and one at Xc[2] == 0 EXACTLY carry the
    queries' exact copies and are never candidates"""
    Rt = _pose(C=(0.0, 0.0, -4.0))                                            # t = (0, 0, 4): the plane Z = -4 goes through the camera
    assert Rt[:, 3].tolist() == [0.0, 0.0, 4.0]
    qpos = np.array([[100.5, 200.0], [320.0, 240.0], [500.0, 100.0]], dtype=np.float32)
    px = [(103.5, 204.0), (103.5, 204.5), (97.5, 196.0), (320.0, 240.0)]
    X = [ph.landmark(x, y, 2.0) - (0.0, 0.0, 4.0) for x, y in px]            # depth 2 in front of the shifted camera
    X += [np.array([0.0, 0.0, -4.0]), np.array([1.0, 1.0, -4.0]), np.array([0.0, 0.0, -8.0]), ph.landmark(500.0, 100.0, -2.0) - (0.0, 0.0, 4.0)]
    X = np.array(X)
    rng = np.random.RandomState(5)
    Q, M = rng.randint(0, 256, (3, 64)).astype(np.uint8), rng.randint(0, 256, (8, 64)).astype(np.uint8)
    M[1] = Q[0]                                                               # just outside: K2NN alone would take it
    M[4], M[5], M[6] = Q[1], Q[1], Q[1]                                       # on the camera plane (twice) and behind it
    M[7] = Q[2]                                                               # behind, its pixel formula ON the query
    st = ph.statement(Q, M, X, Rt, 5.0, 0, gh.CAM_EXACT, feat=qpos)
    assert st["proj"][:4].tolist() == [list(p) for p in px]
    assert (st["proj"][4:].view(np.uint32) == gh.NONE_BITS).all()
    assert st["cand"].astype(int).tolist() == [[1, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]]
    assert gh.plain(Q, M, 0)[0].tolist() == [1, -1, 7]                         # (query 1: three exact copies tie)
    assert st["match"][1] == 3 and st["match"][2] == -1 and st["match"][0] in (0, 2)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        _same(_run(ctx, Q, 8, Rt, 5.0, 0, gh.CAM_EXACT, feat=qpos), st, "3-4-5")
    finally:
        ctx.close()


def _distort(uv, cam):
    """the distorted pixel of an undistorted one (Pinhole_Intrinsic_Radial_K3::add_disto): get_ud_pixel brings it back to within the
    bisection's 1e-10"""
    f, ppx, ppy, k1, k2, k3 = cam
    c = (np.asarray(uv, dtype=np.float64) - (ppx, ppy)) / f
    r2 = (c * c).sum(1, keepdims=True)
    return c * (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) * f + (ppx, ppy)


def _general_case(nq, nm, seed, cam, Rt):
    """landmarks seen (and some not seen) from a general pose; three queries in four are flipped copies of a map row, placed near the
    DISTORTED pixel of its projection.  Returns (Q, M, qpos float32, kps over all 8 levels at about the same positions, X)."""
    rng = np.random.RandomState(seed)
    M = rng.randint(0, 256, (nm, 64)).astype(np.uint8)
    Q = rng.randint(0, 256, (nq, 64)).astype(np.uint8)
    uv = np.column_stack([rng.uniform(-60, gh.W + 60, nm), rng.uniform(-60, gh.H + 60, nm)])
    depth = rng.uniform(2.0, 10.0, nm)
    depth[np.arange(nm) % 11 == 5] *= -1.0                                    # behind the camera
    Xc = np.column_stack([(uv[:, 0] - cam[1]) / cam[0] * depth, (uv[:, 1] - cam[2]) / cam[0] * depth, depth])
    X = (Xc - Rt[:, 3]) @ Rt[:, :3]                                           # R^T (Xc - t)
    qpos = np.column_stack([rng.uniform(10, gh.W - 10, nq), rng.uniform(10, gh.H - 10, nq)])
    rows = rng.permutation(nm)
    for q in range(nq):
        if q % 4 == 3 or q >= nm:
            continue
        m = rows[q]
        Q[q] = gh._flip(rng, M[m], 10)
        qpos[q] = _distort(uv[m:m + 1], cam)[0] + rng.uniform(-1.0, 1.0, 2)
    kps = np.zeros(nq, dtype=synth.KP_DTYPE)
    kps["scale"] = np.arange(nq) % 8
    s = track_host.level_scales(8)[kps["scale"]].astype(np.float64)
    kps["x"], kps["y"] = np.round(qpos[:, 0] / s), np.round(qpos[:, 1] / s)
    return Q, M, qpos.astype(np.float32), kps, X


def test_general_pose_distortion_and_both_row_forms(monkeypatch):
    nq, nm = 300, 513
    Rt = _pose(0.05, -0.1, 0.03, C=(0.3, -0.2, 0.5))
    Q, M, qpos, kps, X = _general_case(nq, nm, 4242, CAM_K, Rt)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        for kw in (dict(feat=qpos, stride=4), dict(kps=kps)):
            st = ph.statement(Q, M, X, Rt, 4.0, 20, CAM_K, **{k: v for k, v in kw.items() if k != "stride"})
            ncand = st["cand"].sum(1)
            noproj = (st["proj"].view(np.uint32) == gh.NONE_BITS).all(1)
            print("general pose, %s: %d accepted, %d without candidates, %d landmarks without a projection" %
                  (sorted(kw)[0], (st["match"] >= 0).sum(), (ncand == 0).sum(), noproj.sum()))
            assert (ncand == 0).any() and (ncand >= 2).any() and (st["match"] >= 0).sum() > 100 and 20 < noproj.sum() < 100
            assert not gh.same_bits(st["qpos"], qpos)                           # the distortion moved the query points
            _same(_run(ctx, Q, nm, Rt, 4.0, 20, CAM_K, **kw), st, sorted(kw)[0])
        assert set(kps["scale"].tolist()) == set(range(8))
    finally:
        ctx.close()


def test_device_side_count(monkeypatch):
    """rows at or past d_count[0] hold NaNs and are answered -1"""
    nq, nm = 300, 513
    Q, M, qpos, X = ph.make_case(nq, nm, 31)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        full = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        for cnt in (200, 129, 0, 1000):
            st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos, count=cnt)
            assert (st["match"][min(cnt, nq):] == -1).all() and (st["qpos"][min(cnt, nq):].view(np.uint32) == gh.NONE_BITS).all()
            assert np.array_equal(st["match"][:min(cnt, nq)], full["match"][:min(cnt, nq)])
            if cnt < nq:
                assert (full["match"][cnt:] >= 0).any()
            _same(_run(ctx, Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos, count=cnt), st, cnt)
    finally:
        ctx.close()


def test_batch_of_unequal_jobs_equals_the_single_calls(monkeypatch):
    """the cameras of one frame against the one map: different poses, radii, thresholds and nq, one job with d_count = 0"""
    nm = 1500
    Q, M, qpos, X = ph.make_case(300, nm, 77)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        shift = _pose(C=(0.015625, 0.0, 0.0))                                 # the projections move by 8 / z pixels
        args = [(Q, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, dict(feat=qpos)),
                (Q[:129], shift, 9.0, 35, gh.CAM_EXACT, dict(feat=qpos[:129], stride=4)),
                (Q[100:164], _pose(0.0, 0.0, 0.002), 2.5, 60, CAM_K, dict(feat=qpos[100:164], count=0)),
                (Q[:5], ph.IDENTITY, 1.0, 0, gh.CAM_EXACT, dict(feat=qpos[:5]))]
        for n_jobs in (3, 4):
            jobs = [_Job(a[0], nm, a[1], a[2], a[3], a[4], **a[5]) for a in args[:n_jobs]]
            ctx.match_map_guided_batch_dev([j.kw for j in jobs])
            ctx.sync()
            for i, (j, a) in enumerate(zip(jobs, args)):
                single = _run(ctx, a[0], nm, a[1], a[2], a[3], a[4], **a[5])
                st = ph.statement(a[0], M, X, a[1], a[2], a[3], a[4], **{k: v for k, v in a[5].items() if k != "stride"})
                _same(j.result(), single, ("batch == single", n_jobs, i))
                _same(single, st, ("single == statement", n_jobs, i))
                if i < 2:
                    assert (st["match"] >= 0).sum() > 20
                if i == 2:
                    assert (st["match"] == -1).all()
    finally:
        ctx.close()


def test_result_does_not_depend_on_the_formulation(monkeypatch):
    torch = _torch()
    nq, nm = 300, 1500
    Q, M, qpos, X = ph.make_case(nq, nm, 99)
    st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
    plain = gh.plain(Q, M, 20)[0]
    for formulation, qpb in (("matrix", 256), ("popcount", 128)):
        ctx = _ctx(monkeypatch, formulation, M=M, X=X)
        try:
            assert ctx.k2nn_plan_query(nq, nm)["queries_per_block"] == qpb           # the context really runs that formulation
            d_q = _dev(Q)
            d_plain = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for rep in range(2):                                                    # (a plain sweep of the context's own in between)
                _same(_run(ctx, Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos), st, (formulation, rep))
                ctx.match_map_dev(d_q.data_ptr(), nq, 20, d_plain.data_ptr())
                ctx.sync()
                assert np.array_equal(d_plain.cpu().numpy(), plain)
        finally:
            ctx.close()


def test_invariant_against_the_plain_map_match(monkeypatch):
    """where clc_match_map_dev's match lies inside the radius the guided match is that row; with a 2 000 px radius and every landmark in
    front the two d_match arrays are equal"""
    torch = _torch()
    nq, nm = 300, 1500
    Q, M, qpos, X = ph.make_case(nq, nm, 8, behind=False)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        job = _Job(Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        d_plain = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.match_map_dev(job.kw["d_q"], nq, 20, d_plain.data_ptr())
        ctx.match_map_guided_dev(**job.kw)
        ctx.sync()
        plain, got = d_plain.cpu().numpy(), job.result()
        assert np.array_equal(plain, gh.plain(Q, M, 20)[0])
        st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        inside = np.array([plain[q] >= 0 and st["cand"][q, plain[q]] for q in range(nq)])
        assert inside.sum() > 20 and np.array_equal(got["match"][inside], plain[inside])
        assert (got["match"] != plain).any()
        wide = _run(ctx, Q, nm, ph.IDENTITY, 2000.0, 20, gh.CAM_EXACT, feat=qpos)
        assert np.array_equal(wide["match"], plain)
    finally:
        ctx.close()


def test_chain_on_rendered_frames():
    """two rendered views through clc_map_init_batch_dev into a context with map and points; a third view through clc_match_map_dev ->
    clc_track_localize_dev, which gives pose P; then clc_match_map_guided_dev under P at a 4 px radius and clc_track_localize_dev again.
    The guided d_match is the statement's, every accepted pair passes the gate recomputed on the host, and the second solve's tracks are
    track_host's for that d_match.  What the scene yields is printed, not fixed in advance."""
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
        assert got["entered"] == [True] and got["map_n"] > 100, (got["entered"], got["map_n"], len(filt[0]["inliers"]))
        nm = got["map_n"]
        # the third view against the map: the plain match, the solve, the guided re-match under its pose, the solve again
        frame = dict(nq=cap, cam=cams[2], d_kps=kc, d_count=cntc)
        ctx.match_map_dev(desc[2].data_ptr(), cap, 60, d_plain.data_ptr(), None)
        first = ctx.track_localize_dev(d_match=d_plain.data_ptr(), seed=7, **frame)
        assert first["Rt"] is not None and len(first["inliers"]) > 30
        P, radius, thr = first["Rt"], 4.0, 60
        ctx.match_map_guided_dev(d_q=desc[2].data_ptr(), Rt=P, radius=radius, threshold=thr, d_match=d_guided.data_ptr(), **frame)
        second = ctx.track_localize_dev(d_match=d_guided.data_ptr(), seed=7, **frame)
        ctx.sync()
        # the statement, from the host copies of the same frame and map
        kps_c = ctxs[2].detect(capacity=cap)[0]                                  # the same pyramid through the host entry
        nc = len(kps_c)
        assert 150 < nc <= cap
        padded = np.concatenate([kps_c, np.zeros(cap - nc, dtype=kps_c.dtype)])
        rows = desc[0].cpu().numpy()[got["map_row"]]
        st = ph.statement(desc[2].cpu().numpy(), rows, got["X"], P, radius, thr, cams[2], kps=padded, count=nc)
        guided = d_guided.cpu().numpy()
        assert np.array_equal(guided, st["match"])
        # the gate, recomputed from the landmarks, P and the keypoints, pair by pair
        proj = ph.project(P, cams[2], got["X"])[0]
        xy = gh.ud_positions(cams[2], kps=kps_c).astype(np.float32)
        acc = np.nonzero(guided >= 0)[0]
        assert len(acc) > 0 and all(ph.gate(xy[q], proj[guided[q]:guided[q] + 1], ph.r2_of(radius))[0] for q in acc)
        tq, tm, _, _ = track_host.build_tracks(guided, got["X"], cams[2], kps=padded, count=nc)
        assert second["n_tracks"] == len(tq) == len(acc) and np.array_equal(second["track_query"], tq) and np.array_equal(second["track_map"], tm)
        plain = d_plain.cpu().numpy()
        print("chain: map of %d landmarks from %d inliers; view 3 with %d keypoints: plain %d tracks / %d inliers, guided (radius %.0f px under the "
              "first pose) %d tracks / %d inliers, %d of the guided matches not the plain match's"
              % (nm, len(filt[0]["inliers"]), nc, first["n_tracks"], len(first["inliers"]), radius, second["n_tracks"], len(second["inliers"]),
                 int((guided[acc] != plain[acc]).sum())))
    finally:
        for c in ctxs:
            c.close()


def build_map_guided_driver(out):
    from coloc_amd import build
    lib = build.build()
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "coloc_amd", "host"),
           os.path.join(ROOT, "tests", "host", "map_guided_policy_driver.cpp"), "-o", out, "-L", os.path.dirname(lib), "-lcoloc_hip", "-ldl",
           "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.check_call(cmd)
    return out


def test_policy_member_equals_the_entry(monkeypatch, tmp_path):
    """HIPMatcher::setMapPoints + matchSceneWithMapGuidedDev through a compiled driver: its d_match is clc_match_map_guided_dev's for the
    same map, pose and frame (Rt formed from the Pose3 as t = -R C)"""
    exe = build_map_guided_driver(str(tmp_path / "map_guided_policy_driver"))
    nq, nm, radius, thr = 300, 513, 4.0, 20
    C = (0.3, -0.2, 0.5)
    Rt = _pose(0.05, -0.1, 0.03, C=C)
    Q, M, _, kps, X = _general_case(nq, nm, 606, CAM_K, Rt)
    np.concatenate([CAM_K, Rt[:, :3].reshape(-1), C, [nq, nm, radius, thr], X.reshape(-1)]).astype(np.float64).tofile(tmp_path / "map_guided.bin")
    kps.tofile(tmp_path / "kps.bin")
    np.concatenate([Q.reshape(-1), M.reshape(-1)]).tofile(tmp_path / "desc.bin")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = np.fromfile(tmp_path / "map_guided_out.bin", dtype=np.int32)
    ctx = _ctx(monkeypatch, "matrix", M=M, X=X)
    try:
        want = _run(ctx, Q, nm, Rt, radius, thr, CAM_K, kps=kps)["match"]
    finally:
        ctx.close()
    assert (want >= 0).sum() > 20
    assert np.array_equal(got, want)


def test_errors_and_edges(monkeypatch):
    from coloc_amd import CLCError, Context, abi
    Q, M, qpos, X = ph.make_case(50, 40, 3)
    ctx = _ctx(monkeypatch, M=M, X=X)
    light = Context(device=0, detector=False, matcher=False)
    fresh, unpointed, short = _ctx(monkeypatch), _ctx(monkeypatch), _ctx(monkeypatch)
    try:
        job = _Job(Q, 40, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        kw = job.kw
        f = kw["d_feat"]
        count = _dev(np.array([50, 50], dtype=np.int32))
        nanRt, infRt = ph.IDENTITY.copy(), ph.IDENTITY.copy()
        nanRt[1, 2], infRt[2, 3] = np.nan, np.inf
        bad = [dict(kw, d_feat=None), dict(kw, d_kps=f),                                                                   # neither / both
               dict(kw, d_q=kw["d_q"] + 8), dict(kw, d_match=kw["d_match"] + 2), dict(kw, d_feat=f + 1), dict(kw, d_qpos=kw["d_qpos"] + 2),
               dict(kw, d_proj=kw["d_proj"] + 2), dict(kw, d_best=kw["d_best"] + 1), dict(kw, d_second=kw["d_second"] + 1),
               dict(kw, d_count=count.data_ptr() + 2),                                                                   # misaligned
               dict(kw, cam=(0.0,) + gh.CAM_EXACT[1:]), dict(kw, cam=(-3.0,) + gh.CAM_EXACT[1:]),                          # focal
               dict(kw, radius=0.0), dict(kw, radius=-1.0), dict(kw, radius=float("inf")), dict(kw, radius=float("nan")),   # radius
               dict(kw, radius=1e20), dict(kw, radius=1e-30),                                                             # r2 = inf / 0
               dict(kw, Rt=nanRt), dict(kw, Rt=infRt),                                                                    # Rt
               dict(kw, nq=-1), dict(kw, d_match=None), dict(kw, d_q=None)]
        for b in bad:
            with pytest.raises(CLCError) as e:
                ctx.match_map_guided_dev(**b)
            assert e.value.status == abi.CLC_ERR_BAD_ARG, b
        with pytest.raises(CLCError) as e:
            ctx.match_map_guided_batch_dev([kw] * (abi.MAX_BATCH + 1))
        assert e.value.status == abi.CLC_ERR_BAD_ARG
        assert ctx.lib.clc_match_map_guided_dev(ctx.h, None, None) == abi.CLC_ERR_BAD_ARG                                  # a null job
        # the context's state: no matcher options; no map; a map without points; fewer points than rows
        unpointed.set_map(M)
        short.set_map(M)
        short.set_map_points(X[:39])
        for c in (light, fresh, unpointed, short):
            with pytest.raises(CLCError) as e:
                c.match_map_guided_dev(**kw)
            assert e.value.status == abi.CLC_ERR_STATE
        ctx.sync()
        assert (job.match.cpu().numpy() == -7).all()                            # nothing was enqueued by any of them
        ctx.match_map_guided_batch_dev([])                                      # nothing to do
        ctx.match_map_guided_dev(**dict(kw, nq=0))                              # no queries: nothing written
        ctx.sync()
        assert (job.match.cpu().numpy() == -7).all() and (job.proj.cpu().numpy() == 5.0).all()
        # an empty map: every query -1, the query points still written
        unpointed.set_map(np.zeros((0, 64), dtype=np.uint8))
        unpointed.match_map_guided_dev(**kw)
        unpointed.sync()
        got = job.result()
        assert (got["match"] == -1).all() and (got["best"] == 65535).all() and (got["second"] == 65535).all()
        assert gh.same_bits(got["qpos"], qpos) and (job.proj.cpu().numpy() == 5.0).all()
    finally:
        for c in (ctx, light, fresh, unpointed, short):
            c.close()


def test_more_than_2_22_map_rows_is_a_capacity_error(monkeypatch):
    """the sweep's keys carry 22 index bits: a map of 2^22 + 1 rows is refused before anything is enqueued"""
    from coloc_amd import CLCError, abi
    n = (1 << 22) + 1
    ctx = _ctx(monkeypatch, maxkp=n)
    try:
        ctx.set_map(np.zeros((n, 64), dtype=np.uint8))
        ctx.set_map_points(np.zeros((n, 3)))
        Q, _, qpos, _ = ph.make_case(8, 1, 1)
        job = _Job(Q, 1, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        with pytest.raises(CLCError) as e:
            ctx.match_map_guided_dev(**dict(job.kw, d_proj=None))
        assert e.value.status == abi.CLC_ERR_CAPACITY
        ctx.sync()
        assert (job.match.cpu().numpy() == -7).all()
    finally:
        ctx.close()

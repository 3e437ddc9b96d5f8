"""The guided match on the device (include/coloc_hip.h: clc_match_guided_dev, clc_match_guided_batch_dev) against the host statement
(tests/guided_host.py).  Every comparison is EXACT: d_match, d_best, d_second, d_line and d_tpos equal the statement bit for bit.

One sweep workgroup holds 128 queries and its 8 waves cut a split, so the shapes straddle 128 queries, and the train counts run from
nothing through fewer rows than waves (1, 2, 7), one split (33) to several splits (513, 1500); what the plan really does is asserted,
not assumed.  The classes (queries with 0, 1 and >= 2 candidates, queries whose unrestricted best row lies outside the band, in-band
ties for the minimum) are asserted on the statement before the device is looked at, wherever the shape leaves room for all of them
(nq >= 127 and nt >= 33: with one query or a handful of train rows they cannot all occur).  A tie for the minimum is rejected, so the
"lowest index" of a tie is not observable in d_match; d_best == d_second is."""
import os
import subprocess

import numpy as np
import pytest

import guided_host as gh
import pair_host
import synth
import track_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM_A = (520.0, 320.0, 240.0, -0.05, 0.01, 0.002)
CAM_B = (500.0, 330.0, 235.0, 0.04, -0.01, 0.001)


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8).reshape(-1) if a.dtype.names else a).cuda()
    torch.cuda.synchronize()
    return t


def _ctx(monkeypatch, formulation="popcount", maxkp=2048):
    from coloc_amd import Context
    monkeypatch.setenv("CLC_K2NN_FORMULATION", formulation)
    return Context(device=0, detector=False, maxkp=maxkp)


def _general_F(cam_a, cam_b):
    """F = Kb^-T [t]_x R Ka^-1 of a small sideways motion: lines that are neither rows nor parallel"""
    a = 0.05
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.array([[1, 0, 0], [0, np.cos(0.02), -np.sin(0.02)], [0, np.sin(0.02), np.cos(0.02)]])
    t = np.array([1.0, 0.08, 0.05])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = lambda c: np.array([[1 / c[0], 0, -c[1] / c[0]], [0, 1 / c[0], -c[2] / c[0]], [0, 0, 1.0]])
    return Ki(cam_b).T @ tx @ R @ Ki(cam_a)


class _Job:
    """one job's device buffers (inputs uploaded, outputs poisoned) and its keyword dict"""

    def __init__(self, Q, T, F, band, thr, cam_a, cam_b, kps_a=None, feat_a=None, kps_b=None, feat_b=None, count_a=None, count_b=None, stride=2):
        torch = _torch()
        nq, nt = len(Q), len(T)
        self.nq, self.nt = nq, nt
        self.keep = [_dev(Q if nq else np.zeros((1, 64), np.uint8)), _dev(T if nt else np.zeros((1, 64), np.uint8))]
        self.match = torch.full((max(nq, 1),), -7, dtype=torch.int32, device="cuda")
        self.best = torch.full((max(nq, 1),), 7, dtype=torch.int16, device="cuda")
        self.second = torch.full((max(nq, 1),), 7, dtype=torch.int16, device="cuda")
        self.line = torch.full((3 * max(nq, 1),), 5.0, dtype=torch.float32, device="cuda")
        self.tpos = torch.full((2 * max(nt, 1),), 5.0, dtype=torch.float32, device="cuda")
        side = {}
        for name, kps, feat in (("a", kps_a, feat_a), ("b", kps_b, feat_b)):
            if kps is not None:
                d = _dev(kps if len(kps) else np.zeros(1, dtype=kps.dtype))
                side["d_kps_" + name] = d.data_ptr()
            else:
                f = np.full((max(len(feat), 1), stride), 7.0, dtype=np.float32)
                f[:len(feat), :2] = feat
                d = _dev(f)
                side["d_feat_" + name], side["feat_stride_" + name] = d.data_ptr(), stride
            self.keep.append(d)
        for name, c in (("a", count_a), ("b", count_b)):
            if c is not None:
                d = _dev(np.array([c, c + 17], dtype=np.uint32).view(np.int32))
                self.keep.append(d)
                side["d_count_" + name] = d.data_ptr()
        torch.cuda.synchronize()
        self.kw = dict(d_q=self.keep[0].data_ptr(), nq=nq, d_t=self.keep[1].data_ptr(), nt=nt, cam_a=cam_a, cam_b=cam_b, F=F, band=band,
                       threshold=thr, d_match=self.match.data_ptr(), d_best=self.best.data_ptr(), d_second=self.second.data_ptr(),
                       d_line=self.line.data_ptr(), d_tpos=self.tpos.data_ptr(), **side)

    def result(self):
        nq, nt = self.nq, self.nt
        return dict(match=self.match.cpu().numpy()[:nq], best=self.best.cpu().numpy()[:nq].view(np.uint16),
                    second=self.second.cpu().numpy()[:nq].view(np.uint16), line=self.line.cpu().numpy()[:3 * nq].reshape(-1, 3),
                    tpos=self.tpos.cpu().numpy()[:2 * nt].reshape(-1, 2))


def _same(got, st, what):
    assert np.array_equal(got["match"], st["match"]), (what, "match", int((got["match"] != st["match"]).sum()))
    assert np.array_equal(got["best"], st["best"]), (what, "best")
    assert np.array_equal(got["second"], st["second"]), (what, "second")
    assert gh.same_bits(got["line"], st["line"]), (what, "line")
    assert gh.same_bits(got["tpos"], st["tpos"]), (what, "tpos")


def _run(ctx, *args, **kw):
    job = _Job(*args, **kw)
    ctx.match_guided_dev(**job.kw)
    ctx.sync()
    return job.result()


NTS = [0, 1, 2, 7, 33, 513, 1500]


@pytest.mark.parametrize("nq", [1, 127, 128, 129, 300])
def test_shapes_equal_the_statement(monkeypatch, nq):
    ctx = _ctx(monkeypatch)
    try:
        for nt in NTS:
            Q, T, qpos, tpos = gh.make_case(nq, nt, 1000 * nq + nt)
            st = gh.statement(Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
            c = gh.classes(st, Q, T, 20)
            print("nq %d nt %d classes %s" % (nq, nt, c))
            if nq >= 127 and nt >= 33:
                assert min(c["none"], c["one"], c["many"], c["best_outside"], c["tie"]) > 0 and c["tie_rejected"], c
            plan = ctx.k2nn_plan_query(nq, nt)                         # a popcount context: the plan the guided sweep runs
            assert plan["queries_per_block"] == 128 and plan["qblocks"] == (nq + 127) // 128
            if nt == 1500:
                assert plan["splits"] >= 2, plan
            if 0 < nt <= 33:
                assert plan["splits"] == 1, plan
            _same(_run(ctx, Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos), st, (nq, nt))
    finally:
        ctx.close()


def test_batch_of_unequal_jobs_equals_the_single_calls(monkeypatch):
    ctx = _ctx(monkeypatch)
    try:
        shapes = [(300, 1500, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT), (129, 33, _general_F(CAM_A, CAM_B), 4.0, 35, CAM_A, CAM_B),
                  (5, 0, gh.F_ROWS, 1.0, 0, gh.CAM_EXACT, CAM_B), (64, 513, gh.F_ROWS, 2.5, 60, CAM_B, gh.CAM_EXACT)]
        cases = [gh.make_case(nq, nt, 77 + i) for i, (nq, nt, *_) in enumerate(shapes)]
        for n_jobs in (3, 4):
            jobs = [_Job(c[0], c[1], s[2], s[3], s[4], s[5], s[6], feat_a=c[2], feat_b=c[3]) for c, s in list(zip(cases, shapes))[:n_jobs]]
            ctx.match_guided_batch_dev([j.kw for j in jobs])
            ctx.sync()
            for i, (j, c, s) in enumerate(zip(jobs, cases, shapes)):
                single = _run(ctx, c[0], c[1], s[2], s[3], s[4], s[5], s[6], feat_a=c[2], feat_b=c[3])
                st = gh.statement(c[0], c[1], s[2], s[3], s[4], s[5], s[6], feat_a=c[2], feat_b=c[3])
                _same(j.result(), single, ("batch == single", n_jobs, i))
                _same(single, st, ("single == statement", n_jobs, i))
    finally:
        ctx.close()


def test_band_edge_is_inside(monkeypatch):
    """e = v_a - y_b exactly (F_ROWS, half-integer positions, the exact camera): |e| == band is a candidate, band + 0.5 is not"""
    ctx = _ctx(monkeypatch)
    try:
        qpos = np.array([[100.5, 100.5], [300.0, 200.0], [10.5, 50.5]], dtype=np.float32)
        tpos = np.array([[7.5, 98.5], [600.5, 102.5], [50.0, 98.0], [51.0, 103.0], [9.0, 202.0], [9.0, 197.5], [9.0, 48.0], [9.0, 53.5]], dtype=np.float32)
        assert np.array_equal(gh.ud_positions(gh.CAM_EXACT, feat=qpos), qpos.astype(np.float64))
        assert np.array_equal(gh.ud_positions(gh.CAM_EXACT, feat=tpos), tpos.astype(np.float64))
        rng = np.random.RandomState(5)
        Q, T = rng.randint(0, 256, (3, 64)).astype(np.uint8), rng.randint(0, 256, (8, 64)).astype(np.uint8)
        T[2] = Q[0]                                                        # the out-of-band rows are the exact copies: K2NN alone would take them
        T[5] = Q[1]
        T[7] = Q[2]
        st = gh.statement(Q, T, gh.F_ROWS, 2.0, 0, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
        assert st["line"].tolist() == [[0.0, -1.0, 100.5], [0.0, -1.0, 200.0], [0.0, -1.0, 50.5]]
        assert st["cand"].astype(int).tolist() == [[1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]]
        assert gh.plain(Q, T, 0)[0].tolist() == [2, 5, 7]
        assert st["match"][1] == 4 and st["match"][2] == -1 and st["match"][0] in (0, 1)
        _same(_run(ctx, Q, T, gh.F_ROWS, 2.0, 0, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos), st, "band edge")
    finally:
        ctx.close()


def test_distortion_and_both_row_forms(monkeypatch):
    ctx = _ctx(monkeypatch)
    try:
        nq, nt = 300, 513
        Q, T, qpos, tpos = gh.make_case(nq, nt, 4242)
        F = _general_F(CAM_A, CAM_B)
        st = gh.statement(Q, T, F, 3.0, 20, CAM_A, CAM_B, feat_a=qpos, feat_b=tpos)
        ncand = st["cand"].sum(1)
        assert (ncand == 0).any() and (ncand >= 2).any() and not gh.same_bits(st["tpos"], tpos)
        _same(_run(ctx, Q, T, F, 3.0, 20, CAM_A, CAM_B, feat_a=qpos, feat_b=tpos, stride=4), st, "k1 k2 k3 on both cameras")
        # detector keypoints on one side (all 8 levels), float rows on the other
        kps = synth.random_keypoints(nq, 640, 480, seed=9)
        kps["scale"][:64] = np.arange(64) % 8
        kpsb = synth.random_keypoints(nt, 640, 480, seed=10)
        kpsb["scale"][:64] = (3 + np.arange(64)) % 8
        for flip in (False, True):
            kw = dict(kps_b=kpsb, feat_a=qpos) if flip else dict(kps_a=kps, feat_b=tpos)
            st = gh.statement(Q, T, gh.F_ROWS, 3.0, 20, CAM_A, CAM_B, **kw)
            assert (st["cand"].sum(1) >= 1).any()
            _same(_run(ctx, Q, T, gh.F_ROWS, 3.0, 20, CAM_A, CAM_B, **kw), st, ("kps / feat", flip))
    finally:
        ctx.close()


def test_device_side_counts(monkeypatch):
    """rows past d_count_a are answered -1 (and hold no line), rows past d_count_b are never candidates"""
    ctx = _ctx(monkeypatch)
    try:
        nq, nt = 300, 513
        Q, T, qpos, tpos = gh.make_case(nq, nt, 31)
        full = gh.statement(Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
        for ca, cb in ((200, 400), (129, 7), (0, 513), (300, 0), (1000, 1000)):
            st = gh.statement(Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos, count_a=ca, count_b=cb)
            assert (st["match"][min(ca, nq):] == -1).all() and not st["cand"][:, min(cb, nt):].any()
            if ca < nq and cb < nt and cb > 7:
                assert (full["match"] >= cb).any() and (st["match"] != full["match"]).any()
            _same(_run(ctx, Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos, count_a=ca, count_b=cb), st, (ca, cb))
    finally:
        ctx.close()


def test_invariant_against_plain_k2nn(monkeypatch):
    """where the plain clc_match_2nn_dev match lies in the band the guided match is that row; with a band wider than the image diagonal
    the guided d_match is clc_match_2nn_dev's over all queries"""
    torch = _torch()
    ctx = _ctx(monkeypatch)
    try:
        nq, nt = 300, 1500
        Q, T, qpos, tpos = gh.make_case(nq, nt, 8)
        job = _Job(Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
        d_plain = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.match_2nn_dev(job.kw["d_q"], nq, job.kw["d_t"], nt, 20, d_plain.data_ptr())
        ctx.match_guided_dev(**job.kw)
        ctx.sync()
        plain, got = d_plain.cpu().numpy(), job.result()
        assert np.array_equal(plain, gh.plain(Q, T, 20)[0])
        st = gh.statement(Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
        inband = np.array([plain[q] >= 0 and st["cand"][q, plain[q]] for q in range(nq)])
        assert inband.sum() > 20 and np.array_equal(got["match"][inband], plain[inband])
        assert (got["match"] != plain).any()
        wide = _run(ctx, Q, T, gh.F_ROWS, 2000.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
        assert np.array_equal(wide["match"], plain)
    finally:
        ctx.close()


def test_result_does_not_depend_on_the_formulation(monkeypatch):
    Q, T, qpos, tpos = gh.make_case(300, 1500, 99)
    st = gh.statement(Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
    for formulation, qpb in (("matrix", 256), ("popcount", 128)):
        ctx = _ctx(monkeypatch, formulation)
        try:
            assert ctx.k2nn_plan_query(300, 1500)["queries_per_block"] == qpb       # the context really runs that formulation
            for rep in range(2):                                                    # (a plain sweep of the context's own in between)
                _same(_run(ctx, Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos), st, (formulation, rep))
                assert np.array_equal(ctx.match_2nn(Q, T, 20), gh.plain(Q, T, 20)[0])
        finally:
            ctx.close()


def test_chain_filter_guide_build():
    """one rendered pair: detect + describe both views, clc_match_2nn_dev, clc_pair_filter_dev('E'), the guided match under its F, then
    clc_pair_build_dev on the guided d_match: the pairs are exactly the statement's and every one satisfies the gate recomputed on the
    host.  What the scene yields is printed, not fixed in advance."""
    torch = _torch()
    from coloc_amd import Context
    w, h, cap, ppu = 640, 480, 2048, 100.0
    K = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1.0]])
    camA, camB = (520.0, 320.0, 240.0, 0.0, 0.0, 0.0), (520.0, 320.0, 240.0, -0.05, 0.01, 0.0)
    tex = synth.plane_texture()
    ca = Context(device=0, width=w, height=h, maxkp=cap, match_thresh=60, fast_thresh=60)
    cb = Context(device=0, width=w, height=h, maxkp=cap, match_thresh=60, fast_thresh=60)
    try:
        Ra, ta = synth.look_at_plane_pose((7.0, 7.0), 5.2)
        Rb, tb = synth.look_at_plane_pose((7.25, 6.85), 5.0, yaw=0.05, tilt=(0.03, -0.02))
        imgs = [_dev(synth.render_plane(tex, ppu, K, R, t, w, h)) for R, t in ((Ra, ta), (Rb, tb))]
        d_match = torch.full((cap,), -5, dtype=torch.int32, device="cuda")
        d_guided = torch.full((cap,), -5, dtype=torch.int32, device="cuda")
        desc = [torch.zeros((cap, 64), dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        bufs = []
        for c, img, d in ((ca, imgs[0], desc[0]), (cb, imgs[1], desc[1])):
            c.pyramid_build_dev(img.data_ptr(), w, h, w, None)
            c.detect_dev(None)
            c.describe_detected_dev(d.data_ptr(), None)
            bufs.append(c.detect_buffers())
        cb.sync()
        (ka, cnta, _), (kb, cntb, _) = bufs
        ca.match_2nn_dev(desc[0].data_ptr(), cap, desc[1].data_ptr(), cap, 60, d_match.data_ptr(), None)
        side = dict(nq=cap, nt=cap, cam_a=camA, cam_b=camB, d_kps_a=ka, d_kps_b=kb, d_count_a=cnta, d_count_b=cntb)
        flt = ca.pair_filter_dev("E", d_match=d_match.data_ptr(), img_wh=(w, h), seed=3, **side)
        assert flt["F"] is not None and len(flt["inliers"]) > 40
        band, thr = 2.0, 60
        ca.match_guided_dev(d_q=desc[0].data_ptr(), d_t=desc[1].data_ptr(), F=flt["F"], band=band, threshold=thr, d_match=d_guided.data_ptr(), **side)
        d_x1 = torch.zeros((2 * cap,), dtype=torch.float64, device="cuda")
        d_x2 = torch.zeros((2 * cap,), dtype=torch.float64, device="cuda")
        d_pq = torch.zeros((cap,), dtype=torch.int32, device="cuda")
        d_pt = torch.zeros((cap,), dtype=torch.int32, device="cuda")
        d_n = torch.zeros((4,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ca.pair_build_dev(d_x1.data_ptr(), d_x2.data_ptr(), d_pq.data_ptr(), d_pt.data_ptr(), d_n.data_ptr(), None, d_match=d_guided.data_ptr(), **side)
        ca.sync()
        kps_a, kps_b = ca.detect(capacity=cap)[0], cb.detect(capacity=cap)[0]      # the same pyramids through the host entry
        na, nb = len(kps_a), len(kps_b)
        assert 150 < na <= cap and 150 < nb <= cap
        pad = lambda k: np.concatenate([k, np.zeros(cap - len(k), dtype=k.dtype)])
        Q, T = desc[0].cpu().numpy(), desc[1].cpu().numpy()
        st = gh.statement(Q, T, flt["F"], band, thr, camA, camB, kps_a=pad(kps_a), kps_b=pad(kps_b), count_a=na, count_b=nb)
        assert np.array_equal(d_guided.cpu().numpy(), st["match"])
        N = int(d_n.cpu()[0])
        want = pair_host.build_pairs(st["match"], cap, camA, camB, kpsA=kps_a, kpsB=kps_b, countA=na, countB=nb)
        pq, pt = d_pq.cpu().numpy()[:N], d_pt.cpu().numpy()[:N]
        assert N == len(want[0]) and np.array_equal(pq, want[0]) and np.array_equal(pt, want[1])
        assert np.array_equal(d_x1.cpu().numpy()[:2 * N].view(np.uint64), want[2].reshape(-1).view(np.uint64))
        assert np.array_equal(d_x2.cpu().numpy()[:2 * N].view(np.uint64), want[3].reshape(-1).view(np.uint64))
        # the gate, recomputed from the positions on the host, pair by pair
        L = gh.lines(flt["F"], gh.ud_positions(camA, kps=kps_a))[0]
        xy = gh.ud_positions(camB, kps=kps_b).astype(np.float32)
        assert N > 0 and all(gh.gate(L[q], xy[t:t + 1], band)[0] for q, t in zip(pq, pt))
        plain = d_match.cpu().numpy()
        print("chain: %d / %d keypoints, plain K2NN %d matches, filter %d inliers, guided (band %.1f px) %d matches, %d of them not plain K2NN's"
              % (na, nb, int((plain >= 0).sum()), len(flt["inliers"]), band, N, int((st["match"][pq] != plain[pq]).sum())))
    finally:
        ca.close()
        cb.close()


def build_guided_driver(out):
    from coloc_amd import build
    lib = build.build()
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "coloc_amd", "host"),
           os.path.join(ROOT, "tests", "host", "guided_policy_driver.cpp"), "-o", out, "-L", os.path.dirname(lib), "-lcoloc_hip", "-ldl",
           "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.check_call(cmd)
    return out


@pytest.mark.parametrize("model", ["E", "F"])
def test_policy_member_equals_the_entry(monkeypatch, tmp_path, model):
    """HIPRobustMatcher::guidedMatchesPairDev through a compiled driver: its d_match is clc_match_guided_dev's for the same pair ('F': the
    model slot holds F; 'E': the member forms F = K2^-T E K1^-1, compared with the entry under that same product)"""
    exe = build_guided_driver(str(tmp_path / "guided_policy_driver"))
    nq, nt, band, thr = 300, 513, 3.0, 20
    Q, T, qpos, tpos = gh.make_case(nq, nt, 606)
    Ki = lambda c: np.array([[1 / c[0], 0, -c[1] / c[0]], [0, 1 / c[0], -c[2] / c[0]], [0, 0, 1.0]])
    if model == "F":
        M = F = gh.F_ROWS
    else:
        Ka, Kb = np.linalg.inv(Ki(CAM_A)), np.linalg.inv(Ki(CAM_B))
        M = Kb.T @ gh.F_ROWS @ Ka                                             # an "essential" matrix whose F is close to F_ROWS
        F = _mul3(_mul3(Ki(CAM_B).T, M), Ki(CAM_A))                             # the member's product, in its operation order
    head = [640, 480, *CAM_A, *CAM_B, ord(model), nq, nt, band, thr, *np.asarray(M, dtype=np.float64).reshape(9)]
    np.concatenate([head, qpos.astype(np.float64).reshape(-1), tpos.astype(np.float64).reshape(-1)]).astype(np.float64).tofile(tmp_path / "guided.bin")
    np.concatenate([Q.reshape(-1), T.reshape(-1)]).tofile(tmp_path / "desc.bin")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = np.fromfile(tmp_path / "guided_out.bin", dtype=np.int32)
    ctx = _ctx(monkeypatch, "matrix")
    try:
        want = _run(ctx, Q, T, F, band, thr, CAM_A, CAM_B, feat_a=qpos, feat_b=tpos)["match"]
    finally:
        ctx.close()
    assert (want >= 0).sum() > 20
    assert np.array_equal(got, want)


def _mul3(A, B):
    """hipgeom::mul: C(i, j) = A(i,0) B(0,j) + A(i,1) B(1,j) + A(i,2) B(2,j), left to right"""
    C = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            C[i, j] = A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j]
    return C


def test_edges(monkeypatch):
    from coloc_amd import CLCError, Context, abi
    ctx = _ctx(monkeypatch)
    light = Context(device=0, detector=False, matcher=False)
    try:
        Q, T, qpos, tpos = gh.make_case(50, 40, 3)
        job = _Job(Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
        kw = job.kw
        fa, fb = kw["d_feat_a"], kw["d_feat_b"]
        bad = [dict(kw, d_feat_a=None), dict(kw, d_kps_a=fa), dict(kw, d_feat_b=None), dict(kw, d_kps_b=fb),               # neither / both
               dict(kw, d_q=kw["d_q"] + 8), dict(kw, d_t=kw["d_t"] + 4), dict(kw, d_match=kw["d_match"] + 2), dict(kw, d_feat_b=fb + 1),
               dict(kw, d_line=kw["d_line"] + 2), dict(kw, d_best=kw["d_best"] + 1),                                    # misaligned
               dict(kw, cam_a=(0.0,) + gh.CAM_EXACT[1:]), dict(kw, cam_b=(-3.0,) + gh.CAM_EXACT[1:]),                    # focal
               dict(kw, band=0.0), dict(kw, band=-1.0), dict(kw, band=float("inf")), dict(kw, band=float("nan")),         # band
               dict(kw, nq=-1), dict(kw, nt=-1), dict(kw, d_match=None)]
        for b in bad:
            with pytest.raises(CLCError) as e:
                ctx.match_guided_dev(**b)
            assert e.value.status == abi.CLC_ERR_BAD_ARG, b
        with pytest.raises(CLCError) as e:
            ctx.match_guided_dev(**dict(kw, nt=(1 << 22) + 1))
        assert e.value.status == abi.CLC_ERR_CAPACITY
        with pytest.raises(CLCError) as e:
            light.match_guided_dev(**kw)
        assert e.value.status == abi.CLC_ERR_STATE
        with pytest.raises(CLCError) as e:
            ctx.match_guided_batch_dev([kw] * (abi.MAX_TRACK_PAIRS + 1))
        assert e.value.status == abi.CLC_ERR_BAD_ARG
        ctx.match_guided_batch_dev([])                                         # nothing to do
        ctx.match_guided_dev(**dict(kw, nq=0))                                 # no queries: nothing written
        ctx.sync()
        assert (job.match.cpu().numpy() == -7).all()
        # a NaN in F: no query has a line; F = 0 the same
        for F in (np.full((3, 3), np.nan), np.zeros((3, 3))):
            got = _run(ctx, Q, T, F, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
            assert (got["match"] == -1).all() and (got["line"].view(np.uint32) == gh.NONE_BITS).all()
            assert (got["best"] == 65535).all() and (got["second"] == 65535).all()
    finally:
        ctx.close()
        light.close()

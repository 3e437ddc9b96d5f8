"""The map match around a predicted pose through a cell grid on the device (include/coloc_hip.h: clc_match_map_binned_dev,
clc_match_map_binned_batch_dev, clc_map_bin_build_dev, clc_map_binned_plan).  Every comparison is EXACT: d_match, d_best, d_second, d_qpos
and d_proj equal the host statement (tests/proj_host.py) bit for bit, and equal clc_match_map_guided_dev's on the same inputs; the table
equals the numpy table builder (tests/bin_host.py).

The match kernel gives a query 16 lanes, so a wave holds 4 queries and a workgroup 16: the shapes straddle both, and the lanes per query
are asserted from the plan, not assumed.  A query reads its window's rows 16 at a time, so the cell loads straddle 16 and reach three
steps (40 rows).  What the plan is (BINNED or SWEEP) is asserted wherever a test depends on it."""
import os
import subprocess

import numpy as np
import pytest

import bin_host as bh
import guided_host as gh
import proj_host as ph
import synth
import track_host
import test_gpu_map_guided as tg                     # the guided entry's job buffers, poses and general-pose case: the same inputs

pytestmark = pytest.mark.gpu

ROOT = tg.ROOT
CAM_K = tg.CAM_K
_Job, _pose, _same, _ctx, _dev, _torch = tg._Job, tg._pose, tg._same, tg._ctx, tg._dev, tg._torch


def _run(ctx, *args, entry="match_map_binned_dev", **kw):
    job = _Job(*args, **kw)
    getattr(ctx, entry)(**job.kw)
    ctx.sync()
    return job.result()


def _both(ctx, st, what, *args, **kw):
    """the binned entry against the statement and against the guided entry on the same inputs"""
    got = _run(ctx, *args, **kw)
    _same(got, st, (what, "binned == statement"))
    _same(got, _run(ctx, *args, entry="match_map_guided_dev", **kw), (what, "binned == guided"))
    return got


def _plan_is(ctx, cam, radius, want, nm):
    p = ctx.map_binned_plan(cam, radius)
    assert p["plan"] == want == bh.plan(cam, radius, nm), (p, radius, nm)
    assert p["cells_per_axis"] == bh.AXIS and p["lanes_per_query"] == 16 and p["cell_side"] == bh.grid(cam, radius)[2]
    return p


@pytest.mark.parametrize("nq", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 300])
def test_shapes_equal_the_statement_and_the_guided_entry(monkeypatch, nq):
    ctx = _ctx(monkeypatch)
    try:
        for nm in tg.NMS:
            Q, M, qpos, X = ph.make_case(nq, nm, 1000 * nq + nm)
            st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
            c = ph.classes(st, Q, M, 20)
            print("nq %d nm %d classes %s" % (nq, nm, c))
            if nq >= 127 and nm >= 33:
                assert ph.all_classes_occur(c), c
            ctx.set_map(M)
            ctx.set_map_points(X)
            p = _plan_is(ctx, gh.CAM_EXACT, 3.0, bh.BINNED, nm)
            assert 64 // p["lanes_per_query"] == 4                           # 4 queries per wave, 16 per workgroup: what nq straddles
            _both(ctx, st, (nq, nm), Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
    finally:
        ctx.close()


LOADS = [0, 1, 15, 16, 17, 40]


def _loaded_cells(seed):
    """a map whose cells (kx, ky) = (11 + 4 j, 11) -- x in [100 + 40 j, 110 + 40 j), y in [100, 110), cells of 10 px -- hold LOADS[j] rows
    at half-integer positions, a few rows elsewhere, and queries in and around those cells: flipped copies of rows, near them"""
    rng = np.random.RandomState(seed)
    pos = []
    for j, n in enumerate(LOADS):
        slots = [(100.5 + 40 * j + a, 100.5 + b) for a in range(10) for b in range(10)]
        pos += [slots[i] for i in rng.permutation(100)[:n]]
    pos += [(400.5 + 20 * i, 300.5) for i in range(5)]
    pos = np.array(pos)
    nm = len(pos)
    M = rng.randint(0, 256, (nm, 64)).astype(np.uint8)
    X = np.array([ph.landmark(x, y, 2.0 ** rng.randint(0, 4)) for x, y in pos])
    qpos, Q = [], []
    for j in range(len(LOADS)):
        for dx, dy in ((5.0, 5.0), (0.0, 0.0), (9.5, 2.5), (-2.0, 5.0), (12.0, 12.0), (5.0, -2.5)):     # centre, corner, edges, the neighbours
            qpos.append((100.0 + 40 * j + dx, 100.0 + dy))
    qpos = np.array(qpos, dtype=np.float32)
    for q in range(len(qpos)):
        d = np.abs(pos - qpos[q]).max(1)
        near = np.nonzero(d <= 2.0)[0]
        Q.append(gh._flip(rng, M[near[rng.randint(len(near))]], 8) if len(near) and q % 5 else rng.randint(0, 256, 64).astype(np.uint8))
    return np.array(Q, dtype=np.uint8), M, qpos, X, pos


def test_cell_loads_straddle_the_16_row_step(monkeypatch):
    Q, M, qpos, X, pos = _loaded_cells(12)
    nm = len(M)
    st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
    rw, W, c = bh.grid(gh.CAM_EXACT, 3.0)
    assert c == 10.0
    cell_start, _ = bh.table(st["proj"], c)
    assert [int(cell_start[11 * bh.AXIS + 11 + 4 * j + 1] - cell_start[11 * bh.AXIS + 11 + 4 * j]) for j in range(len(LOADS))] == LOADS
    visits = bh.visited(st["qpos"], st["proj"], rw, c)
    ncand = st["cand"].sum(1)
    print("cell loads: rows visited per query %s, candidates %s, accepted %d" % (sorted(set(visits.tolist())), sorted(set(ncand.tolist())), (st["match"] >= 0).sum()))
    assert visits.max() >= 40 and visits.min() == 0 and (ncand >= 2).any() and (st["match"] >= 0).sum() >= 10
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        _plan_is(ctx, gh.CAM_EXACT, 3.0, bh.BINNED, nm)
        _both(ctx, st, "cell loads", Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
    finally:
        ctx.close()


def test_ring_cells_borders_and_maps_without_projections(monkeypatch):
    rng = np.random.RandomState(21)
    ctx = _ctx(monkeypatch)
    try:
        # (a) every row in ONE ring cell, far outside the image; queries out there with them, and inside the image with nothing
        nm = 50
        pos = np.array([(-5000.5 - 0.5 * (i % 10), -4000.5 - 0.5 * (i // 10)) for i in range(nm)])
        M = rng.randint(0, 256, (nm, 64)).astype(np.uint8)
        X = np.array([ph.landmark(x, y, 1.0) for x, y in pos])
        qpos = np.array([pos[3], pos[17] + (0.5, 0.0), pos[44], (-5010.0, -4000.5), (100.0, 100.0), (0.0, 0.0), (-1e6, -1e6), (1e30, 3.0)], dtype=np.float32)
        Q = np.array([gh._flip(rng, M[i], 6) for i in (3, 17, 44, 9, 1, 2, 5, 6)], dtype=np.uint8)
        st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        cell_start, _ = bh.table(st["proj"], 10.0)
        assert cell_start[1] == nm and cell_start[0] == 0                     # all of them in cell (0, 0)
        assert (st["match"][:3] == [3, 17, 44]).all() and (st["match"][3:] == -1).all()
        assert bh.visited(st["qpos"], st["proj"], *bh.grid(gh.CAM_EXACT, 3.0)[::2]).tolist()[:8] == [nm, nm, nm, nm, 0, nm, nm, 0]
        ctx.set_map(M)
        ctx.set_map_points(X)
        _plan_is(ctx, gh.CAM_EXACT, 3.0, bh.BINNED, nm)
        _both(ctx, st, "one ring cell", Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        # (b) no row has a projection
        Xb = X.copy()
        Xb[:, 2] = -np.abs(Xb[:, 2])
        Xb[::3, 2] = 0.0
        st = ph.statement(Q, M, Xb, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        assert (st["proj"].view(np.uint32) == gh.NONE_BITS).all() and (st["match"] == -1).all()
        ctx.set_map_points(Xb)
        _both(ctx, st, "no projections", Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        # (c) queries exactly on cell borders and in the ring, rows on both sides of the borders
        qpos = np.array([(100.0, 200.0), (110.0, 200.0), (100.0, 210.0), (0.0, 0.0), (640.0, 480.0), (-3.0, 100.0), (650.0, 490.0), (320.0, -2.0),
                         (630.0, 10.0), (10.0, 470.0)], dtype=np.float32)
        offs = [(-2.5, 0.0), (2.5, 0.0), (0.0, -2.5), (0.0, 2.5), (-2.0, -2.0), (2.0, 2.0), (3.0, 0.0), (0.0, -3.0), (3.5, 0.0), (-0.5, 0.5)]
        pos = np.array([q + o for q in qpos.astype(np.float64) for o in offs])
        nm = len(pos)
        M = rng.randint(0, 256, (nm, 64)).astype(np.uint8)
        X = np.array([ph.landmark(x, y, 2.0) for x, y in pos])
        Q = np.array([gh._flip(rng, M[len(offs) * q + rng.randint(len(offs))], 5) for q in range(len(qpos))], dtype=np.uint8)
        st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        assert gh.same_bits(st["proj"], pos.astype(np.float32))
        ncand = st["cand"].sum(1)
        w = bh.windows(st["qpos"], *bh.grid(gh.CAM_EXACT, 3.0)[::2])
        print("borders: candidates per query %s, windows %s" % (ncand.tolist(), w.tolist()))
        assert (ncand == 9).all() and (w[:, 1] - w[:, 0]).max() <= 2 and (w == 0).any() and (w == 65).any()
        assert (st["match"] >= 0).sum() >= 5
        ctx.set_map(M)
        ctx.set_map_points(X)
        _both(ctx, st, "borders and ring", Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
    finally:
        ctx.close()


def test_the_3_4_5_edge_and_landmarks_without_a_projection(monkeypatch):
    """the guided test's case: dx = 3, dy = 4, radius = 5 is a candidate, dy = 4.5 is not; a landmark behind the camera and one at
    Xc[2] == 0 EXACTLY carry the queries' exact copies and are never candidates, and never binned"""
    Rt = _pose(C=(0.0, 0.0, -4.0))
    qpos = np.array([[100.5, 200.0], [320.0, 240.0], [500.0, 100.0]], dtype=np.float32)
    px = [(103.5, 204.0), (103.5, 204.5), (97.5, 196.0), (320.0, 240.0)]
    X = [ph.landmark(x, y, 2.0) - (0.0, 0.0, 4.0) for x, y in px]
    X += [np.array([0.0, 0.0, -4.0]), np.array([1.0, 1.0, -4.0]), np.array([0.0, 0.0, -8.0]), ph.landmark(500.0, 100.0, -2.0) - (0.0, 0.0, 4.0)]
    X = np.array(X)
    rng = np.random.RandomState(5)
    Q, M = rng.randint(0, 256, (3, 64)).astype(np.uint8), rng.randint(0, 256, (8, 64)).astype(np.uint8)
    M[1] = Q[0]
    M[4], M[5], M[6] = Q[1], Q[1], Q[1]
    M[7] = Q[2]
    st = ph.statement(Q, M, X, Rt, 5.0, 0, gh.CAM_EXACT, feat=qpos)
    assert st["cand"].astype(int).tolist() == [[1, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0]]
    assert st["match"][1] == 3 and st["match"][2] == -1 and st["match"][0] in (0, 2)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        _plan_is(ctx, gh.CAM_EXACT, 5.0, bh.BINNED, 8)
        _both(ctx, st, "3-4-5", Q, 8, Rt, 5.0, 0, gh.CAM_EXACT, feat=qpos)
        d_start, d_row = _dev(np.full(bh.CELLS + 1, -3, dtype=np.int32)), _dev(np.full(8, -3, dtype=np.int32))
        job = _Job(Q, 8, Rt, 5.0, 0, gh.CAM_EXACT, feat=qpos)
        ctx.map_bin_build_dev(d_start.data_ptr(), d_row.data_ptr(), **job.kw)
        ctx.sync()
        assert d_start.cpu().numpy()[-1] == 4 and sorted(d_row.cpu().numpy().tolist()) == [-3, -3, -3, -3, 0, 1, 2, 3]
    finally:
        ctx.close()


def test_plan_sweep_runs_the_guided_path(monkeypatch):
    """a radius wider than the grid takes (2 000 px) equals clc_match_map_dev with every landmark in front; a radius below 2^-10 equals the
    statement; both are SWEEP"""
    torch = _torch()
    nq, nm = 300, 1500
    Q, M, qpos, X = ph.make_case(nq, nm, 8, behind=False)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        _plan_is(ctx, gh.CAM_EXACT, 2000.0, bh.SWEEP, nm)
        _plan_is(ctx, gh.CAM_EXACT, 2.0 ** -11, bh.SWEEP, nm)
        d_plain = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        d_q = _dev(Q)
        ctx.match_map_dev(d_q.data_ptr(), nq, 20, d_plain.data_ptr())
        ctx.sync()
        plain = d_plain.cpu().numpy()
        assert np.array_equal(plain, gh.plain(Q, M, 20)[0]) and (plain >= 0).sum() > 20
        wide = _run(ctx, Q, nm, ph.IDENTITY, 2000.0, 20, gh.CAM_EXACT, feat=qpos)
        assert np.array_equal(wide["match"], plain)
        # tiny radius: only a projection ON the query is a candidate
        qp = qpos.copy()
        st = ph.statement(Q, M, X, ph.IDENTITY, 2.0 ** -11, 20, gh.CAM_EXACT, feat=qp)
        assert 0 < st["cand"].sum() and (st["match"] >= 0).any()
        _both(ctx, st, "radius 2^-11", Q, nm, ph.IDENTITY, 2.0 ** -11, 20, gh.CAM_EXACT, feat=qp)
    finally:
        ctx.close()


def test_general_pose_distortion_and_both_row_forms(monkeypatch):
    nq, nm = 300, 513
    Rt = _pose(0.05, -0.1, 0.03, C=(0.3, -0.2, 0.5))
    Q, M, qpos, kps, X = tg._general_case(nq, nm, 4242, CAM_K, Rt)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        _plan_is(ctx, CAM_K, 4.0, bh.BINNED, nm)
        for kw in (dict(feat=qpos, stride=4), dict(kps=kps)):
            st = ph.statement(Q, M, X, Rt, 4.0, 20, CAM_K, **{k: v for k, v in kw.items() if k != "stride"})
            ncand = st["cand"].sum(1)
            noproj = (st["proj"].view(np.uint32) == gh.NONE_BITS).all(1)
            assert (ncand == 0).any() and (ncand >= 2).any() and (st["match"] >= 0).sum() > 100 and 20 < noproj.sum() < 100
            assert not gh.same_bits(st["qpos"], qpos)                           # the distortion moved the query points
            _both(ctx, st, sorted(kw)[0], Q, nm, Rt, 4.0, 20, CAM_K, **kw)
        assert set(kps["scale"].tolist()) == set(range(8))
    finally:
        ctx.close()


def test_device_side_count(monkeypatch):
    """rows at or past d_count[0] hold NaNs, have no window and are answered -1"""
    nq, nm = 300, 513
    Q, M, qpos, X = ph.make_case(nq, nm, 31)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        _plan_is(ctx, gh.CAM_EXACT, 3.0, bh.BINNED, nm)
        full = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        for cnt in (200, 129, 0, 1000):
            st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos, count=cnt)
            assert (st["match"][min(cnt, nq):] == -1).all() and (st["qpos"][min(cnt, nq):].view(np.uint32) == gh.NONE_BITS).all()
            if cnt < nq:
                assert (full["match"][cnt:] >= 0).any()
            _both(ctx, st, cnt, Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos, count=cnt)
    finally:
        ctx.close()


def test_batch_of_unequal_jobs_equals_the_single_calls(monkeypatch):
    """four jobs against the one map: different poses, radii, thresholds and nq; one is SWEEP by its radius, one has d_count = 0"""
    nm = 1500
    Q, M, qpos, X = ph.make_case(300, nm, 77)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        shift = _pose(C=(0.015625, 0.0, 0.0))                                 # the projections move by 8 / z pixels
        args = [(Q, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, dict(feat=qpos)),
                (Q[:129], shift, 100.0, 35, gh.CAM_EXACT, dict(feat=qpos[:129], stride=4)),
                (Q[100:164], _pose(0.0, 0.0, 0.002), 2.5, 60, CAM_K, dict(feat=qpos[100:164], count=0)),
                (Q[:5], ph.IDENTITY, 1.0, 0, gh.CAM_EXACT, dict(feat=qpos[:5]))]
        assert [ctx.map_binned_plan(a[4], a[2])["plan"] for a in args] == [bh.BINNED, bh.SWEEP, bh.BINNED, bh.BINNED]
        for n_jobs in (3, 4):
            jobs = [_Job(a[0], nm, a[1], a[2], a[3], a[4], **a[5]) for a in args[:n_jobs]]
            ctx.match_map_binned_batch_dev([j.kw for j in jobs])
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


def test_the_same_call_three_times_gives_the_same_bits(monkeypatch):
    nq, nm = 300, 1500
    Q, M, qpos, X = ph.make_case(nq, nm, 99)
    ctx = _ctx(monkeypatch, M=M, X=X)
    try:
        _plan_is(ctx, gh.CAM_EXACT, 3.0, bh.BINNED, nm)
        job = _Job(Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        runs = []
        for _ in range(3):
            ctx.match_map_binned_dev(**job.kw)
            ctx.sync()
            runs.append(job.result())
        _same(runs[1], runs[0], "second call")
        _same(runs[2], runs[0], "third call")
        _same(runs[0], ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos), "statement")
    finally:
        ctx.close()


def test_bin_build_equals_the_numpy_table(monkeypatch):
    ctx = _ctx(monkeypatch)
    try:
        cases = [ph.make_case(40, 1500, 5) + (3.0,), _loaded_cells(13)[:4] + (3.0,), ph.make_case(10, 513, 6) + (30.0,)]
        for Q, M, qpos, X, radius in cases:
            nm = len(M)
            ctx.set_map(M)
            ctx.set_map_points(X)
            job = _Job(Q, nm, ph.IDENTITY, radius, 20, gh.CAM_EXACT, feat=qpos)
            d_start, d_row = _dev(np.full(bh.CELLS + 1, -3, dtype=np.int32)), _dev(np.full(nm, -3, dtype=np.int32))
            ctx.map_bin_build_dev(d_start.data_ptr(), d_row.data_ptr(), **job.kw)
            ctx.sync()
            st = ph.statement(Q, M, X, ph.IDENTITY, radius, 20, gh.CAM_EXACT, feat=qpos)
            cell_start, cell_row = bh.table(st["proj"], bh.grid(gh.CAM_EXACT, radius)[2])
            got_start, got_row = d_start.cpu().numpy(), d_row.cpu().numpy()
            assert np.array_equal(got_start, cell_start)
            n = int(cell_start[-1])
            noproj = np.nonzero((st["proj"].view(np.uint32) == gh.NONE_BITS).all(1))[0]
            assert n == nm - len(noproj) and (got_row[n:] == -3).all()                 # not written past the binned rows
            assert not set(got_row[:n].tolist()) & set(noproj.tolist())                 # rows without a projection are absent
            for cell in np.nonzero(np.diff(cell_start))[0]:
                a, b = cell_start[cell], cell_start[cell + 1]
                assert np.array_equal(np.sort(got_row[a:b]), cell_row[a:b]), cell
            got = job.result()
            assert gh.same_bits(got["proj"], st["proj"]) and gh.same_bits(got["qpos"], st["qpos"]) and (got["match"] == -7).all()
        assert len(noproj) > 0
    finally:
        ctx.close()


def test_chain_on_rendered_frames():
    """the guided test's chain -- two rendered views into a map, a third view matched, solved, then RE-MATCHED under the solve's pose --
    with the binned entry in the re-match: its d_match is the guided entry's, and clc_track_localize_dev from it gives the same tracks"""
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
        d_pair, d_plain, d_guided, d_binned = (torch.full((cap,), -5, dtype=torch.int32, device="cuda") for _ in range(4))
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
        P, radius, thr = first["Rt"], 4.0, 60
        assert ctx.map_binned_plan(cams[2], radius)["plan"] == bh.BINNED
        ctx.match_map_guided_dev(d_q=desc[2].data_ptr(), Rt=P, radius=radius, threshold=thr, d_match=d_guided.data_ptr(), **frame)
        second = ctx.track_localize_dev(d_match=d_guided.data_ptr(), seed=7, **frame)
        ctx.match_map_binned_dev(d_q=desc[2].data_ptr(), Rt=P, radius=radius, threshold=thr, d_match=d_binned.data_ptr(), **frame)
        third = ctx.track_localize_dev(d_match=d_binned.data_ptr(), seed=7, **frame)
        ctx.sync()
        guided, binned = d_guided.cpu().numpy(), d_binned.cpu().numpy()
        assert np.array_equal(binned, guided) and (binned >= 0).sum() > first["n_tracks"]
        assert third["n_tracks"] == second["n_tracks"] == (binned >= 0).sum()
        assert np.array_equal(third["track_query"], second["track_query"]) and np.array_equal(third["track_map"], second["track_map"])
        print("chain: plain %d tracks, guided %d, binned %d" % (first["n_tracks"], second["n_tracks"], third["n_tracks"]))
    finally:
        for c in ctxs:
            c.close()


def test_policy_member_equals_the_entry(monkeypatch, tmp_path):
    """HIPMatcher::setMapPoints + matchSceneWithMapBinnedDev through a compiled driver: its d_match is clc_match_map_binned_dev's for the
    same map, pose and frame"""
    from coloc_amd import build
    lib = build.build()
    exe = str(tmp_path / "map_binned_policy_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "coloc_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "map_binned_policy_driver.cpp"), "-o", exe, "-L", os.path.dirname(lib), "-lcoloc_hip",
                           "-ldl", "-Wl,-rpath," + os.path.dirname(lib)])
    nq, nm, radius, thr = 300, 513, 4.0, 20
    C = (0.3, -0.2, 0.5)
    Rt = _pose(0.05, -0.1, 0.03, C=C)
    Q, M, _, kps, X = tg._general_case(nq, nm, 606, CAM_K, Rt)
    np.concatenate([CAM_K, Rt[:, :3].reshape(-1), C, [nq, nm, radius, thr], X.reshape(-1)]).astype(np.float64).tofile(tmp_path / "map_binned.bin")
    kps.tofile(tmp_path / "kps.bin")
    np.concatenate([Q.reshape(-1), M.reshape(-1)]).tofile(tmp_path / "desc.bin")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = np.fromfile(tmp_path / "map_binned_out.bin", dtype=np.int32)
    ctx = _ctx(monkeypatch, "matrix", M=M, X=X)
    try:
        assert ctx.map_binned_plan(CAM_K, radius)["plan"] == bh.BINNED
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
        d_start, d_row = _dev(np.full(bh.CELLS + 1, -3, dtype=np.int32)), _dev(np.full(40, -3, dtype=np.int32))
        table = (d_start.data_ptr(), d_row.data_ptr())
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
                ctx.match_map_binned_dev(**b)
            assert e.value.status == abi.CLC_ERR_BAD_ARG, b
            with pytest.raises(CLCError) as e:
                ctx.map_bin_build_dev(*table, **b)
            assert e.value.status == abi.CLC_ERR_BAD_ARG, b
        for t in ((None, table[1]), (table[0], None), (table[0] + 2, table[1]), (table[0], table[1] + 2)):                # the table itself
            with pytest.raises(CLCError) as e:
                ctx.map_bin_build_dev(*t, **kw)
            assert e.value.status == abi.CLC_ERR_BAD_ARG, t
        with pytest.raises(CLCError) as e:
            ctx.map_bin_build_dev(*table, **dict(kw, cam=(512.0, 0.0, 240.0, 0, 0, 0)))                                    # the grid has no extent
        assert e.value.status == abi.CLC_ERR_BAD_ARG
        with pytest.raises(CLCError) as e:
            ctx.match_map_binned_batch_dev([kw] * (abi.MAX_BATCH + 1))
        assert e.value.status == abi.CLC_ERR_BAD_ARG
        assert ctx.lib.clc_match_map_binned_dev(ctx.h, None, None) == abi.CLC_ERR_BAD_ARG                                  # a null job
        assert ctx.lib.clc_map_bin_build_dev(ctx.h, None, table[0], table[1], None) == abi.CLC_ERR_BAD_ARG
        # the context's state: no matcher options; no map; a map without points; fewer points than rows
        unpointed.set_map(M)
        short.set_map(M)
        short.set_map_points(X[:39])
        for c in (light, fresh, unpointed, short):
            with pytest.raises(CLCError) as e:
                c.match_map_binned_dev(**kw)
            assert e.value.status == abi.CLC_ERR_STATE
            with pytest.raises(CLCError) as e:
                c.map_bin_build_dev(*table, **kw)
            assert e.value.status == abi.CLC_ERR_STATE
        assert fresh.map_binned_plan(gh.CAM_EXACT, 3.0)["plan"] == bh.SWEEP                                                # no map: nothing to bin
        ctx.sync()
        assert (job.match.cpu().numpy() == -7).all() and (d_start.cpu().numpy() == -3).all()   # nothing was enqueued by any of them
        ctx.match_map_binned_batch_dev([])                                      # nothing to do
        ctx.match_map_binned_dev(**dict(kw, nq=0))                              # no queries: nothing written
        ctx.sync()
        assert (job.match.cpu().numpy() == -7).all() and (job.proj.cpu().numpy() == 5.0).all()
        # an empty map: every query -1, the query points still written
        unpointed.set_map(np.zeros((0, 64), dtype=np.uint8))
        assert unpointed.map_binned_plan(gh.CAM_EXACT, 3.0)["plan"] == bh.SWEEP
        unpointed.match_map_binned_dev(**kw)
        unpointed.sync()
        got = job.result()
        assert (got["match"] == -1).all() and (got["best"] == 65535).all() and (got["second"] == 65535).all()
        assert gh.same_bits(got["qpos"], qpos) and (job.proj.cpu().numpy() == 5.0).all()
    finally:
        for c in (ctx, light, fresh, unpointed, short):
            c.close()


def test_the_row_limits(monkeypatch):
    """65 536 map rows are binned, 65 537 are swept (and refused by clc_map_bin_build_dev); the result is the guided entry's on both
    sides.  More than 2^22 rows: CLC_ERR_CAPACITY before anything is enqueued, as for the guided entry."""
    from coloc_amd import CLCError, abi
    rng = np.random.RandomState(9)
    n = 65537
    Q, _, qpos, _ = ph.make_case(64, 1, 1)
    M = rng.randint(0, 256, (n, 64)).astype(np.uint8)
    pos = np.column_stack([rng.randint(0, 1280, n) * 0.5, rng.randint(0, 960, n) * 0.5])
    X = np.array([ph.landmark(x, y, 2.0) for x, y in pos])
    for q in range(0, 64, 2):                                                  # half the queries sit near a row that is their flipped copy
        m = 65535 if q == 0 else rng.randint(n)
        Q[q] = gh._flip(rng, M[m], 6)
        qpos[q] = pos[m] + (0.5, -0.5)
    ctx = _ctx(monkeypatch, maxkp=n)
    try:
        d_start, d_row = _dev(np.full(bh.CELLS + 1, -3, dtype=np.int32)), _dev(np.full(n, -3, dtype=np.int32))
        for nm, want in ((65536, bh.BINNED), (65537, bh.SWEEP)):
            ctx.set_map(M[:nm])
            ctx.set_map_points(X[:nm])
            _plan_is(ctx, gh.CAM_EXACT, 3.0, want, nm)
            job = _Job(Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
            ctx.match_map_binned_dev(**job.kw)
            ctx.sync()
            got = job.result()
            _same(got, _run(ctx, Q, nm, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos, entry="match_map_guided_dev"), nm)
            assert (got["match"] >= 0).sum() >= 16 and got["match"][0] == 65535
            if nm == 65536:
                ctx.map_bin_build_dev(d_start.data_ptr(), d_row.data_ptr(), **job.kw)
                ctx.sync()
                cell_start, _ = bh.table(got["proj"], 10.0)
                assert np.array_equal(d_start.cpu().numpy(), cell_start) and cell_start[-1] == nm
                assert np.array_equal(np.sort(d_row.cpu().numpy()[:nm]), np.arange(nm))
            else:
                with pytest.raises(CLCError) as e:
                    ctx.map_bin_build_dev(d_start.data_ptr(), d_row.data_ptr(), **job.kw)
                assert e.value.status == abi.CLC_ERR_CAPACITY
    finally:
        ctx.close()
    big = (1 << 22) + 1
    ctx = _ctx(monkeypatch, maxkp=big)
    try:
        ctx.set_map(np.zeros((big, 64), dtype=np.uint8))
        ctx.set_map_points(np.zeros((big, 3)))
        job = _Job(Q[:8], 1, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos[:8])
        with pytest.raises(CLCError) as e:
            ctx.match_map_binned_dev(**dict(job.kw, d_proj=None))
        assert e.value.status == abi.CLC_ERR_CAPACITY
        ctx.sync()
        assert (job.match.cpu().numpy() == -7).all()
    finally:
        ctx.close()

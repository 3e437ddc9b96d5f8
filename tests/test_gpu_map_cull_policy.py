"""The map cull behind the drop-in policy classes: HIPMatcher::observeMapDev -> cullMapDev -> HIPLocalizer::cullMapPoints ->
HIPMatcher::extendMapPairDev -> HIPLocalizer::appendMapPoints on one colocData, through a compiled driver
(tests/host/map_cull_policy_driver.cpp, g++ only, over the C ABI).  Afterwards the matcher's context, the localizer's context and the
host-side database agree: one row count, and row i's landmark id names the point both contexts hold at i; and all of it equals the
binding's result on the same data, exactly."""
import os
import subprocess

import numpy as np
import pytest

import guided_host as gh
import map_cull_host as ch
import map_extend_host as mh
import test_gpu_map_cull as tc
import test_gpu_map_extend as tme

pytestmark = pytest.mark.gpu

ROOT = tme.ROOT
N_OBSERVES = 8


def test_policy_members_keep_contexts_and_database_together(tmp_path):
    from coloc_amd import build
    lib = build.build()
    exe = str(tmp_path / "map_cull_policy_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "coloc_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "map_cull_policy_driver.cpp"), "-o", exe, "-L", os.path.dirname(lib), "-lcoloc_hip",
                           "-ldl", "-Wl,-rpath," + os.path.dirname(lib)])
    na, nb, nm, thr = 300, 320, tme.MAP_N, 40
    views, _ = mh.make_views([na, nb], seed=91, cams=[mh.CAM_K1, mh.CAM])
    a, b = views
    M, X = mh.make_map(nm, 1)
    # every second tracked landmark lies where view A (the identity pose) sees the keypoint that tracks it: found in every frame; the
    # others stay random points nothing near their projections tracks: visible, never found
    ud = gh.ud_positions(a["cam"], feat=a["feat"])
    planted = sorted(set(int(r) for r in a["track"] if r >= 0))[::2]
    for r in planted:
        q = int(np.nonzero(a["track"] == r)[0][0])
        X[r] = ((ud[q, 0] - a["cam"][1]) / a["cam"][0] * 10.0, (ud[q, 1] - a["cam"][2]) / a["cam"][0] * 10.0, 10.0)
    C_a, C_b = (0.0, 0.0, 0.0), (0.6, 0.0, 0.0)                                  # make_views' centres: Pose3(R, C) forms t = -R C as mh.pose does
    np.concatenate([a["cam"], a["Rt"][:, :3].reshape(-1), C_a, b["cam"], b["Rt"][:, :3].reshape(-1), C_b, [na, nb, nm, mh.BAND, thr, mh.CAP, N_OBSERVES],
                    X.reshape(-1)]).astype(np.float64).tofile(tmp_path / "extend.bin")
    np.concatenate([a["desc"].reshape(-1), b["desc"].reshape(-1), M.reshape(-1)]).tofile(tmp_path / "desc.bin")
    np.concatenate([a["feat"].reshape(-1), b["feat"].reshape(-1)]).astype(np.float32).tofile(tmp_path / "feat.bin")
    np.concatenate([a["track"], b["track"]]).astype(np.int32).tofile(tmp_path / "track.bin")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = np.fromfile(tmp_path / "out.bin", dtype=np.int32)
    rows_out = np.fromfile(tmp_path / "rows_out.bin", dtype=np.uint8).reshape(-1, 64)
    X_db, X_m, X_l = (np.fromfile(tmp_path / f, dtype=np.float64).reshape(-1, 3) for f in ("X_db.bin", "X_matcher.bin", "X_localizer.bin"))
    removed, n_added, n_dropped, rows, n_landmarks, n_regions, ctx_rows, in_order = [int(v) for v in out[:8]]
    # the three holders agree
    assert rows == n_landmarks == n_regions == ctx_rows == len(X_db) == len(X_m) == len(X_l) == len(rows_out) and in_order == 1
    assert np.array_equal(X_db.view(np.uint64), X_m.view(np.uint64)) and np.array_equal(X_db.view(np.uint64), X_l.view(np.uint64))
    # and they hold what the binding leaves on the same data, which is the statement
    ctx = tc._ctx(M, X)
    try:
        st = ch.Stats()
        ov = dict(cam=a["cam"], Rt=a["Rt"], feat=a["feat"], track=a["track"], count=None, width=640, height=480, gate=3.0, margin=0.0)
        for _ in range(N_OBSERVES):
            ch.observe(st, X, [ov])
            ctx.map_observe_dev(**tc._Obs(ov).kw)
        want = tc._cull(ctx, st, M, X, tc.RULE, None, [a["track"], b["track"]], "binding == statement")
        assert 5 <= want["n_kept"] < nm and want["n_ratio"] == removed == nm - want["n_kept"]
        assert set(np.nonzero(want["remap"] >= 0)[0]) >= set(planted)
        a2, b2 = dict(a, track=want["lists"][0]), dict(b, track=want["lists"][1])
        va, vb = tme._View(a2, stride=2), tme._View(b2, stride=2)
        ext = ctx.extend_map(va.kw, vb.kw, mh.BAND, thr, mh.CAP)
        tme._same(ext, mh.statement(a2, b2, mh.BAND, thr, mh.CAP, want["n_kept"], 4096), want["n_kept"], "binding == statement")
        n = ext["n_added"]
        assert n >= 5 and (n_added, n_dropped) == (n, ext["n_dropped"]) and rows == want["n_kept"] + n
        kept = np.nonzero(want["remap"] >= 0)[0]
        assert np.array_equal(out[8:8 + rows], np.concatenate([1000 + kept, 1000 + kept.max() + 1 + np.arange(n)]))   # the survivors' ids, then fresh ones
        assert np.array_equal(out[8 + rows:8 + rows + nm], want["remap"])
        assert np.array_equal(out[8 + rows + nm:8 + rows + nm + na], va.tracks()) and np.array_equal(out[8 + rows + nm + na:], vb.tracks())
        assert np.array_equal(rows_out, np.vstack([want["M"], a["desc"][ext["new_q"]]]))
        assert np.array_equal(X_db.view(np.uint64), np.vstack([want["X"], ext["X"]]).view(np.uint64))
    finally:
        ctx.close()

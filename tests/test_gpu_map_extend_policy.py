"""The map extension behind the drop-in policy classes: HIPMatcher::extendMapPairDev and HIPLocalizer::appendMapPoints through a
compiled driver (tests/host/map_extend_policy_driver.cpp, g++ only, over the C ABI).  What the member leaves in colocData -- mapRegions,
mapRegionIdx, the scene's landmarks -- and in the two d_track lists equals the binding's result on the same data, exactly."""
import os
import subprocess

import numpy as np
import pytest

import map_extend_host as mh
import test_gpu_map_extend as tme

pytestmark = pytest.mark.gpu

ROOT = tme.ROOT


def test_policy_member_leaves_the_entry_s_rows_in_colocdata(tmp_path):
    from coloc_amd import build
    lib = build.build()
    exe = str(tmp_path / "map_extend_policy_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "coloc_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "map_extend_policy_driver.cpp"), "-o", exe, "-L", os.path.dirname(lib), "-lcoloc_hip",
                           "-ldl", "-Wl,-rpath," + os.path.dirname(lib)])
    na, nb, nm, thr = 300, 320, tme.MAP_N, 40
    views, _ = mh.make_views([na, nb], seed=91, cams=[mh.CAM_K1, mh.CAM])
    a, b = views
    M, X = mh.make_map(nm, 1)
    C_a, C_b = (0.0, 0.0, 0.0), (0.6, 0.0, 0.0)                                  # make_views' centres: Pose3(R, C) forms t = -R C as mh.pose does
    np.concatenate([a["cam"], a["Rt"][:, :3].reshape(-1), C_a, b["cam"], b["Rt"][:, :3].reshape(-1), C_b, [na, nb, nm, mh.BAND, thr, mh.CAP],
                    X.reshape(-1)]).astype(np.float64).tofile(tmp_path / "extend.bin")
    np.concatenate([a["desc"].reshape(-1), b["desc"].reshape(-1), M.reshape(-1)]).tofile(tmp_path / "desc.bin")
    np.concatenate([a["feat"].reshape(-1), b["feat"].reshape(-1)]).astype(np.float32).tofile(tmp_path / "feat.bin")
    np.concatenate([a["track"], b["track"]]).astype(np.int32).tofile(tmp_path / "track.bin")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = np.fromfile(tmp_path / "out.bin", dtype=np.int32)
    rows = np.fromfile(tmp_path / "rows_out.bin", dtype=np.uint8).reshape(-1, 64)
    feat = np.fromfile(tmp_path / "feat_out.bin", dtype=np.float32).reshape(-1, 2)
    Xo = np.fromfile(tmp_path / "X_out.bin", dtype=np.float64).reshape(-1, 3)
    # the binding on the same data
    ctx, M2, X2 = tme._ctx(maxkp=4096)
    try:
        assert np.array_equal(M2, M) and np.array_equal(X2, X)
        va, vb = tme._View(a, stride=2), tme._View(b, stride=2)
        want = ctx.extend_map(va.kw, vb.kw, mh.BAND, thr, mh.CAP)
        tme._same(want, mh.statement(a, b, mh.BAND, thr, mh.CAP, nm, 4096), nm, "binding == statement")
        n = want["n_added"]
        assert n >= 5
        assert out[0] == n and out[1] == want["n_dropped"] and out[2] == nm + n
        assert np.array_equal(out[3:3 + nm + n], 1000 + np.arange(nm + n))       # fresh ids: one past the largest key, ascending
        assert np.array_equal(out[3 + nm + n:3 + nm + n + na], va.tracks()) and np.array_equal(out[3 + nm + n + na:], vb.tracks())
        assert np.array_equal(rows, np.vstack([M, a["desc"][want["new_q"]]]))
        assert np.array_equal(feat[nm:], a["feat"][want["new_q"]])
        assert np.array_equal(Xo.view(np.uint64), np.vstack([X, want["X"]]).view(np.uint64))
    finally:
        ctx.close()

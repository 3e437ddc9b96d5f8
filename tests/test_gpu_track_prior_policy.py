"""HIPLocalizer::localizeImagePriorDev (coloc_amd/host/HIPLocalizer.hpp: a tracked frame's pose from the prediction) through a C++ program,
against the binding of the same entry (Context.track_prior_dev) on the same frame, prior and gate: the same pose, covariance,
trackedFeatures and inliers, bit for bit; FEW is reported as failure with the pose left as it came in."""
import os
import subprocess

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_track_prior_driver(out):
    from coloc_amd import build
    lib = build.build()
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "coloc_amd", "host"),
           os.path.join(ROOT, "tests", "host", "track_prior_driver.cpp"), "-o", out, "-L", os.path.dirname(lib), "-lcoloc_hip", "-ldl",
           "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.check_call(cmd)
    return out


def test_track_prior_driver_compiles_and_links(tmp_path):
    assert os.path.exists(build_track_prior_driver(str(tmp_path / "track_prior_driver")))


def _distort(x, K, k):
    f, pp = K[0, 0], np.array([K[0, 2], K[1, 2]])
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


@pytest.mark.gpu
@pytest.mark.parametrize("kd", [(-0.12, 0.05, -0.01), (0.0, 0.0, 0.0)])
def test_policy_member_leaves_what_the_binding_leaves(tmp_path, kd):
    import pose_prior_cases as pc
    from test_gpu_track_localize import _bits, _dev, _light_ctx
    exe = build_track_prior_driver(str(tmp_path / "track_prior_driver"))
    sc = synth.pnp_scene(700, seed=4321, outlier_frac=0.3)
    K, kd = sc["K"], np.array(kd)
    rng = np.random.default_rng(5)
    n_map, n_feat, n = 900, 1500, 700
    map_rows = rng.choice(n_map, n, replace=False)
    feat_rows = rng.choice(n_feat, n, replace=False)
    mapX = rng.uniform(-5, 5, (n_map, 3)) + [0, 0, 12]
    mapX[map_rows] = sc["X"]
    feats = np.stack([rng.uniform(0, 1280, n_feat), rng.uniform(0, 720, n_feat)], 1)
    feats[feat_rows] = _distort(sc["x"], K, kd)
    feats = feats.astype(np.float32).astype(np.float64)
    head = [1280, 720, K[0, 0], K[0, 2], K[1, 2], kd[0], kd[1], kd[2], n_map, n_feat, n]
    np.concatenate([head, mapX.reshape(-1), feats.reshape(-1), np.stack([map_rows, feat_rows], 1).reshape(-1)]).astype(np.float64).tofile(
        tmp_path / "loc.bin")
    Rt_true = np.concatenate([sc["R"], np.asarray(sc["t"]).reshape(3, 1)], 1)
    prior, gate = pc.perturbed(Rt_true, 11), 3.0
    np.concatenate([prior.reshape(-1), [gate]]).astype(np.float64).tofile(tmp_path / "prior.bin")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    o = np.fromfile(tmp_path / "prior_out.bin", dtype=np.float64)
    # the binding on the same frame, from the prior as the member read it back from its Pose3 (R, C): t = -R C differs from the t that
    # made C in the last bits, and the solve's iterates follow their start
    prior_read = o[52:64].reshape(3, 4)
    assert np.array_equal(prior_read[:, :3], prior[:, :3]) and np.abs(prior_read[:, 3] - prior[:, 3]).max() < 1e-12
    match = np.full(n_feat, -1, dtype=np.int32)
    match[feat_rows] = map_rows
    feat4 = np.zeros((n_feat, 4), dtype=np.float32)
    feat4[:, :2] = feats
    feat4[:, 2] = 7.0
    cam = (K[0, 0], K[0, 2], K[1, 2]) + tuple(kd)
    ctx = _light_ctx()
    try:
        ctx.set_map_points(mapX)
        d_match, d_feat = _dev(match), _dev(feat4)
        want = ctx.track_prior_dev(d_match=d_match.data_ptr(), nq=n_feat, cam=cam, d_feat=d_feat.data_ptr(), feat_stride=4, Rt_prior=prior_read,
                                   gate=gate, huber_a=16.0)
    finally:
        ctx.close()
    assert want["result"] == 0 and want["n_tracks"] == n and want["n_inliers"] > 0.6 * n
    assert o[0] == 0.0 and int(o[1]) == n and int(o[2]) == want["n_inliers"] and 0.2 < o[3] < 1.5      # false = success
    R, C, cov, inl = o[4:13].reshape(3, 3), o[13:16], o[16:52].reshape(6, 6), o[64:].astype(np.int64)
    assert np.array_equal(_bits(R), _bits(want["Rt"][:, :3]))
    Rw, tw = want["Rt"][:, :3], want["Rt"][:, 3]
    Cw = np.array([-(Rw[0, i] * tw[0] + Rw[1, i] * tw[1] + Rw[2, i] * tw[2]) for i in range(3)])         # Pose3(R, -R^T t), the member's order
    assert np.array_equal(_bits(C), _bits(Cw))
    assert np.array_equal(_bits(cov), _bits(want["cov"]))
    assert np.array_equal(inl, np.flatnonzero(want["mask"]))
    assert np.linalg.norm(C + sc["R"].T @ sc["t"]) < 0.02

"""HIPLocalizer::localizeImageDev (coloc_amd/host/HIPLocalizer.hpp: tracks built on the device) through a C++ program, against
setupTracks + localizeImage on the same frame and seed: the same pose, covariance, rmse, trackedFeatures and inliers, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_track_driver(out):
    from coloc_amd import build
    lib = build.build()
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "coloc_amd", "host"),
           os.path.join(ROOT, "tests", "host", "track_localizer_driver.cpp"), "-o", out, "-L", os.path.dirname(lib), "-lcoloc_hip", "-ldl",
           "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.check_call(cmd)
    return out


def test_track_driver_compiles_and_links(tmp_path):
    assert os.path.exists(build_track_driver(str(tmp_path / "track_localizer_driver")))


def _distort(x, K, k):
    f, pp = K[0, 0], np.array([K[0, 2], K[1, 2]])
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


@pytest.mark.gpu
@pytest.mark.parametrize("kd", [(-0.12, 0.05, -0.01), (0.0, 0.0, 0.0)])
def test_policy_member_leaves_what_localize_image_leaves(tmp_path, kd):
    exe = build_track_driver(str(tmp_path / "track_localizer_driver"))
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
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    o = np.fromfile(tmp_path / "track_out.bin", dtype=np.float64)
    assert o[0] == 0.0 and int(o[1]) == n and int(o[2]) > 0.6 * n and 0.2 < o[3] < 1.5      # false = success; a real localisation
    assert np.linalg.norm(o[4:7] + sc["R"].T @ sc["t"]) < 0.02

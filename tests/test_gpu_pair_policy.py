"""HIPRobustMatcher::filterMatchesPairDev (coloc_amd/host/HIPRobustMatcher.hpp: correspondences built on the device) through a C++
program, against filterMatchesPair on the same matches and seed, under all three models: the same geometricMatches and relativePoses
(vec_inliers, essential_matrix, found_residual_precision, the relative pose), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import twoview_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_pair_driver(out):
    from coloc_amd import build
    lib = build.build()
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "coloc_amd", "host"),
           os.path.join(ROOT, "tests", "host", "pair_policy_driver.cpp"), "-o", out, "-L", os.path.dirname(lib), "-lcoloc_hip", "-ldl",
           "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.check_call(cmd)
    return out


def test_pair_driver_compiles_and_links(tmp_path):
    assert os.path.exists(build_pair_driver(str(tmp_path / "pair_policy_driver")))


def _distort(x, cam):
    f, pp, k = cam[0], np.array(cam[1:3]), cam[3:6]
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["E", "F", "H"])
def test_policy_member_leaves_what_filter_matches_pair_leaves(tmp_path, model):
    exe = build_pair_driver(str(tmp_path / "pair_policy_driver"))
    n, nq, nt = 700, 1200, 1000
    sc = twoview_host.scene(n, 8100 + ord(model), planar=(model == "H"))
    K = sc["K"]
    camA = (K[0, 0], K[0, 2], K[1, 2], -0.12, 0.05, -0.01)
    camB = (K[0, 0], K[0, 2], K[1, 2], 0.08, -0.02, 0.0)
    rng = np.random.default_rng(9)
    qs, rows = np.sort(rng.choice(nq, n, replace=False)), rng.choice(nt, n, replace=False)
    featA = np.stack([rng.uniform(0, 1280, nq), rng.uniform(0, 720, nq)], 1)
    featB = np.stack([rng.uniform(0, 1280, nt), rng.uniform(0, 720, nt)], 1)
    featA[qs], featB[rows] = _distort(sc["x1"], camA), _distort(sc["x2"], camB)
    featA, featB = featA.astype(np.float32).astype(np.float64), featB.astype(np.float32).astype(np.float64)
    match = np.full(nq, -1.0)
    match[qs] = rows
    head = [1280, 720, *camA, *camB, ord(model), nq, nt]
    np.concatenate([head, featA.reshape(-1), featB.reshape(-1), match]).astype(np.float64).tofile(tmp_path / "pair.bin")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    o = np.fromfile(tmp_path / "pair_out.bin", dtype=np.float64)
    assert o[0] == 0.0 and int(o[1]) == n and int(o[2]) > 0.55 * n                     # false = success; a real model
    if model == "E":
        assert np.abs(o[3:12].reshape(3, 3) - sc["R"]).max() < 0.05                    # the scene's rotation (X2 = R X1 + t)

"""HIPRobustMatcher::matchMapsSimilarity (coloc_amd/host/HIPRobustMatcher.hpp; our own statement) driven through a C++
program, checked against the Python binding of the same C ABI (same seed: the same inliers, the same s, R, t) and against the scene."""
import subprocess

import numpy as np
import pytest

import sim3_cases
from test_policy_host import build_driver

pytestmark = pytest.mark.gpu


def _run(exe, tmp_path, old_X, new_X, ci, cj):
    np.concatenate([[len(old_X), len(new_X), len(ci)], old_X.reshape(-1), new_X.reshape(-1), ci, cj]).astype(np.float64).tofile(tmp_path / "maps.bin")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    o = np.fromfile(tmp_path / "maps_out.bin", dtype=np.float64)
    n = int(o[14])
    return dict(status=o[0], s=o[1], R=o[2:11].reshape(3, 3), t=o[11:14], left=o[15:15 + 2 * n].reshape(n, 2).astype(np.int64))


def test_match_maps_similarity_keeps_the_inliers(tmp_path, gpu_ctx):
    exe = build_driver(str(tmp_path / "match_maps_sim_driver"), "match_maps_sim_driver.cpp")
    sc = sim3_cases.planted_scene(200, 0.3, 41)
    rng = np.random.default_rng(42)
    # the two maps hold the pairs' landmarks at shuffled rows, among rows no common feature names; two matches name no landmark at all
    old_rows, new_rows = rng.permutation(260)[:200], rng.permutation(240)[:200]
    old_X, new_X = rng.uniform(-50, 50, (260, 3)), rng.uniform(-50, 50, (240, 3))
    old_X[old_rows], new_X[new_rows] = sc["y"], sc["x"]
    ci, cj = np.concatenate([old_rows, [260, 5]]), np.concatenate([new_rows, [3, 240]])
    got = _run(exe, tmp_path, old_X, new_X, ci, cj)
    ref = gpu_ctx.sim3_acransac(sc["x"], sc["y"], max_iteration=256, seed=1)             # the member's first seed
    assert ref["found"] and np.array_equal(ref["mask"], sc["planted"])
    assert got["status"] == 0.0                                                          # EXIT_SUCCESS through bool
    keep = np.nonzero(ref["mask"])[0]
    assert np.array_equal(got["left"], np.stack([old_rows[keep], new_rows[keep]], 1))    # only the inliers, in their order
    assert got["s"] == ref["s"] and np.array_equal(got["R"], ref["R"]) and np.array_equal(got["t"], ref["t"])
    assert abs(got["s"] - 2.5) < 1e-12 and np.allclose(got["R"], sc["R"], atol=1e-12)
    # nothing to find: EXIT_FAILURE, no common feature left, the identity
    got = _run(exe, tmp_path, rng.uniform(-10, 10, (40, 3)), rng.uniform(-10, 10, (40, 3)), np.arange(40), np.arange(40))
    assert got["status"] == 1.0 and len(got["left"]) == 0 and got["s"] == 1.0 and np.array_equal(got["R"], np.eye(3)) and not got["t"].any()

"""HIPRatioMatcher<bool> driven the way ColoC's non-CUDA build drives CPUMatcher (C++ driver tests/host/ratio_policy_driver.cpp) on the
GPU: computeMatches over three cameras, computeMatchesPair, matchMapFeatures and matchSceneWithMap, each equal to the oracle's
CPUMatcher pairs (orc_cpumatcher_pair: database = first set, queries = second, IndMatch(i_ = database row, j_ = query row))."""
import subprocess

import numpy as np
import pytest

from test_gpu_ratio_match import cameras
from test_policy_host import build_driver

pytestmark = pytest.mark.gpu


def _pairs_from(path):
    return np.fromfile(path, dtype=np.uint32).reshape(-1, 2).astype(np.int64)


def test_ratio_policy_class_end_to_end(tmp_path, oracle):
    exe = build_driver(str(tmp_path / "ratio_policy_driver"), "ratio_policy_driver.cpp")
    descs, xys = cameras((1500, 1200, 0), seed=60)                    # camera 2 has no regions
    for c, (d, xy) in enumerate(zip(descs, xys)):
        d.tofile(str(tmp_path / ("desc%d.bin" % c)))
        xy.astype(np.float32).tofile(str(tmp_path / ("xy%d.bin" % c)))
    out = subprocess.run([exe, str(tmp_path), "3", "4000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    rc = dict(line.split(" ", 1) for line in (tmp_path / "rc.txt").read_text().splitlines())
    assert rc["computeMatches"] == "0" and rc["computeMatchesPair"] == "0" and rc["computeMatchesPair06"] == "0"
    assert rc["matchMapFeatures"] == "0" and rc["matchSceneWithMap"] == "0"

    def want(i, j, ratio=0.8):
        return oracle.cpumatcher_pair(descs[i], xys[i], descs[j], xys[j], ratio=ratio)[0].astype(np.int64)

    n_with = 0
    for i in range(3):
        for j in range(i + 1, 3):
            w = want(i, j)
            path = tmp_path / ("pair_%d_%d.bin" % (i, j))
            if len(w) == 0:
                assert not path.exists()                 # empty results are not inserted (CPUMatcher.hpp:44-50)
                continue
            n_with += 1
            assert np.array_equal(_pairs_from(path), w), (i, j)
    assert n_with == 1 and (tmp_path / "pair_0_1.bin").exists()         # camera 2 has no regions: its pairs are empty
    assert np.array_equal(_pairs_from(tmp_path / "single_0_1.bin"), want(0, 1))
    assert np.array_equal(_pairs_from(tmp_path / "single06_0_1.bin"), want(0, 1, 0.6))
    assert len(want(0, 1, 0.6)) < len(want(0, 1))
    assert np.array_equal(_pairs_from(tmp_path / "mapmap_0_1.bin"), want(0, 1))
    # map tracking: the map (camera 0's regions) is the database, camera 1 the queries
    assert np.array_equal(_pairs_from(tmp_path / "map_1.bin"), want(0, 1))
    # camera 2 has no regions: empty lists with EXIT_SUCCESS, as CPUMatcher; map tracking finds nothing -> EXIT_FAILURE
    assert rc["matchSceneWithMapEmpty"] == "1 0"
    assert rc["computeMatchesPairEmpty"] == "0 0" and rc["computeMatchesPairEmptyDb"] == "0 0" and rc["matchMapFeaturesEmpty"] == "0 0"

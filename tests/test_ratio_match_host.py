"""The distance-ratio matcher (CPUMatcher's rule, include/coloc_hip.h clc_match_ratio_*) without a GPU: the entry points are declared
and exported, the host half -- per-query ratio results -> CPUMatcher's de-duplicated, ordered IndMatch list
(clc_ratio_matches_to_pairs) -- equals the oracle's orc_cpumatcher_pair, and coloc_amd/host/HIPRatioMatcher.hpp compiles stand-alone
with CPUMatcher's member signatures.  The GPU half is tests/test_gpu_ratio_match.py / test_gpu_ratio_policy.py."""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_match_ratio_2nn", "clc_match_ratio_2nn_dev", "clc_match_ratio_pairs", "clc_match_map_ratio",
               "clc_match_map_ratio_dev", "clc_ratio_matches_to_pairs"]


def ratio_scene(n_db, n_q, seed):
    """(D, xy_db, Q, xy_q): database / query descriptors (half the queries near-duplicates of database rows) and positions with planted
    repeats -- queries that are copies of other queries at the same position (same database row, same (x, y) pair: dropped by the
    position pass), database rows sharing a position, query rows sharing a position, and positions on an integer grid."""
    rng = np.random.default_rng(seed)
    Q, D = synth.planted_descriptors(n_q, n_db, seed=seed, frac=0.5, max_flip=40)
    xy_db = rng.integers(0, 64, size=(n_db, 2)).astype(np.float32)
    xy_q = rng.uniform(0, 640, size=(n_q, 2)).astype(np.float32)
    if n_db >= 8 and n_q >= 8:
        k = n_q // 8
        src = rng.choice(n_q, size=k, replace=False)
        dst = rng.choice(np.setdiff1d(np.arange(n_q), src), size=k, replace=False)
        Q[dst] = Q[src]                                       # identical queries -> identical matches ...
        xy_q[dst] = xy_q[src]                                 # ... at identical positions
        a = rng.choice(n_db, size=n_db // 8, replace=False)
        xy_db[a] = xy_db[rng.choice(n_db, size=a.size)]       # database rows sharing a position
        b = rng.choice(n_q, size=n_q // 8, replace=False)
        xy_q[b] = xy_q[rng.choice(n_q, size=b.size)]          # query rows sharing a position
    return D, xy_db, Q, xy_q


def pairs_without_positions(m):
    """the ratio-only form: accepted (i_ = database row, j_ = query row) in ascending (i_, j_)"""
    j = np.nonzero(m >= 0)[0]
    p = np.stack([m[j], j], 1).astype(np.int32).reshape(-1, 2)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


def _declared():
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(clc_[a-z0-9_]+)\s*\(", hdr))


def test_ratio_entries_are_declared_and_exported():
    from coloc_amd import abi
    lib = abi.load_library()
    assert set(NEW_ENTRIES) <= _declared()
    assert set(NEW_ENTRIES) <= set(abi.EXPORTS)
    for n in NEW_ENTRIES:
        assert hasattr(lib, n), "missing export " + n
    assert lib.clc_abi_version() == 4


@pytest.mark.parametrize("ratio", [0.6, 0.8, 1.0, 1.25])
@pytest.mark.parametrize("n_db,n_q,seed", [(2, 1, 1), (40, 60, 2), (500, 700, 3), (3000, 2000, 4)])
def test_pair_list_equals_cpumatcher_oracle(oracle, ratio, n_db, n_q, seed):
    from coloc_amd import ratio_matches_to_pairs
    D, xy_db, Q, xy_q = ratio_scene(n_db, n_q, seed)
    m, _ = oracle.k2nn_omp(Q, D, rule=1, ratio=ratio)
    want, _ = oracle.cpumatcher_pair(D, xy_db, Q, xy_q, ratio=ratio)
    got = ratio_matches_to_pairs(m, xy_db, xy_q)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)                          # order included: (x_I, y_I, x_J, y_J, i_, j_)
    assert np.array_equal(ratio_matches_to_pairs(m), pairs_without_positions(m))


def test_planted_repeats_are_dropped(oracle):
    """the scene exercises the position pass: fewer pairs than accepted queries, and no two kept pairs share all four coordinates"""
    from coloc_amd import ratio_matches_to_pairs
    D, xy_db, Q, xy_q = ratio_scene(2000, 3000, 7)
    m, _ = oracle.k2nn_omp(Q, D, rule=1, ratio=0.8)
    got = ratio_matches_to_pairs(m, xy_db, xy_q)
    assert 200 < len(got) < int((m >= 0).sum()) - 50
    coords = np.concatenate([xy_db[got[:, 0]], xy_q[got[:, 1]]], 1)
    assert len(np.unique(coords, axis=0)) == len(got)
    assert len(ratio_matches_to_pairs(m)) == int((m >= 0).sum())      # without positions only identical pairs go, and there are none


def test_pair_list_edge_cases_and_errors():
    from coloc_amd import abi, ratio_matches_to_pairs
    lib = abi.load_library()
    assert ratio_matches_to_pairs(np.zeros(0, np.int32)).shape == (0, 2)
    assert ratio_matches_to_pairs(np.full(5, -1, np.int32), np.zeros((3, 2)), np.zeros((5, 2))).shape == (0, 2)
    # every query on database row 0 at one position: one pair survives the position pass, all five without positions
    m = np.zeros(5, np.int32)
    assert np.array_equal(ratio_matches_to_pairs(m, np.zeros((1, 2)), np.zeros((5, 2))), [[0, 0]])
    assert np.array_equal(ratio_matches_to_pairs(m), [[0, j] for j in range(5)])
    out = np.zeros((5, 2), np.int32)
    n = C.c_int(-1)
    xy = np.zeros((5, 2), np.float32)
    rc = lib.clc_ratio_matches_to_pairs(m.ctypes.data, 5, xy.ctypes.data, None, out.ctypes.data, C.byref(n))
    assert rc == 1 and n.value == 0                           # positions for one side only
    rc = lib.clc_ratio_matches_to_pairs(m.ctypes.data, 5, None, xy.ctypes.data, out.ctypes.data, C.byref(n))
    assert rc == 1
    # no query rows: nothing to order, so no positions are needed on either side (an empty camera's position array may be NULL)
    for a, b in ((None, None), (xy.ctypes.data, None), (None, xy.ctypes.data)):
        n.value = -1
        assert lib.clc_ratio_matches_to_pairs(m.ctypes.data, 0, a, b, out.ctypes.data, C.byref(n)) == 0 and n.value == 0
    assert ratio_matches_to_pairs(np.zeros(0, np.int32), np.zeros((3, 2))).shape == (0, 2)
    xy[2, 1] = np.nan
    assert lib.clc_ratio_matches_to_pairs(m.ctypes.data, 5, xy.ctypes.data, xy.ctypes.data, out.ctypes.data, C.byref(n)) == 1
    assert lib.clc_ratio_matches_to_pairs(m.ctypes.data, -1, None, None, out.ctypes.data, C.byref(n)) == 1
    assert lib.clc_ratio_matches_to_pairs(m.ctypes.data, 5, None, None, out.ctypes.data, None) == 1
    # the context entries check their arguments before touching a device
    q = np.zeros((4, 64), np.uint8)
    mm = np.zeros(4, np.int32)
    assert lib.clc_match_ratio_2nn(None, q.ctypes.data, 4, q.ctypes.data, 4, C.c_float(0.8), mm.ctypes.data, None, None) == 1
    assert lib.clc_match_ratio_2nn_dev(None, None, 0, None, 0, C.c_float(0.8), None, None) == 1
    assert lib.clc_match_map_ratio_dev(None, None, 0, C.c_float(0.8), None, None) == 1


def test_pair_list_is_n_log_n():
    """the de-duplication is a sort over the accepted matches: 8x the matches costs ~9x the time (a pairwise pass: 64x).  The two sizes
    are timed alternately, best of five each, so that a loaded host slows both alike."""
    from coloc_amd import ratio_matches_to_pairs
    rng = np.random.default_rng(5)

    def case(n):
        m = rng.integers(0, 1000, size=n).astype(np.int32)
        return m, rng.integers(0, 32, size=(1000, 2)).astype(np.float32), rng.integers(0, 32, size=(n, 2)).astype(np.float32)

    small, big = case(50000), case(400000)
    best = {50000: 1e9, 400000: 1e9}
    for _ in range(5):
        for m, xy_db, xy_q in (small, big):
            t0 = time.perf_counter()
            got = ratio_matches_to_pairs(m, xy_db, xy_q)
            best[m.shape[0]] = min(best[m.shape[0]], time.perf_counter() - t0)
    assert best[400000] < 24 * best[50000], best
    m, xy_db, xy_q = big
    assert len(got) == len(np.unique(np.concatenate([xy_db[m], xy_q], 1), axis=0))


SIGNATURES = r"""
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>
#include "HIPRatioMatcher.hpp"
using namespace openMVG;
using namespace openMVG::matching;
using M = coloc::HIPRatioMatcher<bool>;
// include/coloc/CPUMatcher.hpp:32-100, member for member
static_assert(std::is_constructible<M, coloc::MatcherOptions&>::value, "CPUMatcher(MatcherOptions&)");
static_assert(std::is_same<decltype(&M::computeMatches), bool (M::*)(coloc::FeatureMap&, PairWiseMatches&)>::value, "computeMatches");
static_assert(std::is_same<decltype(&M::matchMapFeatures),
                           bool (M::*)(std::unique_ptr<features::AKAZE_Binary_Regions>&, std::unique_ptr<features::AKAZE_Binary_Regions>&,
                                       std::vector<IndMatch>&)>::value, "matchMapFeatures");
static_assert(std::is_same<decltype(&M::computeMatchesPair), bool (M::*)(const Pair&, coloc::FeatureMap&, IndMatches&, float)>::value,
              "computeMatchesPair");
static_assert(std::is_same<decltype(&M::matchSceneWithMap), bool (M::*)(unsigned int, coloc::colocData&, IndMatches&)>::value,
              "matchSceneWithMap");
static_assert(std::is_same<decltype(&M::setMapData), void (M::*)(int, void*)>::value, "setMapData");
// distRatio defaults to 0.8f (CPUMatcher.hpp:67)
static_assert(std::is_same<decltype(std::declval<M&>().computeMatchesPair(std::declval<const Pair&>(), std::declval<coloc::FeatureMap&>(),
                                                                           std::declval<IndMatches&>())), bool>::value, "default distRatio");
template class coloc::HIPRatioMatcher<bool>;
int main() { return 0; }
"""


def test_policy_header_compiles_with_cpumatcher_signatures(tmp_path):
    src = tmp_path / "ratio_signatures.cpp"
    src.write_text(SIGNATURES)
    cmd = ["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "coloc_amd", "host"), str(src)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    hdr = open(os.path.join(ROOT, "coloc_amd", "host", "HIPRatioMatcher.hpp")).read()
    assert "static_assert(CLC_ABI_VERSION >= 4" in hdr
    assert "GetRegionsPositions()" in hdr

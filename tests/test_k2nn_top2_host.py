"""The top-2 network of the matrix sweep (coloc_amd/csrc/k2nn_top2.h: triples, three-pair merges, top2_fold16) through its host build
(tests/host/k2nn_top2_lib.cpp) against a sort.  Keys are the bits of positive finite floats or of +inf; the network works on the bits as
unsigned integers, the reference sorts them as unsigned integers too and, where the keys are accumulator values, as floats as well."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 0x7F800000
MAGIC = 0x4B000000            # bits of 2^23: accumulator = 2^23 + (distance << 13) + index
_LIB = []


def lib():
    if not _LIB:
        out = os.path.join(ROOT, "tests", "host", "libk2nn_top2_host.so")
        src = os.path.join(ROOT, "tests", "host", "k2nn_top2_lib.cpp")
        hdr = os.path.join(ROOT, "coloc_amd", "csrc", "k2nn_top2.h")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        l = C.CDLL(out)
        l.k2nn_top2_host_step_back.restype = C.c_uint32
        l.k2nn_top2_host_step_back.argtypes = [C.c_uint32]
        _LIB.append(l)
    return _LIB[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def fold16(keys, pair):
    """keys n x 16, pair n x 2 (best, second) -> the pairs behind the fold"""
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 16)
    out = np.ascontiguousarray(pair, dtype=np.uint32).reshape(-1, 2).copy()
    assert len(out) == len(keys)
    lib().k2nn_top2_host_fold16(_p(keys), _p(out), C.c_int(len(keys)))
    return out


def two_smallest(all18):
    """n x m -> n x 2, by a sort of the unsigned values"""
    return np.sort(np.asarray(all18, dtype=np.uint32), axis=1)[:, :2]


def test_parts_against_a_sort():
    rng = np.random.default_rng(1)
    vals = [1, 2, 3, 7, 7, INF, INF]
    for k in itertools.product(vals, repeat=3):
        out = np.zeros(2, np.uint32)
        lib().k2nn_top2_host_triple(_p(np.array(k, np.uint32)), _p(out))
        assert tuple(out) == tuple(sorted(k)[:2]), k
    for _ in range(20000):
        p = np.sort(rng.integers(1, 12, size=(3, 2)), axis=1).astype(np.uint32)      # three sorted pairs, ties allowed
        p[rng.random((3, 2)) < 0.1] = INF
        p = np.sort(p, axis=1)
        out = np.zeros(2, np.uint32)
        lib().k2nn_top2_host_merge3(_p(np.ascontiguousarray(p.reshape(6))), _p(out))
        assert tuple(out) == tuple(np.sort(p.reshape(6))[:2]), p


def test_every_placement_of_the_two_smallest():
    """18 inputs = 16 keys + the running pair (slots 16, 17); the smallest at slot i, the second smallest at slot j, 18 x 17 cases.  The
    running pair of the sweep is sorted (best <= second): for the placements that respect that, the result is held to (smallest, second
    smallest) in this order.  The others (the smallest in the `second` slot, or the second smallest there without the smallest in `best`)
    cannot occur in the sweep; the network still keeps the right two VALUES, which is what is asserted for them."""
    rng = np.random.default_rng(2)
    cases, valid = [], []
    for i, j in itertools.permutations(range(18), 2):
        v = rng.permutation(np.arange(100, 116)).astype(np.uint32)          # the sixteen others, distinct
        a = np.zeros(18, np.uint32)
        a[[k for k in range(18) if k not in (i, j)]] = v
        a[i], a[j] = 10, 20
        if i < 16 and j < 16:
            a[16:] = np.sort(a[16:])
        cases.append(a)
        valid.append(a[16] <= a[17])
    a = np.array(cases)
    assert len(a) == 18 * 17
    got = fold16(a[:, :16], a[:, 16:])
    valid = np.array(valid)
    assert valid.sum() == 16 * 15 + 2 * 16 + 1                              # both among the keys; one in `best`, one a key; (best, second)
    np.testing.assert_array_equal(got[valid], np.tile(np.array([10, 20], np.uint32), (int(valid.sum()), 1)))
    np.testing.assert_array_equal(np.sort(got, axis=1), np.tile(np.array([10, 20], np.uint32), (len(a), 1)))


def test_random_orders_of_distinct_keys():
    rng = np.random.default_rng(3)
    n = 10000
    a = np.array([rng.choice(1 << 20, size=18, replace=False) + 1 for _ in range(n)], dtype=np.uint32)
    a[:, 16:] = np.sort(a[:, 16:], axis=1)
    np.testing.assert_array_equal(fold16(a[:, :16], a[:, 16:]), two_smallest(a))


@pytest.mark.parametrize("n_inf", [1, 2, 15, 16, 18])
def test_repeated_inf(n_inf):
    rng = np.random.default_rng(100 + n_inf)
    cases = []
    for _ in range(400):
        a = (rng.choice(1 << 20, size=18, replace=False) + 1).astype(np.uint32)
        a[rng.choice(18, size=n_inf, replace=False)] = INF
        a[16:] = np.sort(a[16:])
        cases.append(a)
    a = np.array(cases)
    want = two_smallest(a)
    if n_inf >= 17:
        assert (want == INF).all()
    np.testing.assert_array_equal(fold16(a[:, :16], a[:, 16:]), want)


def _acc_bits(d, index):
    """bits of the accumulator 2^23 + (d << 13) + index (index may be negative: a stepped-back value), through the float VALUE"""
    v = (8388608.0 + np.asarray(d, np.float64) * 8192.0 + np.asarray(index, np.float64)).astype(np.float32)
    return v.view(np.uint32)


def test_accumulator_range():
    """keys 0x4B000000 + (d << 13) + index for d in 0 .. 512, running pairs that have stepped back (index field negative; with distance 0
    their value lies below 2^23, where the bits are no longer magic + integer): the unsigned order of the bits is the order of the values"""
    rng = np.random.default_rng(4)
    n = 4000
    d = rng.integers(0, 513, size=(n, 18))
    d[: n // 4] = rng.integers(0, 3, size=(n // 4, 18))                    # many at distance 0 .. 2
    d[n // 4: n // 2, :] = 512
    idx = np.array([rng.permutation(32)[:16] for _ in range(n)])           # distinct rows of the tile
    back = -np.array([rng.choice(8192, size=2, replace=False) + 1 for _ in range(n)])   # the pair: distinct rows behind the tile
    keys = _acc_bits(d[:, :16], idx)
    assert (keys == MAGIC + (d[:, :16] << 13) + idx).all()
    pair = np.sort(_acc_bits(d[:, 16:], back), axis=1)
    assert (pair.view(np.float32) < 8388608.0).any() and (pair < MAGIC).any()
    allk = np.concatenate([keys, pair], axis=1)
    want = two_smallest(allk)
    np.testing.assert_array_equal(want.view(np.float32), np.sort(allk.view(np.float32), axis=1)[:, :2])   # bits order == float order
    np.testing.assert_array_equal(fold16(keys, pair), want)
    some_inf = pair.copy()
    some_inf[::2, 1] = INF
    some_inf[::4, 0] = INF
    np.testing.assert_array_equal(fold16(keys, some_inf), two_smallest(np.concatenate([keys, some_inf], axis=1)))


def test_step_back():
    for bits, want in ((INF, INF), (MAGIC + 40, MAGIC + 8), (MAGIC + 5, int(np.float32(8388608.0 + 5 - 32).view(np.uint32)))):
        assert lib().k2nn_top2_host_step_back(bits) == want


def test_chained_folds_with_the_step_back():
    """eight consecutive folds (eight tiles of a lane's sixteen rows), the pair stepping back by 32 behind each, from (+inf, +inf): against
    a sort of all 128 keys with their index relative to the row behind the last tile"""
    rng = np.random.default_rng(5)
    n, chains = 500, 8
    d = rng.integers(0, 513, size=(n, chains, 16))
    d[: n // 5] = rng.integers(0, 2, size=(n // 5, chains, 16))            # ties in the distance everywhere: the index decides
    idx = np.array([[np.sort(rng.permutation(32)[:16]) for _ in range(chains)] for _ in range(n)])
    keys = _acc_bits(d, idx)
    pad = rng.random((n, chains, 16)) < 0.05
    keys[pad] = INF
    pair = np.full((n, 2), INF, np.uint32)
    lib().k2nn_top2_host_chain(_p(np.ascontiguousarray(keys)), _p(pair), C.c_int(n), C.c_int(chains))
    rel = idx - 32 * (chains - np.arange(chains))[None, :, None]           # -(rows behind) .. -1
    final = _acc_bits(d, rel)
    final[pad] = INF
    np.testing.assert_array_equal(pair, two_smallest(final.reshape(n, chains * 16)))

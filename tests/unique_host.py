"""The one-to-one filter on the host (include/coloc_hip.h, clc_match_unique_dev): the rule in numpy, sequential, sharing no code with the
product, and the g++ build of coloc_amd/csrc/unique_math.h (tests/host/unique_lib.cpp) it is held to.  Also the three-camera recipe with
planted doubles that shows what the filter buys the tracks builder (tests/map_host.py::build_tracks)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
MAX_DIST, SHIFT, MAX_ROWS = 512, 22, 1 << 22


def unique(match, best, nt):
    """-> (match one-to-one, owner (nt,)), both int32: entry q claims row t = match[q] iff 0 <= t < nt and best[q] <= 512; a row goes to
    the claimant with the smallest (best, q); every other entry is -1"""
    match, best = np.asarray(match, dtype=np.int64), np.asarray(best, dtype=np.int64)
    held = {}                                                             # row -> (best, q) of its holder so far
    for q in range(len(match)):
        t = int(match[q])
        if 0 <= t < nt and best[q] <= MAX_DIST and (t not in held or (int(best[q]), q) < held[t]):
            held[t] = (int(best[q]), q)
    out, owner = np.full(len(match), -1, dtype=np.int32), np.full(nt, -1, dtype=np.int32)
    for t, (_, q) in held.items():
        out[q], owner[t] = t, q
    return out, owner


def key(best, q):
    return (np.asarray(best, dtype=np.uint64) << np.uint64(SHIFT)) | np.asarray(q, dtype=np.uint64)


# ---- the g++ build of unique_math.h -----------------------------------------------------------------------------------------------------
def lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "tests", "host", "libunique_host.so")
        src = os.path.join(ROOT, "tests", "host", "unique_lib.cpp")
        hdrs = [os.path.join(ROOT, "coloc_amd", "csrc", h) for h in ("unique_math.h", "guided_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", src, "-o", out])
        _LIB = C.CDLL(out)
        _LIB.unique_host_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _LIB.unique_host_claims.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _LIB.unique_host_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def cxx_keys(best, q):
    """(unique_key, unique_holder_of(unique_key)) of every (best, q)"""
    best, q = np.ascontiguousarray(best, dtype=np.uint32), np.ascontiguousarray(q, dtype=np.uint32)
    k, h = np.zeros(len(best), dtype=np.uint32), np.zeros(len(best), dtype=np.int32)
    lib().unique_host_keys(_p(best), _p(q), len(best), _p(k), _p(h))
    return k, h


def cxx_claims(match, best, nt):
    match, best = np.ascontiguousarray(match, dtype=np.int32), np.ascontiguousarray(best, dtype=np.uint16)
    out = np.zeros(len(match), dtype=np.uint8)
    lib().unique_host_claims(_p(match), _p(best), len(match), int(nt), _p(out))
    return out.astype(bool)


def cxx_unique(match, best, nt):
    """the filter as the two kernels run it -- arm, fold the claims' keys by minimum, resolve -- over unique_math.h's statements"""
    m, best = np.array(match, dtype=np.int32), np.ascontiguousarray(best, dtype=np.uint16)
    owner = np.zeros(nt, dtype=np.int32)
    lib().unique_host_filter(_p(m), _p(best), len(m), int(nt), _p(owner))
    return m, owner


# ---- the tracks recipe ------------------------------------------------------------------------------------------------------------------
def _flip(rng, row, n_bits):
    out = row.copy()
    for b in rng.choice(512, size=rng.randint(0, n_bits + 1), replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def three_cameras(n, dup, seed):
    """B and C: noisy copies of n random rows (at most 30 bits flipped); A: the same plus `dup` SECOND near-copies (at most 40 bits) of the
    first `dup` rows -- repeated structure seen twice"""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, (n, 64)).astype(np.uint8)
    A = np.array([_flip(rng, r, 30) for r in base] + [_flip(rng, base[i], 40) for i in range(dup)], dtype=np.uint8)
    B = np.array([_flip(rng, r, 30) for r in base], dtype=np.uint8)
    Cc = np.array([_flip(rng, r, 30) for r in base], dtype=np.uint8)
    return [A, B, Cc]


PAIRS = [(0, 1), (0, 2), (1, 2)]


def pair_lists(matches):
    """[match of pair (0, 1), (0, 2), (1, 2)] -> the tracks builder's pair dicts: the accepted entries as (q, t) edges"""
    return [dict(cam_a=a, cam_b=b, q=np.nonzero(m >= 0)[0], t=m[m >= 0]) for (a, b), m in zip(PAIRS, matches)]


def doubled_rows(match):
    """train rows named by more than one query"""
    t, c = np.unique(match[match >= 0], return_counts=True)
    return t[c > 1]

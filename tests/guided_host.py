"""The guided match on the host: THE statement the device entries are held to (include/coloc_hip.h, clc_match_guided_dev).

  positions   tests/track_host.py (feature_positions, get_ud_pixel): float32 feature positions, undistorted in float64
  line, gate  the g++ build of coloc_amd/csrc/guided_math.h (tests/host/guided_lib.cpp): not restated here
  top-2       a plain loop over the train rows in index order with the reference's running best / second (CUDAK2NN.cu:54-75), over the
              candidates only; no key packing anywhere

Everything is IEEE arithmetic in a fixed order, so the device results are compared bit for bit (float arrays through their uint32 view:
"none" is the quiet NaN 0x7FC00000).
"""
import ctypes as C
import os
import subprocess

import numpy as np

import track_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
NONE_BITS = 0x7FC00000


def lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "tests", "host", "libguided_host.so")
        src = os.path.join(ROOT, "tests", "host", "guided_lib.cpp")
        hdr = os.path.join(ROOT, "coloc_amd", "csrc", "guided_math.h")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        _LIB = C.CDLL(out)
        _LIB.guided_host_none_bits.restype = C.c_uint32
        assert _LIB.guided_host_none_bits() == NONE_BITS
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ud_positions(cam, kps=None, feat=None):
    """(n, 2) float64: feature position (float32) -> get_ud_pixel; exactly one of kps (detector keypoints) / feat (float rows)"""
    assert (kps is None) != (feat is None)
    pos = track_host.feature_positions(kps) if kps is not None else np.asarray(feat, dtype=np.float32)[:, :2]
    return track_host.get_ud_pixel(pos.astype(np.float64), cam)


def lines(F, uv):
    """(L (n, 3) float32, ok (n,) bool): guided_line of every undistorted pixel"""
    F = np.ascontiguousarray(F, dtype=np.float64).reshape(9)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    L = np.empty((len(uv), 3), dtype=np.float32)
    ok = np.zeros(len(uv), dtype=np.uint8)
    lib().guided_host_lines(_p(F), _p(uv), len(uv), _p(L), _p(ok))
    return L, ok.astype(bool)


def gate(L, xy, band):
    """(n,) bool: guided_in_band of one line against n train points"""
    L = np.ascontiguousarray(L, dtype=np.float32).reshape(3)
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    out = np.zeros(len(xy), dtype=np.uint8)
    lib().guided_host_gate(_p(L), _p(xy), len(xy), C.c_float(band), _p(out))
    return out.astype(bool)


def hamming(Q, T):
    """(nq, nt) int32 Hamming distances of 64-byte rows"""
    qb = np.unpackbits(np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 64), axis=1).astype(np.float32)
    tb = np.unpackbits(np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 64), axis=1).astype(np.float32)
    d = qb.sum(1)[:, None] + tb.sum(1)[None, :] - 2.0 * (qb @ tb.T)          # integers <= 512: exact in float32
    return d.astype(np.int32)


def top2(D, cand, threshold):
    """CUDAK2NN.cu:54-75 over the candidates: train rows in index order, every query's running pair advanced per row.
    Returns (match, best, second) with the sentinels 100000 / 200000."""
    nq, nt = D.shape
    best = np.full(nq, 100000, dtype=np.int64)
    second = np.full(nq, 200000, dtype=np.int64)
    bi = np.full(nq, -1, dtype=np.int64)
    for t in range(nt):
        d = D[:, t].astype(np.int64)
        c = cand[:, t]
        lt = c & (d < best)
        lt2 = c & ~lt & (d < second)
        second = np.where(lt, best, np.where(lt2, d, second))
        bi = np.where(lt, t, bi)
        best = np.where(lt, d, best)
    thr = int(threshold) & 0xFF                                              # the reference's kernel parameter is uint8_t
    match = np.where((bi >= 0) & (second - best > thr), bi, -1).astype(np.int32)
    return match, best, second


def plain(Q, T, threshold):
    """K2NN over all train rows (what clc_match_2nn_dev computes), by the same loop"""
    D = hamming(Q, T)
    return top2(D, np.ones(D.shape, dtype=bool), threshold)


def statement(Q, T, F, band, threshold, cam_a, cam_b, kps_a=None, feat_a=None, kps_b=None, feat_b=None, count_a=None, count_b=None):
    """dict: match (nq,) int32, best / second (uint16, saturated), line (nq, 3) float32, tpos (nt, 2) float32, cand (nq, nt) bool,
    D (nq, nt), best_raw / second_raw (with the sentinels)"""
    Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 64)
    T = np.ascontiguousarray(T, dtype=np.uint8).reshape(-1, 64)
    nq, nt = len(Q), len(T)
    nq_eff = nq if count_a is None else min(nq, int(count_a))
    nt_eff = nt if count_b is None else min(nt, int(count_b))
    none = np.array([NONE_BITS], dtype=np.uint32).view(np.float32)[0]
    line = np.full((nq, 3), none, dtype=np.float32)
    tpos = np.full((nt, 2), none, dtype=np.float32)
    if nq_eff:
        uv = ud_positions(cam_a, kps_a[:nq_eff] if kps_a is not None else None, feat_a[:nq_eff] if feat_a is not None else None)
        line[:nq_eff] = lines(F, uv)[0]
    if nt_eff:
        xy = ud_positions(cam_b, kps_b[:nt_eff] if kps_b is not None else None, feat_b[:nt_eff] if feat_b is not None else None)
        tpos[:nt_eff] = xy.astype(np.float32)                                # each coordinate rounded once
    cand = np.zeros((nq, nt), dtype=bool)
    for q in range(nq_eff):
        if nt_eff:
            cand[q, :nt_eff] = gate(line[q], tpos[:nt_eff], band)
    D = hamming(Q, T) if nt else np.zeros((nq, 0), dtype=np.int32)
    match, best, second = top2(D, cand, threshold)
    return dict(match=match, best=np.minimum(best, 65535).astype(np.uint16), second=np.minimum(second, 65535).astype(np.uint16),
                line=line, tpos=tpos, cand=cand, D=D, best_raw=best, second_raw=second)


# ---- inputs the tests share ------------------------------------------------------------------------------------------------------------
F_ROWS = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])     # the line of (u, v) is (0, -1, v): e = v_a - y_b exactly
CAM_EXACT = (512.0, 320.0, 240.0, 0.0, 0.0, 0.0)                            # power-of-two focal, integral principal point, no distortion:
                                                                           # half-integer positions come through get_ud_pixel unchanged
W, H = 640, 480


def _flip(rng, row, nbits):
    out = row.copy()
    for b in rng.choice(512, nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def make_case(nq, nt, seed):
    """Descriptors and float positions (feat rows of stride 2) for F_ROWS-like geometry (the line of a query is the image row through
    it), with every class planted by query index q % 6 wherever the sizes leave room:
      0  a true match in the band
      1  a true match in the band and a closer look-alike far outside it (the unrestricted best row is not a candidate)
      2  two identical train rows in the band: a tie for the minimum
      3  a query whose line misses every train point (no candidates)
      4  a query on the reserved stripe that holds train row 0 alone (exactly one candidate, accepted whatever its distance)
      5  nothing planted
    Returns (Q, T, qpos, tpos)."""
    rng = np.random.RandomState(seed)
    T = rng.randint(0, 256, (nt, 64)).astype(np.uint8)
    Q = rng.randint(0, 256, (nq, 64)).astype(np.uint8)
    tpos = np.column_stack([rng.uniform(20, W - 20, nt), rng.uniform(60, H - 20, nt)]).astype(np.float32)
    qpos = np.column_stack([rng.uniform(20, W - 20, nq), rng.uniform(60, H - 20, nq)]).astype(np.float32)
    if nt:
        tpos[0, 1] = 20.0                                                    # the stripe y < 60 holds train row 0 alone
    for q in range(nq):
        kind = q % 6
        if nt < 2 and kind in (0, 1, 2):
            continue
        m = 1 + rng.randint(nt - 1) if nt > 1 else 0
        if kind in (0, 1, 2):
            Q[q] = _flip(rng, T[m], 10)
            qpos[q, 1] = tpos[m, 1] + np.float32(rng.uniform(-1.0, 1.0))
        if kind in (1, 2) and nt > 2:
            m2 = 1 + rng.randint(nt - 1)
            if m2 == m:
                continue
            if kind == 1:
                T[m2] = _flip(rng, Q[q], 3)
                far = tpos[m, 1] + 150.0
                tpos[m2, 1] = far if far < H - 20 else tpos[m, 1] - 150.0
            else:
                T[m2] = T[m]
                tpos[m2, 1] = tpos[m, 1] + np.float32(0.5)
        if kind == 3:
            qpos[q, 1] = -200.0
        if kind == 4:
            qpos[q, 1] = 20.0 + np.float32(rng.uniform(-1.0, 1.0))
    return Q, T, qpos, tpos


def classes(st, Q, T, threshold):
    """how many queries of a statement fall into each class the tests ask for"""
    ncand = st["cand"].sum(1)
    pm, pb, _ = plain(Q, T, threshold) if len(T) else (np.full(len(Q), -1), None, None)
    nq, nt = st["cand"].shape
    pbest = np.argmin(st["D"], axis=1) if nt else np.full(nq, -1)               # the unrestricted best row (lowest index on ties)
    outside = np.array([nt > 0 and not st["cand"][q, pbest[q]] for q in range(nq)], dtype=bool)
    tie = (ncand >= 2) & (st["best_raw"] == st["second_raw"])
    return dict(none=int((ncand == 0).sum()), one=int((ncand == 1).sum()), many=int((ncand >= 2).sum()), best_outside=int(outside.sum()),
                tie=int(tie.sum()), tie_rejected=bool((st["match"][tie] == -1).all()))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))

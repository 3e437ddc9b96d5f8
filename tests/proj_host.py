"""The map match guided by a predicted pose on the host: THE statement the device entries are held to (include/coloc_hip.h,
clc_match_map_guided_dev).

  query points      tests/guided_host.py (ud_positions over tests/track_host.py): float32 feature positions, undistorted in float64, each
                    coordinate rounded once to float32
  projection, gate  the g++ build of coloc_amd/csrc/proj_math.h (tests/host/proj_lib.cpp): not restated here
  top-2             guided_host.top2: the reference's running best / second (CUDAK2NN.cu:54-75) over the candidates only, in map-row order

Everything is IEEE arithmetic in a fixed order, so the device results are compared bit for bit (float arrays through their uint32 view:
"none" is the quiet NaN 0x7FC00000).
"""
import ctypes as C
import os
import subprocess

import numpy as np

import guided_host as gh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
IDENTITY = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])


def lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "tests", "host", "libproj_host.so")
        src = os.path.join(ROOT, "tests", "host", "proj_lib.cpp")
        hdrs = [os.path.join(ROOT, "coloc_amd", "csrc", h) for h in ("proj_math.h", "guided_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        _LIB = C.CDLL(out)
        _LIB.proj_host_none_bits.restype = C.c_uint32
        assert _LIB.proj_host_none_bits() == gh.NONE_BITS
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def project(Rt, cam, X):
    """(xy (n, 2) float32, ok (n,) bool): proj_point of every landmark under [R|t] (12 numbers) and cam = (focal, ppx, ppy, ...)"""
    Rt = np.ascontiguousarray(Rt, dtype=np.float64).reshape(12)
    c = np.ascontiguousarray(cam[:3], dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    xy = np.empty((len(X), 2), dtype=np.float32)
    ok = np.zeros(len(X), dtype=np.uint8)
    lib().proj_host_points(_p(Rt), _p(c), _p(X), len(X), _p(xy), _p(ok))
    return xy, ok.astype(bool)


def r2_of(radius):
    """radius * radius, formed once in float32 (what the entry forms on the host)"""
    return np.float32(radius) * np.float32(radius)


def gate(q, xy, r2):
    """(n,) bool: proj_in_radius of one query point against n train points"""
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(2)
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    out = np.zeros(len(xy), dtype=np.uint8)
    lib().proj_host_gate(_p(q), _p(xy), len(xy), C.c_float(r2), _p(out))
    return out.astype(bool)


def statement(Q, M, X, Rt, radius, threshold, cam, kps=None, feat=None, count=None):
    """dict: match (nq,) int32, best / second (uint16, saturated), qpos (nq, 2) float32, proj (nm, 2) float32, cand (nq, nm) bool,
    D (nq, nm), best_raw / second_raw (with the sentinels).  M: the map's descriptor rows, X: their landmarks (at least as many)."""
    Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, 64)
    M = np.ascontiguousarray(M, dtype=np.uint8).reshape(-1, 64)
    nq, nm = len(Q), len(M)
    nq_eff = nq if count is None else min(nq, int(count))
    none = np.array([gh.NONE_BITS], dtype=np.uint32).view(np.float32)[0]
    qpos = np.full((nq, 2), none, dtype=np.float32)
    if nq_eff:
        uv = gh.ud_positions(cam, kps[:nq_eff] if kps is not None else None, feat[:nq_eff] if feat is not None else None)
        qpos[:nq_eff] = uv.astype(np.float32)                                # each coordinate rounded once
    proj = project(Rt, cam, np.asarray(X, dtype=np.float64).reshape(-1, 3)[:nm])[0] if nm else np.zeros((0, 2), dtype=np.float32)
    r2 = r2_of(radius)
    cand = np.zeros((nq, nm), dtype=bool)
    for q in range(nq_eff):
        if nm:
            cand[q] = gate(qpos[q], proj, r2)
    D = gh.hamming(Q, M) if nm else np.zeros((nq, 0), dtype=np.int32)
    match, best, second = gh.top2(D, cand, threshold)
    return dict(match=match, best=np.minimum(best, 65535).astype(np.uint16), second=np.minimum(second, 65535).astype(np.uint16),
                qpos=qpos, proj=proj, cand=cand, D=D, best_raw=best, second_raw=second)


# ---- inputs the tests share ------------------------------------------------------------------------------------------------------------
def landmark(x, y, z):
    """the point that gh.CAM_EXACT under the identity pose sees at pixel (x, y) from depth z: with z a power of two and (x, y)
    half-integers every operation of the projection is exact.  z <= 0: the point the same formula gives (never projected)."""
    return np.array([(x - 320.0) * z / 512.0, (y - 240.0) * z / 512.0, z])


def _half(rng, lo, hi, n):
    return rng.randint(2 * lo, 2 * hi + 1, n) * 0.5


def make_case(nq, nm, seed, behind=True):
    """Descriptors, float query positions (feat rows of stride 2) and landmarks for gh.CAM_EXACT under the identity pose, every class
    planted by query index q % 7 while the map has unused rows left (each planted row serves one query):
      0  a true match inside the radius
      1  a true match inside the radius and a closer look-alike far outside it (the unrestricted best row is not a candidate)
      2  two identical map rows inside the radius: a tie for the minimum
      3  a query far from every projection (no candidate)
      4  a query on the reserved stripe that holds map row 0 alone (exactly one candidate, accepted whatever its distance)
      5  nothing planted
      6  the query's exact copy on a landmark with z <= 0 whose pixel formula lands ON the query (never a candidate); behind=False
         leaves this class out, so that every landmark is in front
    Meant for radii of 2 .. 4 px.  Returns (Q, M, qpos (nq, 2) float32, X (nm, 3))."""
    rng = np.random.RandomState(seed)
    M = rng.randint(0, 256, (nm, 64)).astype(np.uint8)
    Q = rng.randint(0, 256, (nq, 64)).astype(np.uint8)
    mpos = np.column_stack([_half(rng, 20, gh.W - 20, nm), _half(rng, 60, gh.H - 20, nm)])
    qpos = np.column_stack([_half(rng, 20, gh.W - 20, nq), _half(rng, 60, gh.H - 20, nq)])
    z = 2.0 ** rng.randint(0, 5, nm)
    if nm:
        mpos[0] = (320.0, 20.0)                                              # the stripe y < 60 holds map row 0 alone
    free = list(1 + rng.permutation(max(nm - 1, 0)))
    for q in range(nq):
        kind = q % 7
        need = {0: 1, 1: 2, 2: 2, 6: 1}.get(kind, 0)
        if kind == 3:
            qpos[q] = (-300.5, -300.5)
        if kind == 4:
            qpos[q] = (320.0 + rng.randint(-1, 2), 20.0 + rng.randint(-1, 2) * 0.5)
        if need == 0 or len(free) < need or (kind == 6 and not behind):
            continue
        m = free.pop()
        if kind in (0, 1, 2):
            Q[q] = gh._flip(rng, M[m], 10)
            qpos[q] = mpos[m] + (rng.randint(-1, 2), rng.randint(-2, 3) * 0.5)
        if kind == 1:
            m2 = free.pop()
            M[m2] = gh._flip(rng, Q[q], 3)
            mpos[m2] = (mpos[m][0], mpos[m][1] + 150.0 if mpos[m][1] + 150.0 < gh.H - 20 else mpos[m][1] - 150.0)
        if kind == 2:
            m2 = free.pop()
            M[m2] = M[m]
            mpos[m2] = mpos[m] + (0.5, 0.0)
        if kind == 6:
            M[m] = Q[q]
            mpos[m] = qpos[q]
            z[m] = 0.0 if (q // 7) % 2 else -z[m]
    X = np.array([landmark(mpos[i, 0], mpos[i, 1], z[i]) for i in range(nm)]).reshape(-1, 3)
    return Q, M, qpos.astype(np.float32), X


def classes(st, Q, M, threshold):
    """how many queries of a statement fall into each class the tests ask for"""
    ncand = st["cand"].sum(1)
    nq, nm = st["cand"].shape
    pbest = np.argmin(st["D"], axis=1) if nm else np.full(nq, -1)               # the unrestricted best row (lowest index on ties)
    outside = np.array([nm > 0 and not st["cand"][q, pbest[q]] for q in range(nq)], dtype=bool)
    noproj = (st["proj"].view(np.uint32) == gh.NONE_BITS).all(1) if nm else np.zeros(0, dtype=bool)
    copy_behind = np.array([nm > 0 and st["D"][q, pbest[q]] == 0 and noproj[pbest[q]] for q in range(nq)], dtype=bool)
    tie = (ncand >= 2) & (st["best_raw"] == st["second_raw"])
    return dict(none=int((ncand == 0).sum()), one=int((ncand == 1).sum()), many=int((ncand >= 2).sum()), best_outside=int(outside.sum()),
                tie=int(tie.sum()), tie_rejected=bool((st["match"][tie] == -1).all()), accepted=int((st["match"] >= 0).sum()),
                copy_behind=int(copy_behind.sum()))


def all_classes_occur(c):
    return min(c["none"], c["one"], c["many"], c["best_outside"], c["tie"], c["accepted"], c["copy_behind"]) > 0 and c["tie_rejected"]

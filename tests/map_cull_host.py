"""The map's observation statistics and the cull on the host: THE statement clc_map_observe_dev, clc_map_cull_dev, clc_map_stats_get and
clc_cull_map_points are held to (include/coloc_hip.h), written sequentially in Python / numpy.

  projection, gate  the g++ build of coloc_amd/csrc/proj_math.h behind tests/proj_host.py (project, gate, r2_of): not restated here
  keypoints         tests/guided_host.py::ud_positions, each coordinate rounded once to float32 (the map-guided prep's bits)
  cover, in view, observe, drops, remap, list remap
                    Python loops and integer arithmetic below; tests/test_map_cull_host.py holds the g++ build of
                    coloc_amd/csrc/cull_math.h (tests/host/map_cull_lib.cpp) to them

Everything is IEEE comparison or integer work, so the device results are compared exactly.  A view is a dict: cam (focal, ppx, ppy, k1,
k2, k3), Rt (3, 4), feat (n, 2) float32 or kps, track (n,) int32 or None, count or None, width, height, gate, margin."""
import ctypes as C
import os
import subprocess

import numpy as np

import guided_host as gh
import proj_host as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = []
KEPT, FLAGGED, RATIO, IDLE = 0, 1, 2, 3
DEFAULT_RULE = dict(min_visible=8, num=1, den=4, max_idle=0)
M32 = 0xFFFFFFFF


def lib():
    if not _LIB:
        out = os.path.join(ROOT, "tests", "host", "libmap_cull_host.so")
        src = os.path.join(ROOT, "tests", "host", "map_cull_lib.cpp")
        hdrs = [os.path.join(ROOT, "coloc_amd", "csrc", h) for h in ("cull_math.h", "proj_math.h", "guided_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        L = C.CDLL(out)
        L.map_cull_host_remap.restype = C.c_int32
        L.map_cull_host_remap_valid.restype = C.c_int32
        _LIB.append(L)
    return _LIB[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the g++ build of cull_math.h -----------------------------------------------------------------------------------------------------
def cxx_bounds(width, height, margin):
    out = np.zeros(3, dtype=np.float32)
    lib().map_cull_host_bounds(int(width), int(height), C.c_float(margin), _p(out))
    return out


def cxx_in_view(uv, lo, hi_x, hi_y):
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    out = np.zeros(len(uv), dtype=np.uint8)
    lib().map_cull_host_in_view(_p(uv), len(uv), C.c_float(lo), C.c_float(hi_x), C.c_float(hi_y), _p(out))
    return out.astype(bool)


def cxx_rule(visible, found, last_view, epoch, flagged, min_visible, num, den, max_idle):
    """(clause (n,) uint8, drops (n,) bool) of the g++ build"""
    v, f, l = (np.ascontiguousarray(a, dtype=np.uint32) for a in (visible, found, last_view))
    fl = None if flagged is None else np.ascontiguousarray(flagged, dtype=np.uint8)
    clause, drops = np.zeros(len(v), dtype=np.uint8), np.zeros(len(v), dtype=np.uint8)
    lib().map_cull_host_rule(_p(v), _p(f), _p(l), len(v), C.c_uint32(epoch & M32), None if fl is None else _p(fl), C.c_uint32(min_visible),
                             C.c_uint32(num), C.c_uint32(den), C.c_uint32(max_idle), _p(clause), _p(drops))
    return clause, drops.astype(bool)


def cxx_remap(drops):
    d = np.ascontiguousarray(drops, dtype=np.uint8)
    out = np.zeros(len(d), dtype=np.int32)
    return out, int(lib().map_cull_host_remap(_p(d), len(d), _p(out)))


def cxx_remap_list(lst, n_before, remap_):
    out = np.ascontiguousarray(lst, dtype=np.int32).copy()
    r = np.ascontiguousarray(remap_, dtype=np.int32)
    lib().map_cull_host_remap_list(_p(out), len(out), int(n_before), _p(r) if len(r) else None)
    return out


def cxx_remap_valid(remap_):
    r = np.ascontiguousarray(remap_, dtype=np.int32)
    return int(lib().map_cull_host_remap_valid(_p(r) if len(r) else None, len(r)))


def cxx_default_rule():
    out = np.zeros(4, dtype=np.int32)
    lib().map_cull_host_default_rule(_p(out))
    return dict(min_visible=int(out[0]), num=int(out[1]), den=int(out[2]), max_idle=int(out[3]))


# ---- the statement --------------------------------------------------------------------------------------------------------------------
class Stats:
    """the context's per-row state: visible, found, last_view (lists of Python ints below 2^32), epoch, rows (the rows they cover)"""

    def __init__(self):
        self.reset()

    def reset(self):
        """whatever replaces the map's rows"""
        self.visible, self.found, self.last_view, self.epoch, self.rows = [], [], [], 0, 0

    def cover(self, map_n):
        """rows [rows, map_n) -- what the extension appended -- start at zero with last_view = the epoch as it stands"""
        for arr in (self.visible, self.found, self.last_view):
            del arr[map_n:]
        while len(self.visible) < map_n:
            self.visible.append(0)
            self.found.append(0)
            self.last_view.append(self.epoch)
        self.rows = map_n

    def arrays(self):
        return tuple(np.array(a, dtype=np.uint32) for a in (self.visible, self.found, self.last_view))

    def copy(self):
        out = Stats()
        out.visible, out.found, out.last_view, out.epoch, out.rows = list(self.visible), list(self.found), list(self.last_view), self.epoch, self.rows
        return out


def bounds(width, height, margin):
    """(lo, hi_x, hi_y) float32, formed once"""
    m = np.float32(margin)
    return m, np.float32(np.float32(width - 1) - m), np.float32(np.float32(height - 1) - m)


def in_view(uv, lo, hi_x, hi_y):
    """(n,) bool: the rectangle test in float32; NaN is outside"""
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        return (uv[:, 0] >= lo) & (uv[:, 0] <= hi_x) & (uv[:, 1] >= lo) & (uv[:, 1] <= hi_y)


def view_flags(X, v):
    """(in_view (map_n,) bool, hit (map_n,) bool, proj (map_n, 2) float32) of one view against the landmarks X"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    nm = len(X)
    proj = ph.project(v["Rt"], v["cam"], X)[0] if nm else np.zeros((0, 2), dtype=np.float32)
    inv = in_view(proj, *bounds(v["width"], v["height"], v["margin"]))
    hit = np.zeros(nm, dtype=bool)
    track = v.get("track")
    if track is not None and nm:
        n = len(track)
        n_eff = n if v.get("count") is None else min(n, int(v["count"]))
        if n_eff:
            kps, feat = v.get("kps"), v.get("feat")
            qpos = gh.ud_positions(v["cam"], kps[:n_eff] if kps is not None else None, feat[:n_eff] if feat is not None else None).astype(np.float32)
            r2 = ph.r2_of(v["gate"])
            for q in range(n_eff):
                r = int(track[q])
                if 0 <= r < nm and ph.gate(qpos[q], proj[r:r + 1], r2)[0]:
                    hit[r] = True
    return inv, hit, proj


def observe(st, X, views):
    """ONE observe call = ONE epoch, a single view or a batch.  Returns per view (n_in_view, n_hit)."""
    nm = len(np.asarray(X).reshape(-1, 3))
    st.cover(nm)
    st.epoch = (st.epoch + 1) & M32
    counts = []
    for v in views:
        inv, hit, _ = view_flags(X, v)
        for r in range(nm):
            if inv[r]:
                st.visible[r] = (st.visible[r] + 1) & M32
                if hit[r]:
                    st.found[r] = (st.found[r] + 1) & M32
                st.last_view[r] = st.epoch
        counts.append((int(inv.sum()), int((inv & hit).sum())))
    return counts


def clause(visible, found, last_view, epoch, flagged, min_visible, num, den, max_idle):
    """the first clause that fires, in the order written"""
    if flagged:
        return FLAGGED
    if visible >= min_visible and found * den < num * visible:           # Python integers: exact
        return RATIO
    if max_idle > 0 and ((epoch - last_view) & M32) > max_idle:
        return IDLE
    return KEPT


def remap(drops):
    """(remap (n,) int32, kept): kept rows in ascending old order"""
    out, kept = [], 0
    for d in drops:
        if d:
            out.append(-1)
        else:
            out.append(kept)
            kept += 1
    return np.array(out, dtype=np.int32).reshape(-1), kept


def remap_list(lst, n_before, remap_):
    return np.array([int(remap_[e]) if 0 <= e < n_before else -1 for e in np.asarray(lst).tolist()], dtype=np.int32).reshape(-1)


def cull(st, M, X, rule, flagged=None, lists=()):
    """A cull of the map (M rows, X points) with the state st, which it leaves as the call does.  Returns dict(remap, map_n_before, n_kept,
    n_dropped, n_flagged, n_ratio, n_idle, M, X, lists)."""
    M, X = np.asarray(M, dtype=np.uint8).reshape(-1, 64), np.asarray(X, dtype=np.float64).reshape(-1, 3)
    n = len(M)
    st.cover(n)
    cl = [clause(st.visible[r], st.found[r], st.last_view[r], st.epoch, bool(flagged[r]) if flagged is not None else False, rule["min_visible"],
                 rule["num"], rule["den"], rule["max_idle"]) for r in range(n)]
    rm, kept = remap([c != KEPT for c in cl])
    keep = [r for r in range(n) if cl[r] == KEPT]
    st.visible, st.found, st.last_view = [st.visible[r] for r in keep], [st.found[r] for r in keep], [st.last_view[r] for r in keep]
    st.rows = kept
    return dict(remap=rm, map_n_before=n, n_kept=kept, n_dropped=n - kept, n_flagged=cl.count(FLAGGED), n_ratio=cl.count(RATIO), n_idle=cl.count(IDLE),
                M=M[keep].copy(), X=X[keep].copy(), lists=[remap_list(l, n, rm) for l in lists])

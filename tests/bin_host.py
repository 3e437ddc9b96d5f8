"""The cell rule of the map match through a cell grid on the host (include/coloc_hip.h, clc_match_map_binned_dev): the numpy statement of
the grid, k, the cell of a projection, the window of a query and the table, and the g++ build of coloc_amd/csrc/bin_math.h
(tests/host/bin_lib.cpp) the statement is held to.

Everything is IEEE fp64 + - * / and floor in a fixed order, so the two are compared exactly.  The table builder (cell_start, the rows of
every cell) is the statement for clc_map_bin_build_dev.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
AXIS = 66
CELLS = AXIS * AXIS
MAX_ROWS = 65536
SWEEP, BINNED = 0, 1


def lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "tests", "host", "libbin_host.so")
        src = os.path.join(ROOT, "tests", "host", "bin_lib.cpp")
        hdrs = [os.path.join(ROOT, "coloc_amd", "csrc", h) for h in ("bin_math.h", "guided_math.h")]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        _LIB = C.CDLL(out)
        _LIB.bin_host_grid.argtypes = [C.c_double, C.c_double, C.c_float, C.c_void_p]
        _LIB.bin_host_k.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p]
        _LIB.bin_host_cells.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p]
        _LIB.bin_host_windows.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]
        _LIB.bin_host_plan.argtypes = [C.c_double, C.c_double, C.c_float, C.c_longlong]
        assert _LIB.bin_host_cells_per_axis() == AXIS and _LIB.bin_host_max_rows() == MAX_ROWS
    return _LIB


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the numpy statement ---------------------------------------------------------------------------------------------------------------
def grid(cam, radius):
    """(rw, W, c) of a job: the window's half-width, the grid's extent, the cell's side; cam = (focal, ppx, ppy, ...)"""
    ppx, ppy = np.float64(cam[1]), np.float64(cam[2])
    rw = np.float64(np.float32(radius)) * (1.0 + 2.0 ** -10)
    with np.errstate(all="ignore"):
        W = 2.0 * (ppx if ppx > ppy else ppy)
        side = W / 64.0
        c = rw if rw > side else side
    return float(rw), float(W), float(c)


def k(v, c):
    """(int32) min(max(floor(v / c), -1), 64) + 1 of float64 values; a NaN falls to the lower clamp"""
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(v, dtype=np.float64) / np.float64(c))
        f = np.where(f > -1.0, f, -1.0)
        f = np.where(f < 64.0, f, 64.0)
    return f.astype(np.int32) + 1


def cells(xy, c):
    """the cell of every float32 point (n, 2); -1 for a row without a projection"""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    there = ~np.isnan(xy).any(1)
    out = k(xy[:, 1].astype(np.float64), c) * AXIS + k(xy[:, 0].astype(np.float64), c)
    return np.where(there, out, -1).astype(np.int32)


def windows(q, rw, c):
    """(n, 4) int32 { kx0, kx1, ky0, ky1 } of float32 query points (n, 2); { 1, 0, 1, 0 } (empty) for a query whose point is NaN"""
    q = np.asarray(q, dtype=np.float32).reshape(-1, 2)
    q64 = q.astype(np.float64)
    with np.errstate(all="ignore"):
        out = np.column_stack([k(q64[:, 0] - rw, c), k(q64[:, 0] + rw, c), k(q64[:, 1] - rw, c), k(q64[:, 1] + rw, c)]).astype(np.int32)
    out[np.isnan(q).any(1)] = (1, 0, 1, 0)
    return out


def plan(cam, radius, map_n):
    """BINNED iff radius >= 2^-10, 8 rw <= W, 0 < map_n <= 65 536 and ppx, ppy finite and positive"""
    ppx, ppy = float(cam[1]), float(cam[2])
    rw, W, _ = grid(cam, radius)
    ok = np.isfinite(ppx) and np.isfinite(ppy) and ppx > 0.0 and ppy > 0.0 and np.float32(radius) >= np.float32(2.0 ** -10) and 8.0 * rw <= W
    return BINNED if ok and 0 < map_n <= MAX_ROWS else SWEEP


def table(proj, c):
    """(cell_start (4357,) int32, cell_row: the binned rows sorted by (cell, row)) of float32 projections (nm, 2): the statement of
    clc_map_bin_build_dev, whose order inside a cell is unspecified"""
    cl = cells(proj, c)
    rows = np.nonzero(cl >= 0)[0]
    order = rows[np.argsort(cl[rows], kind="stable")]
    counts = np.bincount(cl[rows], minlength=CELLS)
    cell_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return cell_start, order.astype(np.int32)


def visited(q, proj, rw, c):
    """how many binned rows the window of each query holds (the rows a query visits)"""
    cell_start, _ = table(proj, c)
    w = windows(q, rw, c)
    n = np.zeros(len(w), dtype=np.int64)
    for ky_off in range(3):
        ky = w[:, 2] + ky_off
        on = ky <= w[:, 3]
        lo = np.where(on, ky * AXIS + w[:, 0], 0)
        hi = np.where(on, ky * AXIS + w[:, 1] + 1, 0)
        n += np.where(on & (w[:, 0] <= w[:, 1]), cell_start[hi] - cell_start[lo], 0)
    return n


# ---- the g++ build of bin_math.h --------------------------------------------------------------------------------------------------------
def cxx_grid(cam, radius):
    out = np.zeros(3, dtype=np.float64)
    lib().bin_host_grid(float(cam[1]), float(cam[2]), float(np.float32(radius)), _p(out))
    return tuple(out.tolist())


def cxx_k(v, c):
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    out = np.zeros(len(v), dtype=np.int32)
    lib().bin_host_k(_p(v), len(v), c, _p(out))
    return out


def cxx_cells(xy, c):
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    out = np.zeros(len(xy), dtype=np.int32)
    lib().bin_host_cells(_p(xy), len(xy), c, _p(out))
    return out


def cxx_windows(q, rw, c):
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 2)
    out = np.zeros((len(q), 4), dtype=np.int32)
    lib().bin_host_windows(_p(q), len(q), rw, c, _p(out))
    return out


def cxx_plan(cam, radius, map_n):
    return lib().bin_host_plan(float(cam[1]), float(cam[2]), float(np.float32(radius)), int(map_n))

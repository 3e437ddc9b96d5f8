"""ctypes access to the host build of the SO(3) helpers and the 6x6 solve (tests/host/so3_host_lib.cpp over coloc_amd/csrc/so3.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        out = os.path.join(ROOT, "tests", "host", "libso3_host.so")
        src = os.path.join(ROOT, "tests", "host", "so3_host_lib.cpp")
        hdr = os.path.join(ROOT, "coloc_amd", "csrc", "so3.h")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
        _LIB = C.CDLL(out)
        _LIB.so3_host_d_rodrigues_entry.restype = C.c_double
        _LIB.so3_host_solve6.restype = C.c_int
        _LIB.so3_host_invert6_column.restype = C.c_int
        _LIB.so3_host_packed6.restype = C.c_int
    return _LIB


def _v(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    assert a.size == n
    return a


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def rodrigues(w):
    w = _v(w, 3); R = np.zeros(9)
    lib().so3_host_rodrigues(_p(w), _p(R))
    return R.reshape(3, 3)


def log_so3(R):
    R = _v(R, 9); w = np.zeros(3)
    lib().so3_host_log(_p(R), _p(w))
    return w


def d_rodrigues(w, R=None):
    """(3, 3, 3): [k] = dR/dw_k."""
    w = _v(w, 3)
    R = _v(rodrigues(w) if R is None else R, 9)
    dR = np.zeros(27)
    lib().so3_host_d_rodrigues(_p(w), _p(R), _p(dR))
    return dR.reshape(3, 3, 3)


def d_rodrigues_entries(w, R=None):
    """The same 27 numbers, each from d_rodrigues_entry (what the kernel's lanes call)."""
    w = _v(w, 3)
    R = _v(rodrigues(w) if R is None else R, 9)
    return np.array([lib().so3_host_d_rodrigues_entry(_p(w), _p(R), C.c_int(k), C.c_int(e)) for k in range(3) for e in range(9)]).reshape(3, 3, 3)


def pack6(A):
    """Packed upper triangle (21) of a symmetric 6 x 6, in the kernel's order."""
    A = np.asarray(A, dtype=np.float64)
    out = np.zeros(21)
    for i in range(6):
        for j in range(i, 6):
            out[lib().so3_host_packed6(i, j)] = A[i, j]
    return out


def solve6(A, g, lam=0.0):
    """(ok, d) with (A + lam diag(A)) d = g."""
    Ap = pack6(A); g = _v(g, 6); d = np.zeros(6)
    ok = lib().so3_host_solve6(_p(Ap), _p(g), C.c_double(lam), _p(d))
    return bool(ok), d


def invert6(A, fill=np.nan):
    """(ok per column, inverse) through invert6_column; columns that failed keep `fill`."""
    Ap = pack6(A); inv = np.full(36, fill)
    ok = [bool(lib().so3_host_invert6_column(_p(Ap), C.c_int(c), _p(inv))) for c in range(6)]
    return ok, inv.reshape(6, 6)

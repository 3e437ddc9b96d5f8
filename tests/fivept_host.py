"""ctypes access to the host build of the sequential five-point solver (tests/host/fivept_host_lib.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# How far the singular values of a returned model may be from (s, s, 0), relative to s.  E', the nearest essential matrix, is
# sqrt((s1 - s2)^2 / 2 + s3^2) from a unit-norm E, and at a point q of the normalised image plane that moves the epipolar line by about
# as much times |q|.  The backward rule of DESIGN.md section 11 allows 4096 * 2^-53 * max(w, h) pixels, so in units of the focal length
# the allowance is 4096 * 2^-53 times the width of the field: 2 in tests/test_fivept_host.py and tests/test_gpu_epipolar.py (|q| <= 1).  (It was 1e-4 while
# the solver's null-space basis let one solution at infinity spoil the others of its sample: observed worst 4.4e-6 then.)
SV_TOL = 4096.0 * 2.0 ** -53 * 2.0
_LIBS = {}
DEFINES = ()          # -D switches of the build that solve() and the rest use (tools/fivept_attribution.py builds the variants of a study)


def lib():
    if DEFINES not in _LIBS:
        tag = "".join("_" + d.replace("=", "") for d in DEFINES)
        out = os.path.join(ROOT, "tests", "host", "libfivept_host%s.so" % tag)
        src = os.path.join(ROOT, "tests", "host", "fivept_host_lib.cpp")
        hdr = os.path.join(ROOT, "coloc_amd", "csrc", "fivept.h")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC"] + ["-D" + d for d in DEFINES] + [src, "-o", out])
        _LIBS[DEFINES] = C.CDLL(out)
        for f in ("fpt_host_solve", "fpt_host_solve_ws", "fpt_host_eig"):
            getattr(_LIBS[DEFINES], f).restype = C.c_int
    return _LIBS[DEFINES]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def solve(q1, q2):
    """q1, q2: 5 x 2 normalised coordinates.  Returns the list of 3 x 3 essential matrices."""
    q1 = np.ascontiguousarray(q1, dtype=np.float64).reshape(5, 2)
    q2 = np.ascontiguousarray(q2, dtype=np.float64).reshape(5, 2)
    E = np.zeros(90)
    n = lib().fpt_host_solve(_p(q1), _p(q2), _p(E))
    return [E[9 * k:9 * k + 9].reshape(3, 3).copy() for k in range(n)]


def workspace(q1, q2):
    """The same solve, and what it left behind: dict(E (n, 3, 3), EE (4, 9) null-space basis, Ax (10, 10), z (10,) complex eigenvalues,
    zdone (10,), xyz (10, 3, 3): per root and stage (start, monomial polish, polish on E) its (x, y, z), reached (10, 3), cand (10, 9),
    valid (10,))."""
    q1 = np.ascontiguousarray(q1, dtype=np.float64).reshape(5, 2)
    q2 = np.ascontiguousarray(q2, dtype=np.float64).reshape(5, 2)
    E, EE, Ax, zr, zi, xyz, cand = np.zeros(90), np.zeros((4, 9)), np.zeros((10, 10)), np.zeros(10), np.zeros(10), np.zeros((10, 3, 3)), np.zeros((10, 9))
    zdone, reached, valid = np.zeros(10, np.int32), np.zeros((10, 3), np.int32), np.zeros(10, np.int32)
    n = lib().fpt_host_solve_ws(_p(q1), _p(q2), _p(E), _p(EE), _p(Ax), _p(zr), _p(zi), _p(zdone), _p(xyz), _p(reached), _p(cand), _p(valid))
    return dict(E=E[:9 * n].reshape(n, 3, 3), EE=EE, Ax=Ax, z=zr + 1j * zi, zdone=zdone, xyz=xyz, reached=reached, cand=cand, valid=valid)


def eig(A):
    """The eigenvalue stage alone on a 10 x 10 matrix: (z (10,) complex, zdone (10,)), or None where the solver gives up."""
    A = np.ascontiguousarray(A, dtype=np.float64).reshape(10, 10)
    zr, zi, zdone = np.zeros(10), np.zeros(10), np.zeros(10, np.int32)
    return (zr + 1j * zi, zdone) if lib().fpt_host_eig(_p(A), _p(zr), _p(zi), _p(zdone)) else None


def normalised(x1, x2, K):
    """Pixels (5, 2) of the two views -> normalised coordinates, as class_slots hands them to the solver."""
    Ki = np.linalg.inv(np.asarray(K, dtype=np.float64).reshape(3, 3))
    return (np.c_[x1, np.ones(5)] @ Ki.T)[:, :2], (np.c_[x2, np.ones(5)] @ Ki.T)[:, :2]


def class_slots(x1, x2, K):
    """The models of a batch of samples in pixels (n, 5, 2) under one K: (n, 10, 9) in calibrated coordinates, NaN where a sample has
    fewer models."""
    out = np.full((len(x1), 10, 9), np.nan)
    for i in range(len(x1)):
        q1, q2 = normalised(x1[i], x2[i], K)
        for k, E in enumerate(solve(q1, q2)):
            out[i, k] = E.reshape(9)
    return out


def random_two_view(rng):
    """A random relative pose and 5 points in front of both cameras: (q1, q2, E_true)."""
    ax = 0.3 * rng.uniform(-1, 1, 3)
    t = rng.uniform(-1, 1, 3) * np.array([1.0, 1.0, 0.3])
    th = np.linalg.norm(ax) + 1e-12
    k = ax / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)
    X = np.c_[rng.uniform(-2, 2, (5, 2)), rng.uniform(2, 6, 5)]
    Y = X @ R.T + t
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return X[:, :2] / X[:, 2:3], Y[:, :2] / Y[:, 2:3], tx @ R

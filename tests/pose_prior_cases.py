"""The case table of the pose-from-the-prediction tests (tests/test_pose_prior_reference.py on the CPU, tests/test_gpu_track_prior.py on
the GPU), built with the scene() recipe of tests/test_gpu_pose_edges.py: n points 4 - 20 units in front of the camera [R | t].

  N           4, 8, 64, 511, 512, 513, 1025, 2000 (512 is the thread stride of the kernel's pass), and the special cases N = 3 and
              "every point behind the prior camera"
  outliers    shares 0, 0.1 and 0.3, displaced by at least 4 gate (12 .. 120 px in a random direction)
  inliers     noise of norm at most 0.5 gate (uniform direction, uniform norm)
  gate        3 px
  prior       the truth perturbed as test_gpu_pose_edges.perturbed() does (0.02 rad, 0.05 units)

A seed is part of the fixture: one whose reference rounds put a track into the 5 % band around the gate (or next to the principal plane)
is a wrong fixture and is replaced, never tolerated (test_pose_prior_reference.py asserts the condition on the reference alone).
reference_live(case) is the 50-digit solve, computed once per process (a minute for the table).  What the GPU tests compare with --
the masks round by round, rounds_run, converged, result -- is also recorded in tests/golden/pose_prior_reference.json (written by
tools/make_pose_prior_reference.py, keyed by a digest of the case's inputs): reference(case) reads the record where the digest matches
and solves live otherwise; test_pose_prior_reference.py holds every record to the live solve.
"""
import functools
import hashlib
import json
import os

import numpy as np

import pose_mp as pm
import pose_prior_mp as ppm
from test_so3_host import HALF_TURNS

GATE = 3.0
HUBER = 16.0

KS = {
    "suite": np.array([[1000.0, 0, 320], [0, 1000, 240], [0, 0, 1]]),
    "skew-40_aniso": np.array([[900.0, -40, 320], [0, 1100, 240], [0, 0, 1]]),
}


def _axis(seed):
    a = np.random.default_rng(seed).standard_normal(3)
    return a / np.linalg.norm(a)


def _rot(angle, axis):
    return pm.to_float(pm.exp_so3(angle * np.asarray(axis, dtype=np.float64)))


ROTS = {"I": np.eye(3), "1rad": _rot(1.0, _axis(4)), "2.5rad": _rot(2.5, _axis(5))}

# (id, K, rotation, N, outlier share, seed, kind)
CASES = [
    ("N-4-out-0", "suite", "1rad", 4, 0.0, 101, "regular"),
    ("N-8-out-0.3", "suite", "2.5rad", 8, 0.3, 102, "regular"),
    ("N-64-out-0", "suite", "I", 64, 0.0, 103, "regular"),
    ("N-64-out-0.1", "skew-40_aniso", "1rad", 64, 0.1, 104, "regular"),
    ("N-64-out-0.3", "suite", "2.5rad", 64, 0.3, 234, "regular"),
    ("N-511-out-0.3", "suite", "1rad", 511, 0.3, 106, "regular"),
    ("N-512-out-0.1", "skew-40_aniso", "2.5rad", 512, 0.1, 107, "regular"),
    ("N-513-out-0", "suite", "I", 513, 0.0, 108, "regular"),
    ("N-1025-out-0.3", "suite", "2.5rad", 1025, 0.3, 276, "regular"),
    ("N-2000-out-0.1", "suite", "1rad", 2000, 0.1, 110, "regular"),
    ("N-3", "suite", "1rad", 3, 0.0, 111, "regular"),
    ("behind-64", "suite", "1rad", 64, 0.1, 112, "behind"),
]
IDS = [c[0] for c in CASES]


def perturbed(Rt, seed):
    a = _axis(seed + 1000)
    d = _axis(seed + 2000)
    return np.concatenate([_rot(0.02, a) @ Rt[:, :3], (Rt[:, 3] + 0.05 * d)[:, None]], 1)


def scene(K, R, n, share, seed, gate=GATE):
    rng = np.random.default_rng(seed)
    z = rng.uniform(4, 20, n)
    Xc = np.stack([rng.uniform(-0.25, 0.25, n) * z, rng.uniform(-0.2, 0.2, n) * z, z], 1)
    t = np.array([0.3, -0.2, 0.5])
    X = (Xc - t) @ R
    uvw = (X @ R.T + t) @ K.T
    ang = rng.uniform(0, 2 * np.pi, n)
    x = uvw[:, :2] / uvw[:, 2:3] + (rng.uniform(0, 0.5 * gate, n))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    n_out = int(share * n)
    out = np.zeros(n, dtype=bool)
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        out[idx] = True
        a2 = rng.uniform(0, 2 * np.pi, n_out)
        x[idx] += rng.uniform(4 * gate, 40 * gate, n_out)[:, None] * np.stack([np.cos(a2), np.sin(a2)], 1)
    return X, x, np.concatenate([R, t[:, None]], 1), out


@functools.lru_cache(maxsize=None)
def build(cid):
    """dict(X, x, K, Rt_true, Rt_prior, outliers) of a case."""
    _, kname, rname, n, share, seed, kind = CASES[IDS.index(cid)]
    K, R = KS[kname], ROTS[rname]
    X, x, Rt_true, out = scene(K, R, n, share, 9000 + seed)
    Rt_prior = perturbed(Rt_true, seed)
    if kind == "behind":
        Rt_prior = HALF_TURNS["e1"] @ Rt_prior            # a half turn about the camera's x axis: every zc changes sign
    return dict(X=X, x=x, K=K, Rt_true=Rt_true, Rt_prior=Rt_prior, outliers=out)


@functools.lru_cache(maxsize=None)
def reference_live(cid):
    c = build(cid)
    return ppm.solve(c["X"], c["x"], c["K"], c["Rt_prior"], GATE, HUBER)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_prior_reference.json")


def digest(cid):
    c = build(cid)
    h = hashlib.sha256()
    for k in ("X", "x", "K", "Rt_prior"):
        h.update(np.ascontiguousarray(c[k], dtype=np.float64).tobytes())
    h.update(repr((GATE, HUBER)).encode())
    return h.hexdigest()


def _bits_of(mask):
    return "".join("1" if v else "0" for v in mask)


def record(cid, ref):
    """what the golden file holds of a reference solve"""
    return dict(digest=digest(cid), masks=[_bits_of(m) for m in ref["masks"]], mask=_bits_of(ref["mask"]), n_inliers=int(ref["n_inliers"]),
                rounds_run=int(ref["rounds_run"]), converged=int(ref["converged"]), result=int(ref["result"]))


@functools.lru_cache(maxsize=None)
def _golden():
    if not os.path.exists(GOLDEN):
        return {}
    with open(GOLDEN) as f:
        return json.load(f)


def reference(cid):
    """masks, mask, n_inliers, rounds_run, converged, result of the reference: the golden record where it is this case's, else the live solve"""
    g = _golden().get(cid)
    if g is None or g["digest"] != digest(cid):
        return reference_live(cid)
    as_mask = lambda s: np.array([ch == "1" for ch in s], dtype=bool)
    return dict(masks=[as_mask(m) for m in g["masks"]], mask=as_mask(g["mask"]), n_inliers=g["n_inliers"], rounds_run=g["rounds_run"],
                converged=g["converged"], result=g["result"])

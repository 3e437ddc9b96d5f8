"""The case lists of the 3-D similarity tests (tests/test_sim3_host.py on the CPU, tests/test_gpu_sim3.py on the GPU): deterministic,
plain numpy.  A minimal case is (name, x (3, 3) new, y (3, 3) old, expect) with expect in {"model", "nan"}; a refit case is
(name, x (n, 3), y (n, 3), expect) with expect in {"refit", "refused"}.  Convention: y ~ s R x + t."""
import numpy as np


def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def similar(x, s, R, t, noise=0.0, rng=None):
    y = s * (x @ R.T) + t
    if noise:
        y = y + rng.normal(0, noise, y.shape)
    return y


def _triangle_with_sine(rng, sine):
    """a triangle whose angle at p0 has the given sine, edges of order 1"""
    p0 = rng.uniform(-2, 2, 3)
    e1 = rng.normal(size=3)
    e1 /= np.linalg.norm(e1)
    n = np.cross(e1, rng.normal(size=3))
    n /= np.linalg.norm(n)
    ang = np.arcsin(sine)
    e2 = 1.3 * (np.cos(ang) * e1 + np.sin(ang) * n)
    return np.stack([p0, p0 + 0.9 * e1, p0 + e2])


def minimal_cases():
    rng = np.random.default_rng(20240)
    out = []
    for i in range(40):                                                # general triangles, noisy: the two triangles are not similar
        x = rng.uniform(-5, 5, (3, 3))
        R = rot(rng.normal(size=3), rng.uniform(0.1, 3.0))
        out.append(("general%d" % i, x, similar(x, rng.uniform(0.5, 4.0), R, rng.uniform(-3, 3, 3), 0.05, rng), "model"))
    for i, s in enumerate(10.0 ** np.linspace(-3, 3, 13)):            # scales 1e-3 .. 1e3
        x = rng.uniform(-5, 5, (3, 3))
        out.append(("scale%d" % i, x, similar(x, s, rot(rng.normal(size=3), 1.0), s * rng.uniform(-3, 3, 3)), "model"))
    for i, ang in enumerate([0.0, 1e-12, 1e-8, 1e-4, np.pi - 1e-4, np.pi - 1e-8, np.pi - 1e-12, np.pi]):   # rotations near 0 and near pi
        x = rng.uniform(-5, 5, (3, 3))
        out.append(("angle%d" % i, x, similar(x, 2.5, rot(rng.normal(size=3), ang), rng.uniform(-3, 3, 3)), "model"))
    for i, sine in enumerate([1.001e-3, 2e-3, 1e-2, 1e-5, 2e-6]):          # thin but on the solved side of the guard (sine^2 > 1e-12)
        x = _triangle_with_sine(rng, sine)
        out.append(("thin%d" % i, x, similar(x, 2.5, rot(rng.normal(size=3), 0.7), rng.uniform(-3, 3, 3)), "model"))
    for i, sine in enumerate([5e-7, 1e-8, 0.0]):                       # the other side: degenerate in both clouds
        x = _triangle_with_sine(rng, sine)
        out.append(("collinear%d" % i, x, similar(x, 2.5, rot(rng.normal(size=3), 0.7), rng.uniform(-3, 3, 3)), "nan"))
    x = _triangle_with_sine(rng, 0.5)
    out.append(("collinear_old_only", x, _triangle_with_sine(rng, 1e-8), "nan"))
    out.append(("collinear_new_only", _triangle_with_sine(rng, 1e-8), x, "nan"))
    p = rng.uniform(-5, 5, (3, 3))
    out.append(("coincident01", np.stack([p[0], p[0], p[2]]), p, "nan"))
    out.append(("coincident02", p, np.stack([p[0], p[1], p[0]]), "nan"))
    out.append(("coincident_all", np.stack([p[0]] * 3), np.stack([p[1]] * 3), "nan"))
    return out


def refit_cases():
    rng = np.random.default_rng(20241)
    out = []
    for n in (4, 128, 129, 2000):                                      # one partial, exactly one, one and a bit, sixteen
        x = rng.uniform(-10, 10, (n, 3)) + [3.0, -2.0, 20.0]
        R = rot(rng.normal(size=3), rng.uniform(0.2, 3.0))
        out.append(("cloud%d" % n, x, similar(x, 2.5, R, [4.0, -1.0, 7.0], 0.02, rng), "refit"))
    x = rng.uniform(-10, 10, (300, 3))
    out.append(("exact300", x, similar(x, 0.37, rot([1, 2, 3], 3.1), [100.0, -50.0, 3.0]), "refit"))
    # a planar cloud: sigma3 = 0 (to rounding).  Its mirror image across the plane is the same cloud, so a REFLECTED old cloud has a proper
    # rotation that fits it exactly -- the case d = -1 of Umeyama's rule (det U det V < 0) is what finds it
    xp = np.concatenate([rng.uniform(-10, 10, (200, 2)), np.zeros((200, 1))], 1)
    Rp = rot(rng.normal(size=3), 1.1)
    out.append(("planar", xp, similar(xp, 2.5, Rp, [1.0, 2.0, 3.0]), "refit"))
    out.append(("planar_reflected", xp, similar(xp * [1.0, 1.0, -1.0], 2.5, Rp @ np.diag([1.0, -1.0, 1.0]), [1.0, 2.0, 3.0]), "refit"))
    # a mirrored noisy cloud: no rotation fits, the best one has d = -1 with sigma3 well above zero
    xm = rng.uniform(-10, 10, (150, 3)) * [1.0, 0.6, 0.25]
    out.append(("mirrored", xm, similar(xm * [1.0, 1.0, -1.0], 1.7, rot(rng.normal(size=3), 0.9), [0.5, 0.5, 0.5], 0.01, rng), "refit"))
    line = np.outer(rng.uniform(-10, 10, 100), [1.0, 2.0, -0.5]) + [1.0, 1.0, 1.0]
    out.append(("collinear", line, similar(line, 2.5, rot([0, 0, 1], 0.3), [0.0, 1.0, 0.0]), "refused"))
    out.append(("one_point", np.tile(rng.uniform(-1, 1, 3), (20, 1)), rng.uniform(-1, 1, (20, 3)), "refused"))
    return out


def planted_scene(n, wrong_share, seed, s=2.5, noise=0.0, duplicates=0):
    """n correspondences y ~ s R x + t of which a share is replaced by uniform points (the planted wrong ones); `duplicates` of the
    right ones are repeated at the end.  -> dict(x, y, planted (bool, n + duplicates), s, R, t)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-10, 10, (n, 3)) + [0.0, 0.0, 25.0]
    R = rot(rng.normal(size=3), 0.1)
    t = np.array([3.0, -2.0, 5.0])
    depth = np.linalg.norm(x, axis=1, keepdims=True)
    y = s * (x @ R.T) + t
    if noise:
        y = y + rng.normal(0, 1.0, y.shape) * noise * depth            # depth-dependent
    planted = np.ones(n, dtype=bool)
    wrong = rng.permutation(n)[: int(round(wrong_share * n))]
    planted[wrong] = False
    lo, hi = y.min(0), y.max(0)
    y[wrong] = rng.uniform(lo, hi, (len(wrong), 3))
    if duplicates:
        dup = rng.choice(np.nonzero(planted)[0], duplicates)
        x, y, planted = np.concatenate([x, x[dup]]), np.concatenate([y, y[dup]]), np.concatenate([planted, planted[dup]])
    return dict(x=x, y=y, planted=planted, s=s, R=R, t=t)

"""The P3P case table (inputs, by deterministic construction) and the two rules a float64 P3P solver is held to against the
high-precision reference (tests/p3p_mp.py, fixture tests/golden/p3p_reference.npz written by tools/make_p3p_reference.py).
DESIGN.md (P3P) derives the rules; in short, with B = 4096 * 2^-53 * max(|x|_inf, fx, fy) and sigma the sine of the world triangle's
angle at the first sample point:

  backward   every returned pose reprojects its own three sample points, at 50 digits, to within B / sigma;
  forward    every in-range reference solution has a returned pose within J_k B / sigma + 16 * 2^-53 * |P|_inf in all 12 entries
             (in range: J B / sigma <= 1e-3 (1 + |P|_inf)), and every returned pose lies within that bound of some reference solution.

Classes: asserted (exact, noisy, skewK, isosceles), hard (far: triangles of size 0.5 seen from 20 to 50; collinear: collinear to
1e-2; completeness only where rho >= 1e-3), one case per guarded branch (cubic, biquadratic, den; where D(v) = 0 at a
solution the quartic has a double root there, the float root lands 1e-8 away, the |den| < 1e-12 guard of p3p_pose_from_root is
not reached and the pose returned is not a solution: the case is in the table, and the tests carry it as a strict xfail), and report-only (tiny: size 0.05
at 20 to 50; collinear4: collinear to 1e-4; equilateral: frontal equilateral, the double-root configuration), whose inputs are not
stored: they are rebuilt here whenever they are wanted.
"""
import math
import os

import numpy as np

import synth

N_PER_CLASS = 60
POOL = 64
ASSERTED = ["exact", "noisy", "skewK", "isosceles"]
HARD = ["far", "collinear"]
BRANCH = ["cubic", "biquadratic", "den"]
REPORT = ["tiny", "collinear4", "equilateral"]
STORED = ASSERTED + HARD + BRANCH
RHO_CAP = 1e-3
K_SKEW = np.array([[900.0, -40.0, 320.0], [0.0, 1100.0, 240.0], [0.0, 0.0, 1.0]])
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p3p_reference.npz")
EPS = 2.0 ** -53
POOLED = ["exact", "noisy", "skewK"]


def class_size(name):
    return 1 if name in BRANCH else N_PER_CLASS


def class_offset(name):
    """Index of the class's first problem in the fixture's per-problem arrays (sigma, rho)."""
    return sum(class_size(c) for c in STORED[:STORED.index(name)])


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def class_references(fx, name):
    """Per problem of a stored class: (sigma, rho, [dict(s_hi (3,), s_lo (3,), J (12,), in_range)])."""
    lo = class_offset(name)
    out = []
    for i in range(lo, lo + class_size(name)):
        rows = np.nonzero(fx["sol_prob"] == i)[0]
        out.append((float(fx["sigma"][i]), float(fx["rho"][i]),
                    [dict(s_hi=fx["s_hi"][r], s_lo=fx["s_lo"][r].astype(np.float64), J=half_to_float(fx["J"][r]), in_range=bool(fx["in_range"][r]))
                     for r in rows]))
    return out


def _project(K, R, t, X):
    uvw = (X @ R.T + t) @ K.T
    return uvw[:, :2] / uvw[:, 2:3]


def pool_scene():
    """The working range: the first POOL points of the noise-free synth.pnp_scene(400, seed=4002) and their pixels, exact, with
    0.5 px of noise, and through the skewed K."""
    sc = synth.pnp_scene(400, seed=4002, outlier_frac=0.0, noise_sigma=0.0)
    X = sc["X"][:POOL].copy()
    x = sc["x"][:POOL].copy()
    rng = np.random.default_rng(4003)
    return dict(X=X, K=sc["K"], R=sc["R"], t=sc["t"], x_exact=x, x_noisy=x + rng.normal(0.0, 0.5, x.shape),
                x_skewK=_project(K_SKEW, sc["R"], sc["t"], X))


def pool_triples(name):
    rng = np.random.default_rng({"exact": 11, "noisy": 12, "skewK": 13}[name])
    return np.stack([rng.choice(POOL, 3, replace=False) for _ in range(N_PER_CLASS)]).astype(np.uint8)


def _random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, a, b, c = q
    return np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                     [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                     [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]])


def _place(rng, tri_cam, K):
    """A triangle given in the camera frame -> world points under a random pose, and its exact pixels."""
    R = _random_rotation(rng)
    t = rng.uniform(-3.0, 3.0, 3)
    X = (tri_cam - t) @ R                      # X = R^T (Xc - t)
    return X, _project(K, R, t, X)


def _centre(rng, lo, hi, K):
    """A point in the camera frame at depth lo..hi that projects well inside a 1280 x 720 image."""
    z = rng.uniform(lo, hi)
    return np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.25, 0.25) * z, z])


def constructed(name):
    """(X (n, 3, 3), x (n, 3, 2), K) of a constructed class."""
    K = synth.pnp_scene(4, seed=4002)["K"]
    rng = np.random.default_rng({"isosceles": 21, "far": 22, "collinear": 23, "tiny": 24, "collinear4": 25, "equilateral": 26}[name])
    Xs, xs = [], []
    for _ in range(N_PER_CLASS):
        if name == "isosceles":                # |X0 X1| = |X1 X2|: a = c, the q = 0 corner of the elimination
            apex = _centre(rng, 6.0, 16.0, K)
            r = rng.uniform(1.0, 3.0)
            d0, d2 = rng.normal(size=3), rng.normal(size=3)
            tri = np.stack([apex + r * d0 / np.linalg.norm(d0), apex, apex + r * d2 / np.linalg.norm(d2)])
        elif name in ("far", "tiny"):
            size = 0.5 if name == "far" else 0.05
            tri = _centre(rng, 20.0, 50.0, K) + rng.uniform(-size, size, (3, 3))
        elif name in ("collinear", "collinear4"):
            off = 1e-2 if name == "collinear" else 1e-4
            a = _centre(rng, 6.0, 16.0, K)
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            nrm = np.cross(d, rng.normal(size=3)); nrm /= np.linalg.norm(nrm)
            L = rng.uniform(2.0, 4.0)
            lam = rng.uniform(0.3, 0.7)
            tri = np.stack([a, a + L * d, a + lam * L * d + off * L * nrm])       # third point off the line by `off` of the length
        else:                                  # frontal equilateral: the plane faces the camera, the centroid on the optical axis
            z = rng.uniform(4.0, 12.0)
            r = rng.uniform(0.5, 2.0)
            ph = rng.uniform(0.0, 2.0 * math.pi)
            tri = np.stack([[r * math.cos(ph + k * 2.0 * math.pi / 3.0), r * math.sin(ph + k * 2.0 * math.pi / 3.0), z] for k in range(3)])
        X, x = _place(rng, tri, K)
        Xs.append(X); xs.append(x)
    return np.stack(Xs), np.stack(xs), K


def class_inputs(name, fx=None):
    """(X (n, 3, 3), x (n, 3, 2), K) of any class; stored classes come from the fixture `fx` when it is given."""
    if fx is not None and name in STORED:
        K = K_SKEW if name == "skewK" else fx["K"]
        if name in POOLED:
            tr = fx["triples"][POOLED.index(name)].astype(np.int64)
            return fx["pool_X"][tr], fx["pool_x"][POOLED.index(name)][tr], K
        lo = sum(class_size(c) for c in STORED[len(POOLED):STORED.index(name)])
        return fx["con_X"][lo:lo + class_size(name)], fx["con_x"][lo:lo + class_size(name)], K
    if name in BRANCH:
        raise ValueError("the branch cases are built by tools/make_p3p_reference.py and live in the fixture only")
    if name in POOLED:
        p = pool_scene()
        tr = pool_triples(name).astype(np.int64)
        return p["X"][tr], p["x_" + name][tr], (K_SKEW if name == "skewK" else p["K"])
    return constructed(name)


def sigma_float(X):
    a, b = X[1] - X[0], X[2] - X[0]
    return float(np.linalg.norm(np.cross(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b)))


def bound_B(x, K):
    return 4096.0 * EPS * max(float(np.abs(x).max()), abs(float(K[0][0])), abs(float(K[1][1])))


def half_up(a):
    """float64 -> the next float16 at or above it; the fixture keeps the sensitivities J in this form (<= 0.1 % above at 6e-5 and more, two bytes).
    Raises where a value is beyond the format's range."""
    a = np.asarray(a, dtype=np.float64)
    h = a.astype(np.float16)
    h = np.where(h.astype(np.float64) < a, np.nextafter(h, np.float16(np.inf)), h).astype(np.float16)
    if not (np.isfinite(h).all() and (h.astype(np.float64) >= a).all()):
        raise ValueError("a sensitivity beyond float16's range: %r" % (a,))
    return h


def half_to_float(u):
    return np.asarray(u, dtype=np.float16).astype(np.float64)


def in_range(J, Pref, B, sig):
    return bool((J * B / sig).max() <= 1e-3 * (1.0 + np.abs(Pref).max()))


def forward_bound(J, Pref, B, sig):
    return J * B / sig + 16.0 * EPS * np.abs(Pref).max()


def pose_difference(P, hi, lo):
    """|P - (hi + lo)| entry by entry, without losing lo: (P - hi) is exact or nearly so for nearby doubles."""
    return np.abs((P - hi) - lo)


def check_slots(slots):
    """Structure of the four pose slots of one sample: each all NaN or wholly finite, R orthonormal to 1e-9, det R > 0.
    Returns the list of the finite poses (12,)."""
    out = []
    for s in np.asarray(slots).reshape(4, 12):
        nan = np.isnan(s)
        assert nan.all() or (not nan.any() and np.isfinite(s).all()), "a slot is neither all NaN nor wholly finite: %r" % (s,)
        if nan.all():
            continue
        R = s.reshape(3, 4)[:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-9 and np.linalg.det(R) > 0
        out.append(s.copy())
    return out


def judge(got, refs, B, sig, rho, complete_needs_rho):
    """The forward rule on one problem.  got: the returned poses (12,), refs: list of dict(hi, lo, J, in_range).  Returns
    (missed, spurious, worst): the in-range reference solutions with no returned pose within the bound (counted only where
    rho >= RHO_CAP when complete_needs_rho), the returned poses within the bound of no reference solution, and the worst ratio
    difference / bound among the matches."""
    missed, spurious, worst = 0, 0, 0.0
    bounds = [forward_bound(r["J"], r["hi"], B, sig) for r in refs]
    for r, bd in zip(refs, bounds):
        if not r["in_range"] or (complete_needs_rho and rho < RHO_CAP):
            continue
        ratios = [float((pose_difference(g, r["hi"], r["lo"]) / bd).max()) for g in got]
        if not ratios or min(ratios) > 1.0:
            missed += 1
        else:
            worst = max(worst, min(ratios))
    for g in got:
        if not any((pose_difference(g, r["hi"], r["lo"]) <= bd).all() for r, bd in zip(refs, bounds)):
            spurious += 1
    return missed, spurious, worst


_REFS = {}


def class_table(fx, name):
    """(X, x, K, [per problem: dict(B, sigma, rho, refs=[dict(hi, lo, J, in_range)])]) of a stored class; the reference poses are
    rebuilt from the stored depths once per session."""
    if name not in _REFS:
        import p3p_mp
        X, x, K = class_inputs(name, fx)
        table = []
        for i, (sig, rho, sols) in enumerate(class_references(fx, name)):
            refs = []
            for s in sols:
                hi, lo, _ = p3p_mp.pose_from_stored_depths(X[i], x[i], K, s["s_hi"], s["s_lo"])
                refs.append(dict(hi=np.array(hi), lo=np.array(lo), J=s["J"], in_range=s["in_range"]))
            table.append(dict(B=bound_B(x[i], K), sigma=sig, rho=rho, refs=refs if rho >= 0 else None))   # rho < 0: never certified
        _REFS[name] = (X, x, K, table)
    return _REFS[name]


def evaluate(name, slots, fx=None, table=None):
    """Both rules over one class.  slots: (n, 4, 12) pose slots, one row of four per problem.  Returns the figures the tests assert on
    and print: worst backward error (px, and as a multiple of B / sigma), missed / spurious counts, worst forward ratio."""
    import p3p_mp
    if table is None:
        X, x, K, table = class_table(fx, name)
    else:
        X, x, K, table = table
    out = dict(poses=0, refs=0, backward_px=0.0, backward_ratio=0.0, missed=0, spurious=0, forward_ratio=0.0)
    for i, row in enumerate(table):
        got = check_slots(slots[i])
        out["poses"] += len(got)
        for g in got:
            be = p3p_mp.backward_error(g, X[i], x[i], K)
            out["backward_px"] = max(out["backward_px"], be)
            out["backward_ratio"] = max(out["backward_ratio"], be * row["sigma"] / row["B"])
        if row["refs"] is not None:
            out["refs"] += len(row["refs"])
            m, s, w = judge(got, row["refs"], row["B"], row["sigma"], row["rho"], name in HARD)
            out["missed"] += m; out["spurious"] += s; out["forward_ratio"] = max(out["forward_ratio"], w)
    return out


def reference_problem(X, x, K):
    """dict(sigma, rho, sols=[dict(s_hi, s_lo, J (float16), in_range, hi, lo)]) or None when the case never certifies."""
    import p3p_mp
    from mpmath import mp, mpf
    try:
        ref = p3p_mp.solve(X, x, K)
        sig = float(p3p_mp.sigma(X))
        B = bound_B(x, K)
        sols = []
        for s in ref["sols"]:
            J16 = half_up(np.array([float(j) for j in p3p_mp.sensitivity(X, x, K, s, ref["dps"])]))
            J = half_to_float(J16)
            s_hi, s_lo = p3p_mp.hi_lo(s["s"])
            s_lo = np.array(s_lo, dtype=np.float32)
            hi, lo, _ = p3p_mp.pose_from_stored_depths(X, x, K, s_hi, s_lo)
            with mp.workdps(p3p_mp.DPS):
                off = max(abs(mpf(h) + mpf(l) - p) for h, l, p in zip(hi, lo, s["P"]))
            if float(off) > 1e-3 * 16.0 * EPS * max(abs(h) for h in hi):
                raise p3p_mp.NotCertified("float32 lo of the depths does not carry the pose: off by %.3g" % float(off))
            hi = np.array(hi)
            sols.append(dict(s_hi=np.array(s_hi), s_lo=s_lo, J=J16, in_range=in_range(J, hi, B, sig), hi=hi, lo=np.array(lo), Jf=J))
        return dict(sigma=sig, rho=float(ref["rho"]), sols=sols)
    except p3p_mp.NotCertified as e:
        print("    dropped: %s" % e)
        return None


_REPORT = {}
N_REPORT_REF = 12


def report_table(name):
    """(X, x, K, table) of a report-only class; the first N_REPORT_REF problems get a reference, solved here once per session (about
    a tenth of a second each), so that missed and spurious poses can be counted over them; the backward error covers all of the class."""
    if name not in _REPORT:
        X, x, K = class_inputs(name)
        table = []
        for i in range(len(X)):
            r = reference_problem(X[i], x[i], K) if i < N_REPORT_REF else None
            table.append(dict(B=bound_B(x[i], K), sigma=sigma_float(X[i]), rho=r["rho"] if r else 0.0,
                              refs=[dict(hi=s["hi"], lo=s["lo"], J=s["Jf"], in_range=s["in_range"]) for s in r["sols"]] if r else None))
        _REPORT[name] = (X, x, K, table)
    return _REPORT[name]

"""The seven-point / four-point case table (inputs, by deterministic construction) and the two rules a float64 solver is held to
against the high-precision reference (tests/twoview_mp.py, fixture tests/golden/twoview_reference.npz written by
tools/make_twoview_reference.py).  DESIGN.md section 11 derives the rules; in short, on models in the coordinates conditioned by
the image size, scaled to unit Frobenius norm:

  backward   'F': zero the model's smallest singular value at 60 digits; the worst, over the sample, of the smaller of the two point-to-
             epipolar-line distances, in pixels.  'H': the worst |x2 - H x1| in pixels.  Rule: backward error <= bound_i =
             4096 * max(2^-53 max(w, h), r_ref_i), r_ref_i the worst backward error of the problem's reference solutions rounded entry
             by entry to float64 (the floor any float64 model can reach on that problem; measured on the reference alone).
  forward    every in-range reference solution (J bound_i <= 1e-3) has a returned model within J_k bound_i + 16 * 2^-53 in all nine
             entries, and every returned model lies within that bound of some reference solution: none missed, none spurious.  In the
             hard classes completeness is asked only where rho >= 1e-3.

Every class is a pool of POOL correspondences and N_PER_CLASS samples of uint8 indices into it.
'F' asserted: exact, noisy (0.5 px), vga (0.5 px at 640 x 480), puretrans (R = I).  'F' hard: nearplanar (within 1e-3 of a plane,
relative to depth), smallbase (baseline 1e-3 of the mean depth), neardouble (samples of the exact pool searched for rho in [1e-6, 1e-3]).
'H' asserted: exact, noisy, vga.  'H' hard: collinear (three of the four collinear to 1e-3 of their span), tinyquad (the four within
10 px of each other), corners (the four within 2 px of the image corners).

The five-point solver ('E', coloc_amd/csrc/fivept.h and fivept_wave.h) has the same reference and the same two rules
(tests/golden/fivept_reference.npz).  Asserted: exact, noisy, smallrot (rotation 1e-3 rad).  Hard: smallbase (1e-3), forward (motion
along the optical axis), nearplanar, far (depth 50 to 60).  K = [1000 0 640; 0 1000 360; 0 0 1] for both cameras, models in calibrated
coordinates.  'E' has no rho: completeness is asked of every in-range solution of every class.
"""
import os

import numpy as np

N_PER_CLASS = 30
POOL = 24
RHO_CAP = 1e-3
EPS = 2.0 ** -53
ASSERTED = {"F": ["exact", "noisy", "vga", "puretrans"], "H": ["exact", "noisy", "vga"]}
HARD = {"F": ["nearplanar", "smallbase", "neardouble"], "H": ["collinear", "tinyquad", "corners"]}
ASSERTED["E"], HARD["E"] = ["exact", "noisy", "smallrot"], ["smallbase", "forward", "nearplanar", "far"]
REPORT = {"F": [], "H": [], "E": []}
STORED_E = ["exact", "noisy", "smallbase", "forward", "nearplanar", "far", "smallrot"]      # (the order of FIXTURE_E's classes)
MODELS = ["F", "H"]                                 # (the models of FIXTURE; 'E' has FIXTURE_E)
M_OF = {"F": 7, "H": 4, "E": 5}
SLOTS = {"F": 3, "H": 1, "E": 10}
K_E = np.array([[1000.0, 0.0, 640.0], [0.0, 1000.0, 360.0], [0.0, 0.0, 1.0]])
POOL_OF = {("F", "neardouble"): "exact"}            # (classes that draw from another class's pool)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twoview_reference.npz")
FIXTURE_E = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fivept_reference.npz")
_SEED = {"exact": 1, "noisy": 2, "vga": 3, "puretrans": 4, "nearplanar": 5, "smallbase": 6, "neardouble": 7, "collinear": 8, "tinyquad": 9,
         "corners": 10, "forward": 11, "far": 12, "smallrot": 13}


def classes(model):
    return ASSERTED[model] + HARD[model] + REPORT[model]


def stored_classes(model):
    """The classes in the order their fixture keeps them."""
    return STORED_E if model == "E" else classes(model)


def all_classes():
    return [(m, c) for m in MODELS for c in classes(m)]


def class_offset(model, name):
    """Index of the class's first problem in its fixture's per-problem arrays."""
    return (STORED_E.index(name) if model == "E" else all_classes().index((model, name))) * N_PER_CLASS


def pool_names(model):
    return [c for c in stored_classes(model) if (model, c) not in POOL_OF]


def image_size(name):
    return (640, 480) if name == "vga" else (1280, 720)


def camera(model, name):
    """What the solver's entry takes besides the pixels: the image size ('F', 'H': conditioning), K of both cameras ('E')."""
    return K_E if model == "E" else image_size(name)


def _rodrigues(ax):
    th = np.linalg.norm(ax)
    if th == 0.0:
        return np.eye(3)
    k = ax / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def pool(model, name):
    """(POOL, 4) float64: x1 (u, v), x2 (u, v) in pixels."""
    name = POOL_OF.get((model, name), name)
    rng = np.random.default_rng(1000 * (1 + "FHE".index(model)) + _SEED[name])
    wh = image_size(name)
    f = 1000.0 * wh[0] / 1280.0
    K = np.array([[f, 0.0, wh[0] / 2.0], [0.0, f, wh[1] / 2.0], [0.0, 0.0, 1.0]])
    Ki = np.linalg.inv(K)
    R = np.eye(3) if name == "puretrans" else _rodrigues((1e-3 if name == "smallrot" else 0.15) * rng.uniform(-1, 1, 3))
    t = rng.uniform(-1, 1, 3) * np.array([0.8, 0.5, 0.3])
    if name == "forward":
        t = np.array([0.0, 0.0, 0.8])
    if name == "smallbase":
        t *= 1e-3 * 7.0 / np.linalg.norm(t)
    normal = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0])
    dist = 7.0
    planar = model == "H" or name == "nearplanar"
    if name == "collinear":                     # POOL / 3 triples: the third point off the line of the first two by 1e-3 of their span
        u = []
        while len(u) < POOL:
            a = np.array([rng.uniform(100, wh[0] - 100), rng.uniform(100, wh[1] - 100)])
            ph = rng.uniform(0, 2 * np.pi)
            L = rng.uniform(150.0, 300.0)
            dr = np.array([np.cos(ph), np.sin(ph)])
            lam = rng.uniform(0.3, 0.7)
            b = a + L * dr
            if 0.0 <= b[0] <= wh[0] and 0.0 <= b[1] <= wh[1]:
                u += [a, b, a + lam * L * dr + 1e-3 * L * np.array([-dr[1], dr[0]])]
        u = np.array(u)
    elif name == "tinyquad":                    # POOL / 6 clusters of six points in a 7 x 7 px square: any two within 10 px
        u = np.concatenate([np.array([rng.uniform(100, wh[0] - 100), rng.uniform(100, wh[1] - 100)]) + rng.uniform(0.0, 7.0, (6, 2))
                            for _ in range(POOL // 6)])
    elif name == "corners":                     # POOL / 4 points within 2 px of each corner, inside the image
        cs = np.array([[0.0, 0.0], [wh[0], 0.0], [0.0, wh[1]], [wh[0], wh[1]]])
        u = np.concatenate([c + np.where(c > 0, -1.0, 1.0) * rng.uniform(0.0, 1.4, (POOL // 4, 2)) for c in cs])
    else:
        u = None
    out = []
    k = 0
    while len(out) < POOL:
        p = u[k] if u is not None else np.array([rng.uniform(40, wh[0] - 40), rng.uniform(40, wh[1] - 40)])
        k += 1
        ray = Ki @ np.array([p[0], p[1], 1.0])
        z = dist / (ray @ normal) if planar else (rng.uniform(50.0, 60.0) if name == "far" else rng.uniform(4.0, 10.0))
        if name == "nearplanar":
            z *= 1.0 + 1e-3 * rng.uniform(-1, 1)
        Y = K @ (R @ (ray * z) + t)
        q = Y[:2] / Y[2]
        if u is None and not (0 <= q[0] <= wh[0] and 0 <= q[1] <= wh[1]):
            continue
        out.append([p[0], p[1], q[0], q[1]])
    out = np.array(out)
    if name in ("noisy", "vga"):
        out = out + rng.normal(0.0, 0.5, out.shape)
    return np.ascontiguousarray(out)


def rho_float(q1, q2):
    """float64 estimate of rho for a batch of conditioned seven-point samples (B, 7, 2): only the search for the neardouble class uses it
    (the generator measures the rho it stores at 60 digits)."""
    u1, v1, u2, v2 = q1[..., 0], q1[..., 1], q2[..., 0], q2[..., 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1)
    Vh = np.linalg.svd(A, full_matrices=True)[2]
    a, b = Vh[:, 7].reshape(-1, 3, 3), Vh[:, 8].reshape(-1, 3, 3)
    c0, c3, p1, m1 = np.linalg.det(a), np.linalg.det(b), np.linalg.det(a + b), np.linalg.det(a - b)
    c2, c1 = 0.5 * (p1 + m1) - c0, 0.5 * (p1 - m1) - c3
    nrm = np.sqrt(c0 * c0 + c1 * c1 + c2 * c2 + c3 * c3)
    c0, c1, c2, c3 = c0 / nrm, c1 / nrm, c2 / nrm, c3 / nrm
    disc = 18 * c3 * c2 * c1 * c0 - 4 * c2 ** 3 * c0 + c2 * c2 * c1 * c1 - 4 * c3 * c1 ** 3 - 27 * c3 * c3 * c0 * c0
    rho = np.ones(len(A))
    for i in np.nonzero(np.abs(disc) < 1e-5)[0]:
        r = np.roots([c3[i], c2[i], c1[i], c0[i]])
        if len(r) == 3:
            rho[i] = min(abs(r[j] - r[k]) / np.sqrt((1 + abs(r[j]) ** 2) * (1 + abs(r[k]) ** 2)) for j in range(3) for k in range(j))
    return rho


def samples(model, name):
    """(N_PER_CLASS, m) uint8 indices into the class's pool."""
    m = M_OF[model]
    rng = np.random.default_rng(2000 * (1 + "FHE".index(model)) + _SEED[name])
    if name == "collinear":                     # a triple and one point of another triple
        out = []
        for i in range(N_PER_CLASS):
            tr = i % (POOL // 3)
            other = rng.choice([j for j in range(POOL) if j // 3 != tr])
            out.append(rng.permutation([3 * tr, 3 * tr + 1, 3 * tr + 2, other]))
        return np.array(out, dtype=np.uint8)
    if name == "tinyquad":                      # four of one cluster
        return np.array([6 * (i % (POOL // 6)) + rng.choice(6, 4, replace=False) for i in range(N_PER_CLASS)], dtype=np.uint8)
    if name == "corners":                       # one point per corner
        return np.array([rng.permutation([c * (POOL // 4) + rng.integers(POOL // 4) for c in range(4)]) for i in range(N_PER_CLASS)], dtype=np.uint8)
    if name == "neardouble":                    # (margins inside [1e-6, 1e-3]: the float estimate decides membership only away from the ends)
        p = pool(model, name)
        w, h = image_size(name)
        d = 1.0 / np.sqrt(float(w * h))
        q = (p - np.array([w / 2.0, h / 2.0, w / 2.0, h / 2.0])) * d
        out = []
        while len(out) < N_PER_CLASS:
            idx = np.argsort(rng.random((20000, POOL)), axis=1)[:, :7]
            rho = rho_float(q[idx][..., :2], q[idx][..., 2:])
            for i in np.nonzero((rho > 2e-6) & (rho < 5e-4))[0]:
                if len(out) < N_PER_CLASS and not any(set(idx[i]) == set(o) for o in out):
                    out.append(idx[i])
        return np.array(out, dtype=np.uint8)
    return np.stack([rng.choice(POOL, m, replace=False) for _ in range(N_PER_CLASS)]).astype(np.uint8)


def load_fixture(model="F"):
    with np.load(FIXTURE_E if model == "E" else FIXTURE) as z:
        return {k: z[k] for k in z.files}


def class_inputs(model, name, fx=None):
    """(x1 (n, m, 2), x2 (n, m, 2), camera) in pixels; from the fixture `fx` when it is given, else rebuilt."""
    if fx is not None:
        p = fx[model + "_pool"][pool_names(model).index(POOL_OF.get((model, name), name))]
        s = fx[model + "_samples"][stored_classes(model).index(name)].astype(np.int64)
    else:
        p, s = pool(model, name), samples(model, name).astype(np.int64)
    return np.ascontiguousarray(p[s][..., :2]), np.ascontiguousarray(p[s][..., 2:]), camera(model, name)


def flat_inputs(model, name, fx=None):
    """The class as one call of a batched solver takes it: (x1 (n m, 2), x2 (n m, 2), wh, samples (n, m) int32)."""
    x1, x2, wh = class_inputs(model, name, fx)
    n, m = x1.shape[:2]
    return x1.reshape(-1, 2), x2.reshape(-1, 2), wh, np.arange(n * m, dtype=np.int32).reshape(n, m)


J_SCALE = 64.0


def half_up(a):
    """float64 -> the next float16 at or above a / J_SCALE: the fixture keeps the sensitivities J in this form, two bytes each.  The
    scale puts the largest J that can be in range (1e-3 / bound = 3.4e6 at 640 x 480) inside the format; above 6e-5 J_SCALE the stored
    value is at most 0.1 % high, below it at most 6e-8 J_SCALE = 4e-6 high, which moves a forward bound by less than its rounding term.
    A value beyond the format becomes inf: that solution is out of range."""
    a = np.asarray(a, dtype=np.float64) / J_SCALE
    with np.errstate(over="ignore"):
        h = a.astype(np.float16)
        h = np.where(h.astype(np.float64) < a, np.nextafter(h, np.float16(np.inf)), h).astype(np.float16)
    if not (h.astype(np.float64) >= a).all():
        raise ValueError("a sensitivity not rounded up: %r" % (a,))
    return h


def half_to_float(u):
    return np.asarray(u, dtype=np.float16).astype(np.float64) * J_SCALE


def bound(wh, r_ref):
    return 4096.0 * max(EPS * max(wh), float(r_ref))


def in_range(J, bd):
    return bool((J * bd).max() <= 1e-3)


def forward_bound(J, bd):
    return J * bd + 16.0 * EPS


def class_references(fx, model, name):
    """Per problem of a class: (rho, r_ref, [dict(M (9,), J (9,), in_range)])."""
    lo = class_offset(model, name)
    out = []
    for i in range(lo, lo + N_PER_CLASS):
        rws = np.nonzero(fx["sol_prob"] == i)[0]
        out.append((float(fx["rho"][i]) if "rho" in fx else 1.0, float(fx["r_ref"][i]),
                    [dict(M=fx["M"][r].astype(np.float64), J=half_to_float(fx["J"][r]), in_range=bool(fx["in_range"][r])) for r in rws]))
    return out


def unit(M, like=None):
    """Unit Frobenius norm; the sign that agrees with `like` (a model is a ray: where two entries tie for the largest, the sign rule
    of the reference is followed, not re-decided), else the largest entry positive."""
    M = np.asarray(M, dtype=np.float64).reshape(9)
    M = M / np.linalg.norm(M)
    if like is not None:
        return M if M @ like > 0 else -M
    return M if M[np.argmax(np.abs(M))] > 0 else -M


def check_slots(slots, ordered=True):
    """Structure of one sample's model slots: each all NaN or wholly finite, and (`ordered`: the seven-point and four-point entries) NaN
    slots only after the finite ones.  Returns the finite models (9,)."""
    out, ended = [], False
    for s in np.asarray(slots).reshape(-1, 9):
        nan = np.isnan(s)
        assert nan.all() or (not nan.any() and np.isfinite(s).all()), "a slot is neither all NaN nor wholly finite: %r" % (s,)
        if nan.all():
            ended = True
            continue
        assert not (ended and ordered), "a model after an empty slot"
        out.append(s.copy())
    return out


def judge(got, refs, bd, rho, complete_needs_rho):
    """The forward rule on one problem.  got: the returned models (9,), refs: list of dict(hi, lo, J, in_range).  Returns
    (missed, spurious, worst ratio difference / bound among the matches, pairs): pairs[j] is the reference solution returned model j
    matched best, None for a spurious one."""
    missed, spurious, worst = 0, 0, 0.0
    bounds = [forward_bound(r["J"], bd) for r in refs]
    diffs = [[np.abs((unit(g, r["hi"]) - r["hi"]) - r["lo"]) for r in refs] for g in got]
    for k, (r, b) in enumerate(zip(refs, bounds)):
        if not r["in_range"] or (complete_needs_rho and rho < RHO_CAP):      # ('E' has no rho: class_references gives 1.0)
            continue
        ratios = [float((diffs[j][k] / b).max()) for j in range(len(got))]
        if not ratios or min(ratios) > 1.0:
            missed += 1
        else:
            worst = max(worst, min(ratios))
    pairs = []
    for j in range(len(got)):
        ok = [k for k, b in enumerate(bounds) if (diffs[j][k] <= b).all()]
        pairs.append(min(ok, key=lambda k: float((diffs[j][k] / bounds[k]).max())) if ok else None)
        spurious += 0 if ok else 1
    return missed, spurious, worst, pairs


_TABLES = {}
RECERT_STEPS = {"F": 2, "H": 2, "E": 4}
N_REPORT_REF = 15          # the tests would bring the references of this many problems of a report-only class back (30 ms a solution,
                           # five to a problem); no class is report only today


def class_table(fx, model, name):
    """(x1, x2, camera, [per problem: dict(bound, rho, refs=[dict(hi, lo, J, in_range, cert)])]) of a class; every stored solution is
    brought back to the certified one by Newton steps at 60 digits (two from a float64 model, four from a float32 one), once per session."""
    if (model, name) not in _TABLES:
        import twoview_mp
        x1, x2, cam = class_inputs(model, name, fx)
        table = []
        for i, (rho, r_ref, sols) in enumerate(class_references(fx, model, name)):
            refs = [] if (name not in REPORT[model] or i < N_REPORT_REF) else None
            for s in (sols if refs is not None else []):
                hi, lo, cert = twoview_mp.recertify(model, x1[i], x2[i], cam, s["M"], RECERT_STEPS[model])
                refs.append(dict(hi=np.array(hi), lo=np.array(lo), J=s["J"], in_range=s["in_range"], cert=float(cert)))
            table.append(dict(bound=bound(image_size(name), r_ref), rho=rho, refs=refs))
        _TABLES[(model, name)] = (x1, x2, cam, table)
    return _TABLES[(model, name)]


def evaluate(model, name, slots, fx=None, table=None):
    """Both rules over one class.  slots: (n, 3 | 1 | 10, 9) model slots (conditioned coordinates for 'F' and 'H', calibrated ones for
    'E'), NaN where a sample has fewer models.  Returns the figures the tests assert on and print; `doubled` counts the returned models
    that share their reference solution with another returned model of the same sample.  The backward error covers every problem;
    missed, spurious, doubled and the forward ratio the problems whose row carries references (all, but for the report-only classes
    in the tests: their first N_REPORT_REF)."""
    import twoview_mp
    x1, x2, cam, table = class_table(fx, model, name) if table is None else table
    out = dict(models=0, refs=0, backward_px=0.0, backward_median=0.0, backward_ratio=0.0, backward_at=-1, above_bound=0, missed=0, spurious=0,
               forward_ratio=0.0, doubled=0)
    bes = []
    for i, row in enumerate(table):
        got = check_slots(slots[i], ordered=model != "E")
        out["models"] += len(got)
        for g in got:
            be = twoview_mp.backward_error(model, g, x1[i], x2[i], cam)
            bes.append(be)
            out["above_bound"] += 1 if be > row["bound"] else 0
            if be / row["bound"] > out["backward_ratio"]:
                out["backward_ratio"], out["backward_at"] = be / row["bound"], i
        if row["refs"] is None:
            continue
        out["refs"] += len(row["refs"])
        m, s, w, pairs = judge(got, row["refs"], row["bound"], row["rho"], name in HARD[model])
        out["missed"] += m; out["spurious"] += s; out["forward_ratio"] = max(out["forward_ratio"], w)
        out["doubled"] += sum(1 for k in set(pairs) if k is not None and pairs.count(k) > 1)
    out["backward_px"], out["backward_median"] = (max(bes), float(np.median(bes))) if bes else (0.0, 0.0)
    return out


def reference_problem(model, x1, x2, cam, wh=(1280, 720)):
    """dict(rho, r_ref, sols=[dict(M (9; float64, float32 for 'E'), J (float16), Jf, in_range, hi, lo)]) of one sample, or None when it
    never certifies.  cam: the image size ('F', 'H') or K ('E', whose image size is `wh`)."""
    import twoview_mp
    try:
        ref = twoview_mp.solve_five(x1, x2, cam) if model == "E" else twoview_mp.solve(model, x1, x2, cam)
        wh = wh if model == "E" else cam
        his = [np.array(twoview_mp.hi_lo(s["M"])[0]) for s in ref["sols"]]
        r_ref = float(np.float32(max([twoview_mp.backward_error(model, h, x1, x2, cam) for h in his] + [0.0])))
        bd = bound(wh, r_ref)
        sols = []
        for s, h in zip(ref["sols"], his):
            J16 = half_up(np.array([float(j) for j in twoview_mp.sensitivity(model, x1, x2, cam, s, ref["dps"])]))
            stored = h.astype(np.float32) if model == "E" else h
            hi, lo, cert = twoview_mp.recertify(model, x1, x2, cam, stored.astype(np.float64), RECERT_STEPS[model])
            if cert > twoview_mp.CERT_TOL or not np.array_equal(np.array(hi), h):
                raise twoview_mp.NotCertified("the stored model does not lead back to the certified one: %.3g" % float(cert))
            J = half_to_float(J16)
            sols.append(dict(M=stored, J=J16, Jf=J, in_range=in_range(J, bd), hi=h, lo=np.array(lo), cert=float(cert)))
        return dict(rho=float(np.float32(float(ref["rho"]))), r_ref=r_ref, sols=sols)
    except twoview_mp.NotCertified as e:
        print("    dropped: %s" % e)
        return None

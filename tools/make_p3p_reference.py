#!/usr/bin/env python3
"""Write tests/golden/p3p_reference.npz: the P3P case table (tests/p3p_cases.py) solved by the high-precision reference
(tests/p3p_mp.py).  Nothing in it comes from a GPU or from the solver under test.

Stored, to stay below the largest fixture of tests/golden/: the inputs in float64 (the three random classes as a pool of scene points
and index triples), and per reference solution its three depths as float64 hi + float32 lo, the sensitivities J as float16 rounded
UP (at most 0.1 % above), and the in-range flag computed from the J that is stored.  The tests rebuild each reference pose from its
depths at 60 digits (the triads: no root finding); this tool checks that the rebuilt pose is the certified one to 1e-3 of the rounding
term of the forward bound before it stores a solution.  Per problem: sigma and rho.  The report-only classes are not stored.

Refuses to write when more than 5 % of an asserted class is out of range, or when the rho cap leaves out more than 25 % of a hard
class.  Prints, per class, the shares left out and what the host build of p3p.h scores under the two rules.

    python tools/make_p3p_reference.py            # writes the fixture
    python tools/make_p3p_reference.py --report   # also solves the report-only classes and prints their figures
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import p3p_cases as cases   # noqa: E402
import p3p_host             # noqa: E402
import p3p_mp               # noqa: E402
from mpmath import mp, mpf  # noqa: E402


reference_problem = cases.reference_problem


def host_slots(X, x, K):
    return np.stack([p3p_host.sample_poses(X[i], x[i], K, [0, 1, 2]).reshape(4, 12) for i in range(len(X))])


def build_branch_case(kind):
    """One problem that takes a guarded branch of p3p.h: a random camera, three pixels, the first two depths fixed, the third point moved
    along its ray until the guarded quantity vanishes at 50 digits; the world points are then rounded to float64.
      cubic        the quartic's leading coefficient co[4]
      biquadratic  the linear coefficient q of the depressed quartic
      den          D(v) at v = s3 / s1 of the solution the case is built around
    The first candidate (seeds in order) whose rounded problem the host build sends through the branch is kept.  For `den` that cannot
    be asked: where D vanishes at a solution the quartic has a double root there, the float root lands 1e-8 away and the guard is not
    reached; the first candidate whose polished root brings |D| below 1e-5 is kept, and the tests state that the
    guard is not taken."""
    K = cases.pool_scene()["K"]
    for seed in range(100, 400):
        rng = np.random.default_rng(seed)
        R = cases._random_rotation(rng)
        t = rng.uniform(-3.0, 3.0, 3)
        x = np.stack([rng.uniform(100.0, 1180.0, 3), rng.uniform(60.0, 660.0, 3)], 1)
        s01 = rng.uniform(6.0, 16.0, 2)
        with mp.workdps(50):
            f = p3p_mp.bearings(x, K)
            Q0 = [mpf(s01[0]) * e for e in f[0]]
            Q1 = [mpf(s01[1]) * e for e in f[1]]

            def quantity(lam):
                Q2 = [lam * e for e in f[2]]
                sides, cosines = p3p_mp.sides_and_cosines([Q0, Q1, Q2], f)
                co, N, D, W = p3p_mp.quartic(sides, cosines)
                if kind == "cubic":
                    return co[4]
                if kind == "den":
                    return p3p_mp._peval(D, lam / mpf(s01[0]))
                a, b, c = co[3] / co[4], co[2] / co[4], co[1] / co[4]
                return a ** 3 / 8 - a * b / 2 + c

            grid = [mpf(2) + mpf(k) * mpf(38) / 190 for k in range(191)]
            vals = [quantity(g) for g in grid]
            lam = None
            for k in range(190):
                if vals[k] * vals[k + 1] < 0:
                    lam = mp.findroot(quantity, (grid[k], grid[k + 1]), solver="anderson", tol=mpf(10) ** -90, verify=False)
                    if abs(quantity(lam)) < mpf(10) ** -40 and grid[k] <= lam <= grid[k + 1]:
                        break
                    lam = None
            if lam is None:
                continue
            Rm = [[mpf(float(R[i][j])) for j in range(3)] for i in range(3)]
            Xw = []
            for Q in (Q0, Q1, [lam * e for e in f[2]]):
                d = [Q[i] - mpf(float(t[i])) for i in range(3)]
                Xw.append([float(Rm[0][j] * d[0] + Rm[1][j] * d[1] + Rm[2][j] * d[2]) for j in range(3)])     # R^T (Q - t), rounded
        X = np.array(Xw)
        br = p3p_host.sample_branches(X, x, K, [0, 1, 2])
        taken = {"cubic": br["ok"] and not br["polish"], "biquadratic": br["ok"] and br["polish"] and br["biquadratic"],
                 "den": br["ok"] and br["polish"] and bool((np.abs(br["den"]) < 1e-5).any())}[kind]
        if taken:
            print("  %s: seed %d, third depth %s" % (kind, seed, mp.nstr(lam, 12)))
            return X[None], x[None], K
    raise RuntimeError("no %s case found" % kind)


def main():
    report = "--report" in sys.argv[1:]
    pool = cases.pool_scene()
    fx = dict(K=pool["K"], pool_X=pool["X"], pool_x=np.stack([pool["x_" + c] for c in cases.POOLED]),
              triples=np.stack([cases.pool_triples(c) for c in cases.POOLED]))
    con_X, con_x, sigma, rho = [], [], [], []
    sol = dict(sol_prob=[], s_hi=[], s_lo=[], J=[], in_range=[])
    figures = {}
    for name in cases.STORED + (cases.REPORT if report else []):
        print("class %s" % name)
        X, x, K = build_branch_case(name) if name in cases.BRANCH else cases.class_inputs(name)
        stored = name in cases.STORED
        if stored and name not in cases.POOLED:
            con_X.append(X); con_x.append(x)
        table, n_out, n_sol, n_rho, n_drop = [], 0, 0, 0, 0
        for i in range(len(X)):
            r = reference_problem(X[i], x[i], K)
            if r is None:
                n_drop += 1
                r = dict(sigma=cases.sigma_float(X[i]), rho=-1.0, sols=None)       # rho < 0 marks a case without a reference
            table.append(dict(B=cases.bound_B(x[i], K), sigma=r["sigma"], rho=r["rho"],
                              refs=None if r["sols"] is None else [dict(hi=s["hi"], lo=s["lo"], J=s["Jf"], in_range=s["in_range"]) for s in r["sols"]]))
            if stored:
                sigma.append(r["sigma"]); rho.append(r["rho"])
            for s in r["sols"] or []:
                n_sol += 1
                n_out += 0 if s["in_range"] else 1
                n_rho += 1 if (s["in_range"] and r["rho"] < cases.RHO_CAP) else 0
                if stored:
                    sol["sol_prob"].append(cases.class_offset(name) + i)
                    for k in ("s_hi", "s_lo", "J", "in_range"):
                        sol[k].append(s[k])
        fig = cases.evaluate(name, host_slots(X, x, K), table=(X, x, K, table))
        fig.update(out_of_range=n_out, below_rho_cap=n_rho, solutions=n_sol, dropped=n_drop)
        figures[name] = fig
        print("  problems %d, dropped %d, reference solutions %d, out of range %d (%.1f %%), in range below the rho cap %d (%.1f %%)"
              % (len(X), n_drop, n_sol, n_out, 100.0 * n_out / max(n_sol, 1), n_rho, 100.0 * n_rho / max(n_sol, 1)))
        print("  host build: poses %(poses)d, worst backward error %(backward_px).3g px = %(backward_ratio).3g x B/sigma, missed %(missed)d, "
              "spurious %(spurious)d, worst forward error %(forward_ratio).3g x bound" % fig)
        if name in cases.ASSERTED and (n_out > 0.05 * n_sol or n_drop):
            raise SystemExit("refusing to write: more than 5 %% of asserted class %s is out of range (or a case was dropped)" % name)
        if name in cases.HARD and n_rho > 0.25 * n_sol:
            raise SystemExit("refusing to write: the rho cap leaves out more than 25 %% of hard class %s" % name)
    fx.update(con_X=np.concatenate(con_X), con_x=np.concatenate(con_x), sigma=np.array(sigma), rho=np.array(rho, dtype=np.float32),
              sol_prob=np.array(sol["sol_prob"], dtype=np.int16), s_hi=np.array(sol["s_hi"]), s_lo=np.array(sol["s_lo"], dtype=np.float32),
              J=np.array(sol["J"], dtype=np.float16), in_range=np.array(sol["in_range"], dtype=bool))
    np.savez_compressed(cases.FIXTURE, **fx)
    size = os.path.getsize(cases.FIXTURE)
    golden = os.path.dirname(cases.FIXTURE)
    largest = max(os.path.getsize(os.path.join(golden, f)) for f in os.listdir(golden) if f != os.path.basename(cases.FIXTURE))
    print("wrote %s: %d bytes (largest other fixture: %d)" % (cases.FIXTURE, size, largest))
    if size > largest:
        raise SystemExit("the fixture is larger than the largest fixture already in tests/golden/")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Where the host build of the five-point solver (coloc_amd/csrc/fivept.h) loses a reference solution, per class of
tests/golden/fivept_reference.npz, and what each build variant scores under the two rules of DESIGN.md section 11.

A reference solution is lost where no returned model is within its forward bound (twoview_cases.judge).  Its coordinate in the
solver's own null-space basis is x* = c0 / c3 of the least-squares fit E_ref = c0 E1 + c1 E2 + c2 E3 + c3 E4; the eigenvalue
nearest to x* in chordal distance is the root that should have become it.  The first stage at which that root fails:

  unconverged   the eigenvalue iteration hit its sweep limit with this root still moving, and the root is judged complex or is
                further than 1e-3 (chordal) from x*
  complex       the root had stopped, and fpt_root_is_real says complex
  start         fpt_root_start found the 6 x 6 system singular
  polish        the root was real and started; after the polish its model is further than 1e-6 from the reference solution
  gate          the polished model is within 1e-6 of the reference solution and fpt_root_finish rejected it
  merged        valid, and fpt_compact dropped it as a duplicate
  inexact       returned, but outside the forward bound

    python tools/fivept_attribution.py                    # the table of the build as it is
    python tools/fivept_attribution.py study NULL_COMPLETE=0,ORTHO_BASIS=0 E_STEPS=1 SWEEPS=12 ...
                                                          # the rules per host build variant (-DFPT_<switch>, comma = together)
    python tools/fivept_attribution.py eig                # the eigenvalue stage's backward error per class, the solver's and LAPACK's
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fivept_host              # noqa: E402
import twoview_cases as cases   # noqa: E402

STAGES = ["unconverged", "complex", "start", "polish", "gate", "merged", "inexact"]


def chordal(a, b):
    if np.isinf(a):
        return 1.0 / np.sqrt(1.0 + abs(b) ** 2)
    return abs(a - b) / np.sqrt((1.0 + abs(a) ** 2) * (1.0 + abs(b) ** 2))


def is_real(z):
    return not abs(z.imag) > 1e-6 * (1.0 + abs(z.real))          # fpt_root_is_real


def stage_of(ws, ref):
    c = np.linalg.lstsq(ws["EE"].T, ref["hi"], rcond=None)[0]
    xs = c[0] / c[3] if c[3] != 0.0 else np.inf
    k = min(range(10), key=lambda j: chordal(xs, ws["z"][j]))
    small_e4 = abs(c[3]) < 1e-3 * np.linalg.norm(c)
    far = chordal(xs, ws["z"][k]) > 1e-3
    if not ws["zdone"][k] and (far or not is_real(ws["z"][k])):
        return "unconverged", small_e4
    if not is_real(ws["z"][k]):
        return "complex", small_e4
    if not ws["reached"][k][0]:
        return "start", small_e4
    last = max(s for s in range(3) if ws["reached"][k][s])
    x, y, z = ws["xyz"][k][last]
    E = x * ws["EE"][0] + y * ws["EE"][1] + z * ws["EE"][2] + ws["EE"][3]
    near = np.isfinite(E).all() and np.abs(cases.unit(E, ref["hi"]) - ref["hi"]).max() <= 1e-6
    if not ws["valid"][k]:
        return ("gate" if near else "polish"), small_e4
    returned = any(np.array_equal(ws["cand"][k], e.reshape(9)) for e in ws["E"])
    return ("inexact" if returned else "merged"), small_e4


def attribute(fx, name):
    x1, x2, K, table = cases.class_table(fx, "E", name)
    lost = dict((s, 0) for s in STAGES)
    n_small = 0
    for i, row in enumerate(table):
        ws = fivept_host.workspace(*fivept_host.normalised(x1[i], x2[i], K))
        got = [e.reshape(9) for e in ws["E"]]
        bounds = [cases.forward_bound(r["J"], row["bound"]) for r in row["refs"]]
        for r, b in zip(row["refs"], bounds):
            if any((np.abs((cases.unit(g, r["hi"]) - r["hi"]) - r["lo"]) <= b).all() for g in got):
                continue
            st, small = stage_of(ws, r)
            lost[st] += 1
            n_small += small
    return lost, n_small


def rules(fx, name):
    x1, x2, K = cases.class_inputs("E", name, fx)
    f = cases.evaluate("E", name, fivept_host.class_slots(x1, x2, K), fx)
    return "%d/%d %.2g (%.2g; %d) %d/%d" % (f["models"], f["refs"], f["backward_px"], f["backward_ratio"], f["above_bound"], f["missed"], f["spurious"])


def eig_errors(fx, name):
    """Worst sigma_min(A - x I) / |A|_2 at 60 digits over the real eigenvalues of the class's action matrices: (the solver's, LAPACK's)."""
    from mpmath import mp, mpf
    x1, x2, K = cases.class_inputs("E", name, fx)
    worst = [0.0, 0.0]
    with mp.workdps(60):
        for i in range(len(x1)):
            Ax = fivept_host.workspace(*fivept_host.normalised(x1[i], x2[i], K))["Ax"]
            A, norm2 = mp.matrix(Ax.tolist()), mpf(float(np.linalg.norm(Ax, 2)))
            mine = [z.real for z in fivept_host.eig(Ax)[0] if is_real(z)]
            theirs = [z.real for z in np.linalg.eigvals(Ax) if z.imag == 0.0]
            for w, xs in enumerate((mine, theirs)):
                for x in xs:
                    worst[w] = max(worst[w], float(mp.svd_r(A - mpf(float(x)) * mp.eye(10), compute_uv=False)[9] / norm2))
    return worst


def main():
    fx = cases.load_fixture("E")
    if sys.argv[1:2] == ["eig"]:
        for name in cases.STORED_E:
            print("%s: solver %.3g, LAPACK %.3g" % ((name,) + tuple(eig_errors(fx, name))), flush=True)
        return
    if sys.argv[1:2] == ["study"]:
        variants = [()] + [tuple(a.split(",")) for a in sys.argv[2:]]
        print("models / reference solutions; worst backward error px (x bound; models above their bound); missed / spurious")
        for v in variants:
            fivept_host.DEFINES = tuple("FPT_" + d for d in v)
            print("| %s | %s |" % (" ".join(v) or "as built", " | ".join(rules(fx, n) for n in cases.STORED_E)), flush=True)
        return
    print("| class | lost | " + " | ".join(STAGES) + " | of them with an E4 component under 1e-3 |")
    for name in cases.STORED_E:
        lost, n_small = attribute(fx, name)
        print("| %s | %d | %s | %d |" % (name, sum(lost.values()), " | ".join(str(lost[s]) for s in STAGES), n_small), flush=True)


if __name__ == "__main__":
    main()

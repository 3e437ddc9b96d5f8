#!/usr/bin/env python3
"""Write tests/golden/twoview_reference.npz and tests/golden/fivept_reference.npz: the seven-point / four-point / five-point case table (tests/twoview_cases.py) solved by the
high-precision reference (tests/twoview_mp.py).  Nothing in it comes from a GPU or from the solver under test.

Stored, to stay below the largest fixture of tests/golden/: per class a pool of correspondences in float64 and the samples as uint8
indices; per reference solution the nine entries of the unit-norm conditioned model as float64 (the tests bring each back to the
certified solution with two Newton steps at 60 digits; this tool checks that they do), the sensitivities J as float16 rounded UP and
the in-range flag computed from the J and the r_ref that are stored; per problem rho and r_ref as float32.

Conditions, checked on the reference alone before any solver runs: no problem dropped and no solution out of range in an asserted
class; at most 25 % of a hard class's reference solutions out of range or (in range and) under the rho cap.  The neardouble class
is under the cap by construction: there the condition is on the range alone.  The tool refuses to write otherwise.  It then prints what
the host build of twoview_min.h scores under the two rules.

The five-point classes ('E') go to tests/golden/fivept_reference.npz in the same layout, their models as float32 (the
tests take four Newton steps from them; this tool checks that those land on the certified solution) and without rho.

    python tools/make_twoview_reference.py [FH] [E]      # both files by default; about three and ten minutes
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import twoview_cases as cases   # noqa: E402
import twoview_host as tvh      # noqa: E402
import twoview_mp               # noqa: E402


def host_slots(model, x1, x2, cam):
    if model != "E":
        return tvh.class_slots(model, x1, x2, cam)
    import fivept_host
    return fivept_host.class_slots(x1, x2, cam)


def write(models, path):
    fx = {}
    for model in models:
        fx[model + "_pool"] = np.stack([cases.pool(model, c) for c in cases.pool_names(model)])
        fx[model + "_samples"] = np.stack([cases.samples(model, c) for c in cases.stored_classes(model)])
    rho, r_ref = [], []
    sol = dict(sol_prob=[], M=[], J=[], in_range=[])
    tables = {}
    for model, name in [(m, c) for m in models for c in cases.stored_classes(m)]:
        print("class %s %s" % (model, name))
        x1, x2, wh = cases.class_inputs(model, name)
        size = cases.image_size(name)
        table, n_out, n_cap, n_sol, n_drop, worst_cert = [], 0, 0, 0, 0, 0.0
        for i in range(len(x1)):
            r = cases.reference_problem(model, x1[i], x2[i], wh)
            if r is None:
                n_drop += 1
                r = dict(rho=-1.0, r_ref=0.0, sols=[])
            rho.append(r["rho"]); r_ref.append(r["r_ref"])
            table.append(dict(bound=cases.bound(size, r["r_ref"]), rho=r["rho"],
                              refs=[dict(hi=s["hi"], lo=s["lo"], J=s["Jf"], in_range=s["in_range"]) for s in r["sols"]]))
            for s in r["sols"]:
                n_sol += 1
                n_out += 0 if s["in_range"] else 1
                n_cap += 1 if (s["in_range"] and r["rho"] < cases.RHO_CAP) else 0
                worst_cert = max(worst_cert, s["cert"])
                sol["sol_prob"].append(cases.class_offset(model, name) + i)
                for k in ("M", "J", "in_range"):
                    sol[k].append(s[k])
        tables[(model, name)] = (x1, x2, wh, table)
        rhos = np.array([t["rho"] for t in table])
        print("  problems %d, dropped %d, reference solutions %d (worst certificate %.1e), out of range %d (%.1f %%), in range under the "
              "rho cap %d (%.1f %%); rho %.2e .. %.2e; r_ref up to %.2e px, bound %.2e .. %.2e px"
              % (len(x1), n_drop, n_sol, worst_cert, n_out, 100.0 * n_out / max(n_sol, 1), n_cap, 100.0 * n_cap / max(n_sol, 1), rhos.min(),
                 rhos.max(), max(r_ref[-len(x1):]), min(t["bound"] for t in table), max(t["bound"] for t in table)))
        if name in cases.ASSERTED[model] and (n_out or n_drop):
            raise SystemExit("refusing to write: asserted class %s %s has a dropped problem or a solution out of range" % (model, name))
        excluded = n_out + (0 if name == "neardouble" else n_cap)
        if name in cases.HARD[model] and (excluded > 0.25 * n_sol or n_drop):
            raise SystemExit("refusing to write: more than 25 %% of hard class %s %s is left out (or a case was dropped)" % (model, name))
        if name == "neardouble" and not ((rhos >= 1e-6) & (rhos <= 1e-3)).all():
            raise SystemExit("refusing to write: a neardouble sample has rho outside [1e-6, 1e-3]")
    fx.update(r_ref=np.array(r_ref, dtype=np.float32), sol_prob=np.array(sol["sol_prob"], dtype=np.int16),
              M=np.array(sol["M"]), J=np.array(sol["J"], dtype=np.float16), in_range=np.array(sol["in_range"], dtype=bool))
    if models != ["E"]:
        fx.update(rho=np.array(rho, dtype=np.float32))
    np.savez_compressed(path, **fx)
    size = os.path.getsize(path)
    print("wrote %s: %d bytes" % (path, size))
    if size > 74200:
        raise SystemExit("the fixture is larger than the largest fixture of tests/golden/ (74 200 bytes)")
    for (model, name), tb in tables.items():
        fig = cases.evaluate(model, name, host_slots(model, *tb[:3]), table=tb)
        print("host build, %s %s: models %d, backward error median %.3g worst %.3g px = %.3g x bound (problem %d; %d above their bound), missed "
              "%d, spurious %d, doubled %d, worst forward error %.3g x bound"
              % (model, name, fig["models"], fig["backward_median"], fig["backward_px"], fig["backward_ratio"], fig["backward_at"],
                 fig["above_bound"], fig["missed"], fig["spurious"], fig["doubled"], fig["forward_ratio"]))


def main():
    which = sys.argv[1:] or ["FH", "E"]
    if "FH" in which:
        write(cases.MODELS, cases.FIXTURE)
    if "E" in which:
        write(["E"], cases.FIXTURE_E)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Every output bit of the two pose Levenberg-Marquardt entries on the tests' own case tables, as hex, for comparing two builds of the
library (csrc/pose_lm.h is their one statement of the pass; profiles/pose_lm_once.txt is the comparison this was written for).

  clc_pnp_refine         over CASES of tests/test_gpu_pose_edges.py: from the perturbed start, from the true pose where the data is
                         exact, and under a byte mask that drops every third point -> Rt, cov, rmse, iterations
  clc_pnp_refine_prior   over tests/pose_prior_cases.py: the defaults, and huber_a = 2, rounds = 2, max_iter = 3, min_inliers = 5
                         -> Rt, cov, rmse, iterations, n_inliers, rounds_run, converged, result, mask
  both                   on the scenes of tests/test_gpu_track_prior.py::test_prior_with_every_track_in_equals_the_refine

Run it once per library, each run a process of its own (COLOC_HIP_LIB selects the library), and compare the two files byte for byte.
usage: tools/dump_pose_bits.py out.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import pose_prior_cases as pc  # noqa: E402
import test_gpu_pose_edges as pe  # noqa: E402
import test_gpu_track_prior as tp  # noqa: E402
from coloc_amd import Context  # noqa: E402


def hx(v):
    return np.ascontiguousarray(v).tobytes().hex()


def refine_line(what, r):
    Rt, cov, rmse, it = r
    return "%s Rt %s cov %s rmse %s iterations %d" % (what, hx(Rt), hx(cov), hx(np.float64(rmse)), it)


def prior_line(what, r):
    return "%s Rt %s cov %s rmse %s iterations %d n_inliers %d rounds_run %d converged %d result %d mask %s" % (
        what, hx(r["Rt"]), hx(r["cov"]), hx(np.float64(r["rmse"])), r["iterations"], r["n_inliers"], r["rounds_run"], r["converged"],
        r["result"], hx(r["mask"].astype(np.uint8)))


def main():
    out_path = sys.argv[1]
    ctx = Context(device=0, detector=False, matcher=False)
    lines = []
    for seed, case in enumerate(pe.CASES):
        cid, kname, rname, n, noise, outliers, huber = case
        K, R = pe.KS[kname], pe.ROTS[rname]
        X, x, Rt_true = pe.scene(K, R, n, noise, outliers, 7000 + seed)
        start = pe.perturbed(Rt_true, seed)
        if noise == 0.0:
            lines.append(refine_line("refine %s true" % cid, ctx.pnp_refine(X, x, K, Rt_true, huber_a=huber)))
        lines.append(refine_line("refine %s" % cid, ctx.pnp_refine(X, x, K, start, huber_a=huber, max_iter=50)))
        mask = (np.arange(n) % 3 != 1).astype(np.uint8)
        lines.append(refine_line("refine %s masked" % cid, ctx.pnp_refine(X, x, K, start, mask=mask, huber_a=huber, max_iter=50)))
    for cid in pc.IDS:
        c = pc.build(cid)
        lines.append(prior_line("prior %s" % cid, ctx.pnp_refine_prior(c["X"], c["x"], c["K"], c["Rt_prior"], pc.GATE, huber_a=pc.HUBER)))
        lines.append(prior_line("prior %s step" % cid, ctx.pnp_refine_prior(c["X"], c["x"], c["K"], c["Rt_prior"], pc.GATE, huber_a=2.0, rounds=2,
                                                                         max_iter=3, min_inliers=5)))
    for n in tp.AGREE_NS:
        X, x, K, start = tp._agree_scene(n)
        lines.append(refine_line("agree %d refine" % n, ctx.pnp_refine(X, x, K, start, huber_a=tp.AGREE_HUBER)))
        lines.append(prior_line("agree %d prior" % n, ctx.pnp_refine_prior(X, x, K, start, tp.AGREE_GATE, huber_a=tp.AGREE_HUBER, rounds=1,
                                                                         min_inliers=4)))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d records -> %s" % (len(lines), out_path))


if __name__ == "__main__":
    main()

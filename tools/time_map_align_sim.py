#!/usr/bin/env python3
"""The map align step under the a-contrario similarity (clc_map_align_sim_dev: rows + sweep, the 3-D pair gather, the solve's rounds and
refit, the transform) beside clc_map_align_dev (rows + sweep, one align launch) on the same context, report only, for n_old = n_new =
2 000 and 10 000 with half the rows common and a fifth of those wrong, in one process and run.

Device events on the context's own stream around batches of warm calls, the two alternating batch by batch after a settle of both (both
calls wait for their pinned records, so an event pair brackets whole calls).  The figure to report is the ADDED latency against
clc_map_align_dev in the same run: the step buys correctness (profiles are records, not gates).  Before a time is taken the new call
is checked against the host statement (tests/sim3_host.py) at the small size.
usage: tools/time_map_align_sim.py [out.txt]   (default profiles/map_align_sim.txt; the text also goes to stdout)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sim3_cases  # noqa: E402
import sim3_host as sh  # noqa: E402
from coloc_amd import Context  # noqa: E402

SIZES = (2000, 10000)


def case(n, seed):
    """n old and n new rows, n / 2 of them common (near-copies, 4 flipped bits); the new map = the old one under s = 2.5, 0.1 rad and a
    translation, a fifth of the common landmarks replaced by far-away points"""
    rng = np.random.default_rng(seed)
    new_desc = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    old_desc = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    q = np.sort(rng.choice(n, n // 2, replace=False))
    t = rng.permutation(n)[: n // 2]
    d = new_desc[t].copy()
    for _ in range(4):
        d[np.arange(len(d)), rng.integers(0, 64, len(d))] ^= (1 << rng.integers(0, 8, len(d))).astype(np.uint8)
    old_desc[q] = d
    new_X = np.stack([rng.uniform(-5, 5, n), rng.uniform(-3, 3, n), rng.uniform(6, 20, n)], 1)
    old_X = np.stack([rng.uniform(-5, 5, n), rng.uniform(-3, 3, n), rng.uniform(6, 20, n)], 1) * 2.5
    old_X[q] = 2.5 * new_X[t] @ sim3_cases.rot([0.3, -1.0, 0.5], 0.1).T + [3.0, -2.0, 5.0] + rng.normal(0, 0.01, (len(q), 3))
    wrong = q[rng.random(len(q)) < 0.2]
    old_X[wrong] += rng.uniform(10, 30, (len(wrong), 3))
    match = np.full(n, -1, dtype=np.int32)
    match[q] = t
    return dict(n=n, old_desc=old_desc, old_X=old_X, new_desc=new_desc, new_X=new_X, match=match, n_wrong=len(wrong))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "map_align_sim.txt")
    dev = torch.device("cuda", 0)
    lines = ["map align under the a-contrario similarity against clc_map_align_dev, report only, %s" % torch.cuda.get_device_name(0),
             "device events on the context's stream, 20 batches of 10 warm calls each, alternating, after 30 calls of both; one run"]
    for n in SIZES:
        c = case(n, 40 + n)
        ctx = Context(device=0, maxkp=n, detector=False)
        ctx.set_map(c["old_desc"])
        ctx.set_map_points(c["old_X"])
        d_desc, d_X = torch.from_numpy(c["new_desc"]).to(dev), torch.from_numpy(c["new_X"]).to(dev)
        torch.cuda.synchronize()
        calls = {"sim": lambda: ctx.map_align_sim_dev(d_desc.data_ptr(), d_X.data_ptr(), n, install=False, apply=sh.APPLY_FULL, seed=3, want_match=False, want_X=False),
                 "plain": lambda: ctx.map_align_dev(d_desc.data_ptr(), d_X.data_ptr(), n, install=False, want_match=False, want_X=False)}
        got, plain = calls["sim"](), calls["plain"]()
        assert got["n_common"] == plain["n_common"] == n // 2, "the sweep did not find the planted common features"
        if n == SIZES[0]:
            want = sh.map_align_sim(c["old_X"], c["new_X"], c["match"], apply=sh.APPLY_FULL, seed=3)
            assert got["n_inliers"] == want["n_inliers"] and got["s"] == want["s"] and np.array_equal(got["inlier"], want["inlier"]), "differs from the host statement"
        s = torch.cuda.ExternalStream(ctx.stream, device=dev)
        for _ in range(30):
            for f in calls.values():
                f()
        s.synchronize()
        per = {k: [] for k in calls}
        batch, rounds = 10, 20
        for r in range(rounds):
            for k in (("sim", "plain") if r % 2 == 0 else ("plain", "sim")):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(batch):
                    calls[k]()
                b.record(s)
                b.synchronize()
                per[k].append(a.elapsed_time(b) * 1e3 / batch)
        med = {k: float(np.median(v)) for k, v in per.items()}
        lines.append("n_old = n_new = %d, %d common features of which %d wrong: similarity s %.6f (planted 2.5), %d inliers, %d iterations, refit %d; mean of ratios %.6f"
                     % (n, got["n_common"], c["n_wrong"], got["s"], got["n_inliers"], got["iterations"], got["refit"], plain["scale"]))
        for k in ("sim", "plain"):
            v = per[k]
            what = "clc_map_align_sim_dev: rows + sweep, pair gather, rounds + refit, transform" if k == "sim" else "clc_map_align_dev"
            lines.append("  %-5s us per call: median %.1f  min %.1f  max %.1f   (%s)" % (k, med[k], min(v), max(v), what))
        lines.append("  added latency (medians): %+.1f us" % (med["sim"] - med["plain"]))
        ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

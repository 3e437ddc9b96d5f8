#!/usr/bin/env python3
"""The map match through a cell grid (clc_match_map_binned_dev: prep launch + bin launch + match launch) beside the guided sweep
(clc_match_map_guided_dev: prep launch + gated popcount sweep) and clc_match_map_dev on the same context (whatever formulation it runs by
default) for 10k queries against 2 000 and 10 000 map rows, in one process and run.  The inputs are tools/time_map_guided.py's.

Device events on one stream around batches of warm calls, the three legs rotating batch by batch after a settle of a few hundred calls of
each (clocks up, code objects loaded); the spread of the batches is reported with the medians.  Before a time is taken the binned result
is checked: against the host statement (tests/proj_host.py) at 2k x 2k, and at each timed size against clc_match_map_guided_dev, match,
best and second, bit for bit.  The rows a query visits and its candidates come from the statement's side (tests/bin_host.py).

THE CONDITION the binned entry is held to (include in whatever quotes this file): at 10 000 rows EVERY batch of the binned entry is below
EVERY batch of the guided entry; at 2 000 rows its median is below the guided median.  The last lines say whether it holds.
usage: tools/time_map_binned.py [out.txt]   (default profiles/map_binned.txt; the text also goes to stdout)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bin_host as bh  # noqa: E402
import guided_host as gh  # noqa: E402
import proj_host as ph  # noqa: E402
import synth  # noqa: E402
from coloc_amd import Context  # noqa: E402

NQ = 10000
MAPS = (2000, 10000)
RADIUS = 8.0
THR = 40
LEGS = ("binned", "guided", "plain")
WHAT = {"binned": "clc_match_map_binned_dev: prep + bin + match launch", "guided": "clc_match_map_guided_dev: prep launch + gated sweep",
        "plain": "clc_match_map_dev"}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "map_binned.txt")
    dev = torch.device("cuda", 0)
    ctx = Context(device=0, maxkp=NQ, detector=False)
    qpb = ctx.k2nn_plan_query(NQ, MAPS[-1])["queries_per_block"]
    formulation = {128: "popcount", 256: "matrix"}.get(qpb, "%d queries per block" % qpb)
    rng = np.random.default_rng(5)

    def inputs(nq, nm):
        Q, M = synth.planted_descriptors(nq, nm, seed=3000, frac=0.3, max_flip=60)
        qpos = np.column_stack([rng.uniform(0, gh.W, nq), rng.uniform(0, gh.H, nq)]).astype(np.float32)
        mpix = np.column_stack([rng.uniform(0, gh.W, nm), rng.uniform(0, gh.H, nm)])
        X = np.array([ph.landmark(x, y, z) for (x, y), z in zip(mpix, rng.uniform(2.0, 10.0, nm))])
        return Q, M, qpos, X

    def on_device(Q, M, qpos, X):
        ctx.set_map(M)
        ctx.set_map_points(X)
        n = len(Q)
        d = dict(q=torch.from_numpy(Q).to(dev), f=torch.from_numpy(qpos).to(dev), p=torch.empty(n, dtype=torch.int32, device=dev))
        for leg in ("binned", "guided"):
            d[leg] = dict(m=torch.empty(n, dtype=torch.int32, device=dev), b=torch.empty(n, dtype=torch.int16, device=dev),
                          s=torch.empty(n, dtype=torch.int16, device=dev))
        torch.cuda.synchronize()
        return d

    def around(leg, d, nq, radius, stream=None, full=False):
        o = d[leg]
        extra = dict(d_best=o["b"].data_ptr(), d_second=o["s"].data_ptr()) if full else {}
        getattr(ctx, "match_map_%s_dev" % leg)(stream, d_q=d["q"].data_ptr(), nq=nq, cam=gh.CAM_EXACT, Rt=ph.IDENTITY, radius=radius, threshold=THR,
                                               d_match=o["m"].data_ptr(), d_feat=d["f"].data_ptr(), feat_stride=2, **extra)

    # -- correctness first
    small = inputs(2000, 2000)
    ds = on_device(*small)
    assert ctx.map_binned_plan(gh.CAM_EXACT, RADIUS)["plan"] == bh.BINNED
    around("binned", ds, 2000, RADIUS)
    ctx.sync()
    st = ph.statement(small[0], small[1], small[3], ph.IDENTITY, RADIUS, THR, gh.CAM_EXACT, feat=small[2])
    assert np.array_equal(ds["binned"]["m"].cpu().numpy(), st["match"]), "binned map match differs from the statement at 2k x 2k"

    lines = ["map match through a cell grid against the guided sweep and clc_match_map_dev (%s formulation), %d queries, %s" % (formulation, NQ, torch.cuda.get_device_name(0)),
             "device events on one stream, 40 batches of 50 warm calls each per leg, the legs rotating, after 200 calls of each; one run"]
    holds = True
    for nm in MAPS:
        case = inputs(NQ, nm)
        d = on_device(*case)
        plan = ctx.map_binned_plan(gh.CAM_EXACT, RADIUS)
        assert plan["plan"] == bh.BINNED
        for leg in ("binned", "guided"):
            around(leg, d, NQ, RADIUS, full=True)
        ctx.match_map_dev(d["q"].data_ptr(), NQ, THR, d["p"].data_ptr())
        ctx.sync()
        for k in ("m", "b", "s"):
            assert np.array_equal(d["binned"][k].cpu().numpy(), d["guided"][k].cpu().numpy()), "binned map match differs from the guided entry (%s) at %d rows" % (k, nm)
        accepted = int((d["binned"]["m"].cpu().numpy() >= 0).sum())
        accepted_plain = int((d["p"].cpu().numpy() >= 0).sum())
        # what a query visits and what passes the gate, from the statement's side
        proj = ph.project(ph.IDENTITY, gh.CAM_EXACT, case[3])[0]
        rw, _, c = bh.grid(gh.CAM_EXACT, RADIUS)
        visited = bh.visited(case[2], proj, rw, c)
        r2 = ph.r2_of(RADIUS)
        sample = np.arange(0, NQ, 10)
        cand = np.array([ph.gate(case[2][q], proj, r2).sum() for q in sample])

        s = torch.cuda.Stream(device=dev)
        calls = {"binned": lambda: around("binned", d, NQ, RADIUS, s.cuda_stream), "guided": lambda: around("guided", d, NQ, RADIUS, s.cuda_stream),
                 "plain": lambda: ctx.match_map_dev(d["q"].data_ptr(), NQ, THR, d["p"].data_ptr(), s.cuda_stream)}
        for _ in range(200):
            for f in calls.values():
                f()
        s.synchronize()
        per = {k: [] for k in calls}
        batch, rounds = 50, 40
        for r in range(rounds):
            for i in range(3):
                k = LEGS[(r + i) % 3]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(batch):
                    calls[k]()
                b.record(s)
                b.synchronize()
                per[k].append(a.elapsed_time(b) * 1e3 / batch)
        med = {k: float(np.median(v)) for k, v in per.items()}
        lines.append("%d x %d map rows, radius %.1f px over a %d x %d image, cells of %.3f px, %d lanes per query, threshold %d; accepted: binned = guided %d, plain %d"
                     % (NQ, nm, RADIUS, gh.W, gh.H, c, plan["lanes_per_query"], THR, accepted, accepted_plain))
        lines.append("  rows visited per query: mean %.1f, max %d; candidates per query (every tenth query): mean %.2f, max %d"
                     % (visited.mean(), visited.max(), cand.mean(), cand.max()))
        for k in LEGS:
            v = per[k]
            lines.append("  %-7s us per call: median %.2f  min %.2f  max %.2f   (%s)" % (k, med[k], min(v), max(v), WHAT[k]))
        lines.append("  binned / guided (medians): %.3f   binned / plain (medians): %.3f" % (med["binned"] / med["guided"], med["binned"] / med["plain"]))
        if nm == MAPS[-1]:
            ok = max(per["binned"]) < min(per["guided"])
            lines.append("  condition at %d rows (every binned batch below every guided batch: max %.2f < min %.2f): %s"
                         % (nm, max(per["binned"]), min(per["guided"]), "holds" if ok else "FAILS"))
        else:
            ok = med["binned"] < med["guided"]
            lines.append("  condition at %d rows (binned median below the guided median: %.2f < %.2f): %s" % (nm, med["binned"], med["guided"], "holds" if ok else "FAILS"))
        holds = holds and ok
    lines.append("the condition %s" % ("holds at both sizes" if holds else "FAILS"))
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The map match guided by a predicted pose (clc_match_map_guided_dev: prep launch + gated popcount sweep) beside clc_match_map_dev on the
same context (whatever formulation it runs by default) for 10k queries against 2 000 and 10 000 map rows, in one process and run.

Device events on one stream around batches of warm calls, the two alternating batch by batch after a settle of a few hundred calls
of both (clocks up, code objects loaded); the spread of the batches is reported with the medians.  Before a time is taken the guided
result is checked: against the host statement (tests/proj_host.py) at 2k x 2k, and at each timed size against clc_match_map_dev under a
radius wider than the image (every row a candidate: the two must agree).  A record, not a gate.
usage: tools/time_map_guided.py [out.txt]   (default profiles/map_guided.txt; the text also goes to stdout)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import guided_host as gh  # noqa: E402
import proj_host as ph  # noqa: E402
import synth  # noqa: E402
from coloc_amd import Context  # noqa: E402

NQ = 10000
MAPS = (2000, 10000)
RADIUS = 8.0
THR = 40


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "map_guided.txt")
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
        d = dict(q=torch.from_numpy(Q).to(dev), f=torch.from_numpy(qpos).to(dev), m=torch.empty(len(Q), dtype=torch.int32, device=dev),
                 p=torch.empty(len(Q), dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        return d

    def guided(d, nq, radius, stream=None):
        ctx.match_map_guided_dev(stream, d_q=d["q"].data_ptr(), nq=nq, cam=gh.CAM_EXACT, Rt=ph.IDENTITY, radius=radius, threshold=THR,
                                 d_match=d["m"].data_ptr(), d_feat=d["f"].data_ptr(), feat_stride=2)

    # -- correctness first
    small = inputs(2000, 2000)
    ds = on_device(*small)
    guided(ds, 2000, RADIUS)
    ctx.sync()
    st = ph.statement(small[0], small[1], small[3], ph.IDENTITY, RADIUS, THR, gh.CAM_EXACT, feat=small[2])
    assert np.array_equal(ds["m"].cpu().numpy(), st["match"]), "guided map match differs from the statement at 2k x 2k"

    lines = ["map match guided by a predicted pose against clc_match_map_dev (%s formulation), %d queries, %s" % (formulation, NQ, torch.cuda.get_device_name(0)),
             "device events on one stream, 40 batches of 50 warm calls each, alternating, after 200 calls of both; one run"]
    for nm in MAPS:
        d = on_device(*inputs(NQ, nm))
        guided(d, NQ, 4000.0)
        ctx.match_map_dev(d["q"].data_ptr(), NQ, THR, d["p"].data_ptr())
        ctx.sync()
        assert np.array_equal(d["m"].cpu().numpy(), d["p"].cpu().numpy()), "guided map match under an all-inclusive radius differs from clc_match_map_dev"
        guided(d, NQ, RADIUS)
        ctx.sync()
        accepted_guided, accepted_plain = int((d["m"].cpu().numpy() >= 0).sum()), int((d["p"].cpu().numpy() >= 0).sum())

        s = torch.cuda.Stream(device=dev)
        calls = {"guided": lambda: guided(d, NQ, RADIUS, s.cuda_stream),
                 "plain": lambda: ctx.match_map_dev(d["q"].data_ptr(), NQ, THR, d["p"].data_ptr(), s.cuda_stream)}
        for _ in range(200):
            for f in calls.values():
                f()
        s.synchronize()
        per = {k: [] for k in calls}
        batch, rounds = 50, 40
        for r in range(rounds):
            for k in (("guided", "plain") if r % 2 == 0 else ("plain", "guided")):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                for _ in range(batch):
                    calls[k]()
                b.record(s)
                b.synchronize()
                per[k].append(a.elapsed_time(b) * 1e3 / batch)
        med = {k: float(np.median(v)) for k, v in per.items()}
        lines.append("%d x %d map rows, radius %.1f px over a %d x %d image (about %.1f candidates per query), threshold %d; accepted: guided %d, plain %d"
                     % (NQ, nm, RADIUS, gh.W, gh.H, nm * np.pi * RADIUS * RADIUS / (gh.W * gh.H), THR, accepted_guided, accepted_plain))
        for k in ("guided", "plain"):
            v = per[k]
            what = "clc_match_map_guided_dev: prep launch + gated sweep" if k == "guided" else "clc_match_map_dev"
            lines.append("  %-7s us per call: median %.2f  min %.2f  max %.2f   (%s)" % (k, med[k], min(v), max(v), what))
        lines.append("  guided / plain (medians): %.3f" % (med["guided"] / med["plain"]))
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

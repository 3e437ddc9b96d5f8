#!/usr/bin/env python3
"""The guided match (clc_match_guided_dev: prep launch + gated popcount sweep) at 10k x 10k beside the plain popcount sweep
(clc_match_2nn_dev on a context created with CLC_K2NN_FORMULATION=popcount), in one process and run.

Device events on one stream around batches of warm calls, the two alternating batch by batch after a settle of a few hundred calls
of both (clocks up, code objects loaded); the spread of the batches is reported with the medians.  Before a time is taken the guided
result is checked: against the host statement (tests/guided_host.py) at 2k x 2k, and at 10k x 10k against the plain sweep under a band
wider than the image (every row a candidate: the two must agree).  A record, not a gate.
usage: tools/time_guided_match.py [out.txt]   (default profiles/guided_match.txt; the text also goes to stdout)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["CLC_K2NN_FORMULATION"] = "popcount"

import numpy as np  # noqa: E402
import torch  # noqa: E402

import guided_host as gh  # noqa: E402
import synth  # noqa: E402
from coloc_amd import Context  # noqa: E402

N = 10000
BAND = 3.0
THR = 40


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "guided_match.txt")
    dev = torch.device("cuda", 0)
    ctx = Context(device=0, maxkp=N, detector=False)
    assert ctx.k2nn_plan_query(N, N)["queries_per_block"] == 128, "not a popcount context"
    rng = np.random.default_rng(5)

    def inputs(n):
        Q, T = synth.planted_descriptors(n, n, seed=3000, frac=0.3, max_flip=60)
        qpos = np.column_stack([rng.uniform(0, gh.W, n), rng.uniform(0, gh.H, n)]).astype(np.float32)
        tpos = np.column_stack([rng.uniform(0, gh.W, n), rng.uniform(0, gh.H, n)]).astype(np.float32)
        return Q, T, qpos, tpos

    def on_device(Q, T, qpos, tpos):
        d = dict(q=torch.from_numpy(Q).to(dev), t=torch.from_numpy(T).to(dev), fa=torch.from_numpy(qpos).to(dev), fb=torch.from_numpy(tpos).to(dev),
                 m=torch.empty(len(Q), dtype=torch.int32, device=dev), p=torch.empty(len(Q), dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        return d

    def guided(d, n, band, stream=None):
        ctx.match_guided_dev(stream, d_q=d["q"].data_ptr(), nq=n, d_t=d["t"].data_ptr(), nt=n, cam_a=gh.CAM_EXACT, cam_b=gh.CAM_EXACT, F=gh.F_ROWS,
                             band=band, threshold=THR, d_match=d["m"].data_ptr(), d_feat_a=d["fa"].data_ptr(), feat_stride_a=2,
                             d_feat_b=d["fb"].data_ptr(), feat_stride_b=2)

    # -- correctness first
    small = inputs(2000)
    ds = on_device(*small)
    guided(ds, 2000, BAND)
    ctx.sync()
    st = gh.statement(small[0], small[1], gh.F_ROWS, BAND, THR, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=small[2], feat_b=small[3])
    assert np.array_equal(ds["m"].cpu().numpy(), st["match"]), "guided match differs from the statement at 2k x 2k"
    big = inputs(N)
    d = on_device(*big)
    guided(d, N, 4000.0)
    ctx.match_2nn_dev(d["q"].data_ptr(), N, d["t"].data_ptr(), N, THR, d["p"].data_ptr())
    ctx.sync()
    assert np.array_equal(d["m"].cpu().numpy(), d["p"].cpu().numpy()), "guided match under an all-inclusive band differs from the plain sweep"
    guided(d, N, BAND)
    ctx.sync()
    accepted_guided, accepted_plain = int((d["m"].cpu().numpy() >= 0).sum()), int((d["p"].cpu().numpy() >= 0).sum())

    # -- the two sweeps, alternating
    s = torch.cuda.Stream(device=dev)
    calls = {"guided": lambda: guided(d, N, BAND, s.cuda_stream),
             "popcount": lambda: ctx.match_2nn_dev(d["q"].data_ptr(), N, d["t"].data_ptr(), N, THR, d["p"].data_ptr(), s.cuda_stream)}
    for _ in range(200):
        for f in calls.values():
            f()
    s.synchronize()
    per = {k: [] for k in calls}
    batch, rounds = 50, 40
    for r in range(rounds):
        for k in (("guided", "popcount") if r % 2 == 0 else ("popcount", "guided")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(batch):
                calls[k]()
            b.record(s)
            b.synchronize()
            per[k].append(a.elapsed_time(b) * 1e3 / batch)
    ctx.close()
    med = {k: float(np.median(v)) for k, v in per.items()}
    lines = ["guided match against the plain popcount sweep, %d x %d, %s" % (N, N, torch.cuda.get_device_name(0)),
             "band %.1f px over a %d x %d image (about %.0f candidates per query), threshold %d; accepted: guided %d, plain K2NN %d"
             % (BAND, gh.W, gh.H, N * 2 * BAND / gh.H, THR, accepted_guided, accepted_plain),
             "device events on one stream, %d batches of %d warm calls each, alternating, after 200 calls of both" % (rounds, batch)]
    for k in ("guided", "popcount"):
        v = per[k]
        what = "clc_match_guided_dev: prep launch + gated sweep" if k == "guided" else "clc_match_2nn_dev, CLC_K2NN_FORMULATION=popcount"
        lines.append("%-9s us per call: median %.2f  min %.2f  max %.2f   (%s)" % (k, med[k], min(v), max(v), what))
    lines.append("guided / popcount (medians): %.3f" % (med["guided"] / med["popcount"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

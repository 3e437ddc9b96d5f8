#!/usr/bin/env python3
"""The distance-ratio matcher (CPUMatcher's rule) at 10k x 10k on the GPU, beside the K2NN sweep and the CPU oracle.

  1. clc_match_ratio_2nn_dev against clc_match_2nn_dev on the same pair: device events on one stream around batches of warm calls,
     the two rules alternating batch by batch (the spread of the batches is reported with the medians);
  2. host-buffer clc_match_ratio_pairs with positions, end to end (upload, sweep, download, host de-duplication): host clock around
     the synchronous call, warm, median / min;
  3. the CPU oracle on the same inputs: orc_cpumatcher_pair (sweep + both de-duplication passes, all host cores; the figure
     bench.py --full reports as cpu_baseline.openmvg_ratio_rule) and the ratio sweep alone (orc_k2nn_omp_timed, rule 1).
Every GPU result is checked against the oracle before a time is taken.  usage: tools/time_ratio_match.py [out.json] (JSON also on stdout)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle_lib  # noqa: E402
import synth  # noqa: E402
from coloc_amd import Context  # noqa: E402

N = 10000
RATIO = 0.8


def median(v):
    return float(np.median(np.asarray(v)))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    orc = oracle_lib.Oracle()
    Q, T = synth.planted_descriptors(N, N, seed=3000, frac=0.3, max_flip=60)
    rng = np.random.default_rng(3001)
    xy_t = rng.uniform(0, 640, size=(N, 2)).astype(np.float32)        # database = the train camera (pairs[p].first)
    xy_q = rng.uniform(0, 640, size=(N, 2)).astype(np.float32)
    ctx = Context(device=0, width=640, height=480, maxkp=N, detector=False)
    res = {"shape": [N, N], "ratio": RATIO, "device": torch.cuda.get_device_name(0)}

    # -- correctness first
    want_m, _ = orc.k2nn_omp(Q, T, rule=1, ratio=RATIO)
    want_p, _ = orc.cpumatcher_pair(T, xy_t, Q, xy_q, ratio=RATIO)
    assert np.array_equal(ctx.match_ratio(Q, T, RATIO), want_m), "match_ratio differs from the oracle"
    assert np.array_equal(ctx.match_ratio_pairs([T, Q], [(0, 1)], RATIO, xys=[xy_t, xy_q])[0], want_p), "match_ratio_pairs differs"
    res["accepted_queries"] = int((want_m >= 0).sum())
    res["pairs_after_dedup"] = int(want_p.shape[0])

    # -- 1. device sweeps, alternating
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    dq, dt = torch.from_numpy(Q).to(dev), torch.from_numpy(T).to(dev)
    dm = torch.empty(N, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    calls = {"ratio": lambda: ctx.match_ratio_dev(dq.data_ptr(), N, dt.data_ptr(), N, RATIO, dm.data_ptr(), st.cuda_stream),
             "k2nn": lambda: ctx.match_2nn_dev(dq.data_ptr(), N, dt.data_ptr(), N, 40, dm.data_ptr(), st.cuda_stream)}
    for _ in range(200):                                              # clocks up, code objects loaded
        for f in calls.values():
            f()
    st.synchronize()
    per = {k: [] for k in calls}
    batch, rounds = 50, 40
    for r in range(rounds):
        for k in (("ratio", "k2nn") if r % 2 == 0 else ("k2nn", "ratio")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(batch):
                calls[k]()
            b.record(st)
            b.synchronize()
            per[k].append(a.elapsed_time(b) * 1e3 / batch)
    calls["ratio"]()
    st.synchronize()
    assert np.array_equal(dm.cpu().numpy(), want_m), "match_ratio_dev differs from the oracle"
    for k, v in per.items():
        res["sweep_us_" + k] = {"median": median(v), "min": float(min(v)), "max": float(max(v)), "batches": rounds, "calls_per_batch": batch}
    res["ratio_over_k2nn_median"] = res["sweep_us_ratio"]["median"] / res["sweep_us_k2nn"]["median"]

    # -- 2. host-buffer pairs with positions, end to end
    for _ in range(5):
        ctx.match_ratio_pairs([T, Q], [(0, 1)], RATIO, xys=[xy_t, xy_q])
    ts = []
    for _ in range(30):
        t0 = time.perf_counter()
        ctx.match_ratio_pairs([T, Q], [(0, 1)], RATIO, xys=[xy_t, xy_q])
        ts.append((time.perf_counter() - t0) * 1e3)
    res["pairs_end_to_end_ms"] = {"median": median(ts), "min": float(min(ts)), "max": float(max(ts)), "calls": len(ts),
                                  "what": "clc_match_ratio_pairs, host buffers, positions, one pair: upload + sweep + download + de-duplication"}
    ts = []
    for _ in range(30):
        t0 = time.perf_counter()
        ctx.match_ratio(Q, T, RATIO)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["per_query_host_ms"] = {"median": median(ts), "min": float(min(ts)), "what": "clc_match_ratio_2nn, host buffers (no de-duplication)"}

    # -- 3. the CPU oracle on the same inputs
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        orc.cpumatcher_pair(T, xy_t, Q, xy_q, ratio=RATIO, kernel=0)
        ts.append((time.perf_counter() - t0) * 1e3)
    _, nthr, best = orc.k2nn_omp_timed(Q, T, rule=1, ratio=RATIO, kernel=0, reps=7)
    res["cpu_oracle"] = {"cpumatcher_pair_ms": {"median": median(ts), "min": float(min(ts))}, "ratio_sweep_only_ms_best": best * 1e3,
                         "threads": int(nthr), "cpu_count": os.cpu_count(),
                         "what": "orc_cpumatcher_pair (8 x popcount64 per pair, OpenMP over queries, then the de-duplication sort)"}
    ctx.close()
    line = json.dumps(res, indent=1)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of clc_match_2nn_dev alone for the library COLOC_HIP_LIB points to (A/B of two builds: alternate two such runs in one call),
at the shapes given as arguments, e.g. 10000x10000 8192x20000 9000x9000 (queries x train rows).  Per shape: 500 untimed launches first
(clock settling), then median / min of 200 event-bracketed launches, 2000 launches back to back under a host clock, and the number of
accepted matches plus a checksum of the match vector, so that two builds can be told to agree.  One JSON line."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, synth
from coloc_amd import Context
dev = torch.device("cuda", 0)
ctx = Context(device=0, width=640, height=480, maxkp=20000)
st = torch.cuda.Stream(device=dev); torch.cuda.set_stream(st)
out = {"lib": os.path.basename(os.environ.get("COLOC_HIP_LIB", "in tree"))}
for shape in sys.argv[1:]:
    nq, nt = (int(v) for v in shape.split("x"))
    Qh, Th = synth.planted_descriptors(nq, nt, seed=5)
    Q, T = torch.from_numpy(Qh).to(dev), torch.from_numpy(Th).to(dev)
    m = torch.empty(nq, dtype=torch.int32, device=dev)
    for _ in range(500): ctx.match_2nn_dev(Q.data_ptr(), nq, T.data_ptr(), nt, 40, m.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    ts = []
    for rep in range(200):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st); ctx.match_2nn_dev(Q.data_ptr(), nq, T.data_ptr(), nt, 40, m.data_ptr(), st.cuda_stream); b.record(st)
        b.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
    t0 = time.perf_counter()
    for _ in range(2000): ctx.match_2nn_dev(Q.data_ptr(), nq, T.data_ptr(), nt, 40, m.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    bb = (time.perf_counter() - t0) / 2000 * 1e6
    out[shape] = {"events_median_us": round(sorted(ts)[100], 3), "events_min_us": round(min(ts), 3), "back_to_back_us": round(bb, 3),
                  "accepted": int((m >= 0).sum()), "crc": int(m.to(torch.int64).mul(torch.arange(1, nq + 1, device=dev)).sum().item())}
print(json.dumps(out))
ctx.close()

"""The frame tail, from "d_match is ready on the device" to "pose and covariance on the host", two ways in one process and run:
  (a) today's path: matches and feature positions copied back, synchronisation, numpy gather, clc_pnp_localize_ac (bench_stream.py's solve_pose)
  (b) clc_track_localize_dev / clc_track_localize_batch_dev: tracks built on the device, the host waits for the track count only
at ~1 000 tracks among 1 600 queries, 30 % outliers, for one camera and for a batch of 8; p50 over FRAMES frames each.  The host leg is
timed TWICE (before and after the device leg): the difference between its two p50s is the run's noise.  Then the track
kernel alone (clc_track_build_dev between two events on a stream of its own).
usage: time_track_localize.py [frames]        both paths
       time_track_localize.py new [frames]    path (b) only -- the run to put under rocprofv3 --memory-copy-trace / --kernel-trace --stats"""
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch

import synth
from coloc_amd import Context, abi

only_new = len(sys.argv) > 1 and sys.argv[1] == "new"
args = [a for a in sys.argv[1:] if a != "new"]
FRAMES = int(args[0]) if args else 200
N, NB = 1000, 8
CAM = (1000.0, 640.0, 360.0, 0.0, 0.0, 0.0)
K = np.array([[1000.0, 0, 640.0], [0, 1000.0, 360.0], [0, 0, 1.0]])


def frame(seed, map_X, off):
    sc = synth.pnp_scene(N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    nq = int(1.6 * N)
    rows = off + rng.permutation(N)
    map_X[rows] = sc["X"]
    qs = np.sort(rng.choice(nq, N, replace=False))
    match = np.full(nq, -1, dtype=np.int32); match[qs] = rows
    feat = np.zeros((nq, 4), dtype=np.float32)
    feat[:, :2] = np.stack([rng.uniform(0, 1280, nq), rng.uniform(0, 720, nq)], 1)
    feat[qs, :2] = sc["x"]
    return match, feat


map_X = np.zeros((NB * N, 3))
frames = [frame(4000 + 10 * j, map_X, j * N) for j in range(NB)]
ctxs = [Context(device=0, detector=False, matcher=False) for _ in range(NB)]
ctxs[0].set_map_points(map_X)
dev = [(torch.from_numpy(m).cuda(), torch.from_numpy(f).cuda()) for m, f in frames]
torch.cuda.synchronize()


def old_inputs(j):
    m = dev[j][0].cpu().numpy()                    # copies + synchronisation
    f = dev[j][1].cpu().numpy()
    sel = np.nonzero(m >= 0)[0]
    return map_X[m[sel]], f[sel, :2].astype(np.float64)


def old_one(f):
    X, x = old_inputs(0)
    return ctxs[0].pnp_acransac(X, x, K, seed=f + 1, refine=True)


def old_batch(f):
    return abi.pnp_localize_batch(ctxs, [old_inputs(j) + (K,) for j in range(NB)], seeds=[f + 1 + j for j in range(NB)], refine=True)


def job(j, f):
    return dict(d_match=dev[j][0].data_ptr(), nq=len(frames[j][0]), cam=CAM, d_feat=dev[j][1].data_ptr(), feat_stride=4, seed=f + 1 + j, refine=True)


def new_one(f):
    return ctxs[0].track_localize_dev(**job(0, f))


def new_batch(f):
    return abi.track_localize_batch_dev(ctxs, [job(j, f) for j in range(NB)])


def p50(fn):
    t = []
    for f in range(FRAMES + 10):
        t0 = time.perf_counter()
        r = fn(f)
        t.append((time.perf_counter() - t0) * 1e6)
    t = np.sort(t[10:])
    return t[len(t) // 2], t[int(len(t) * 0.95)], r


print("frame tail, %d tracks among %d queries, p50 / p95 over %d frames (us); host leg timed twice, |a1 - a2| = the run's noise" % (N, len(frames[0][0]), FRAMES))
for what, old, new in (("1 camera  ", old_one, new_one), ("batch of %d" % NB, old_batch, new_batch)):
    if only_new:
        b, b95, r = p50(new)
        print("%s (b) device tracks p50 %8.1f  p95 %8.1f" % (what, b, b95))
        continue
    a1, a1_95, ra = p50(old)
    b, b95, rb = p50(new)
    a2, a2_95, _ = p50(old)
    ra0, rb0 = (ra[0], rb[0]) if isinstance(ra, list) else (ra, rb)
    noise = abs(a1 - a2)
    print("%s (a) host gather p50 %8.1f / %8.1f (p95 %8.1f / %8.1f)  (b) device tracks p50 %8.1f (p95 %8.1f)  noise %6.1f  "
          "b - min(a) %+8.1f  %s   inliers %d%s" % (what, a1, a2, a1_95, a2_95, b, b95, noise, b - min(a1, a2),
                                                    "not slower" if b <= min(a1, a2) + noise else "SLOWER", len(rb0["inliers"]),
                                                    "" if np.array_equal(ra0["inliers"], rb0["inliers"]) else "  (!! inliers differ)"))

# the track kernel alone: one launch between two events on a stream of its own
st = torch.cuda.Stream()
nq = len(frames[0][0])
d_X = torch.empty(3 * nq, dtype=torch.float64, device="cuda"); d_x = torch.empty(2 * nq, dtype=torch.float64, device="cuda")
d_q = torch.empty(nq, dtype=torch.int32, device="cuda"); d_m = torch.empty(nq, dtype=torch.int32, device="cuda")
d_n = torch.empty(4, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
ts = []
j0 = job(0, 0)
j0 = {k: j0[k] for k in ("d_match", "nq", "cam", "d_feat", "feat_stride")}
for it in range(FRAMES + 10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    ctxs[0].track_build_dev(d_X.data_ptr(), d_x.data_ptr(), d_q.data_ptr(), d_m.data_ptr(), d_n.data_ptr(), st.cuda_stream, **j0)
    e1.record(st)
    e1.synchronize()
    ts.append(e0.elapsed_time(e1) * 1e3)
ts = np.sort(ts[10:])
print("track kernel alone (event to event, one launch, %d queries -> %d tracks): p50 %.1f us" % (nq, int(d_n.cpu()[0]), ts[len(ts) // 2]))
for c in ctxs:
    c.close()

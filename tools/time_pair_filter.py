"""The pair filter, from "d_match is ready on the device" to "model and inliers on the host", two ways in one process and run:
  (a) today's path: matches and feature positions copied back, synchronisation, numpy gather and undistortion, clc_two_view_acransac
      (clc_two_view_acransac_batch for the batch)
  (b) clc_pair_filter_dev / clc_pair_filter_batch_dev: correspondences built on the device, the host waits for the pair count only
for each model 'E', 'F', 'H' at ~1 000 correspondences among 1 600 queries, ~30 % outliers, for one pair and for a batch of 8; p50 over PAIRS
calls each.  The host leg is timed TWICE (before and after the device leg): the difference between its two p50s is the run's noise.
Then the pair kernel alone (clc_pair_build_dev between two events on a stream of its own).
usage: time_pair_filter.py [pairs]        both paths
       time_pair_filter.py new [pairs]    path (b) only -- the run to put under rocprofv3 --memory-copy-trace / --kernel-trace --stats"""
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch

import track_host
import twoview_host
from coloc_amd import Context, abi

only_new = len(sys.argv) > 1 and sys.argv[1] == "new"
args = [a for a in sys.argv[1:] if a != "new"]
PAIRS = int(args[0]) if args else 200
N, NB = 1000, 8
W, H = 1280, 720
K = twoview_host.K_DEFAULT
CAM_A = (K[0, 0], K[0, 2], K[1, 2], -0.28, 0.07, 0.0)
CAM_B = (K[0, 0], K[0, 2], K[1, 2], 0.1, -0.02, 0.003)


def distort(x, cam):
    f, pp, k = cam[0], np.array(cam[1:3]), cam[3:6]
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


def pair(model, seed):
    sc = twoview_host.scene(N, seed, planar=(model == "H"))
    rng = np.random.default_rng(seed + 1)
    nq, nt = int(1.6 * N), int(1.3 * N)
    qs, rows = np.sort(rng.choice(nq, N, replace=False)), rng.choice(nt, N, replace=False)
    match = np.full(nq, -1, dtype=np.int32); match[qs] = rows
    fa = np.zeros((nq, 4), dtype=np.float32); fb = np.zeros((nt, 4), dtype=np.float32)
    fa[:, :2] = np.stack([rng.uniform(0, W, nq), rng.uniform(0, H, nq)], 1); fb[:, :2] = np.stack([rng.uniform(0, W, nt), rng.uniform(0, H, nt)], 1)
    fa[qs, :2] = distort(sc["x1"], CAM_A); fb[rows, :2] = distort(sc["x2"], CAM_B)
    return match, fa, fb


ctxs = [Context(device=0, detector=False, matcher=False) for _ in range(NB)]


def p50(fn):
    t = []
    for f in range(PAIRS + 10):
        t0 = time.perf_counter()
        r = fn(f)
        t.append((time.perf_counter() - t0) * 1e6)
    t = np.sort(t[10:])
    return t[len(t) // 2], t[int(len(t) * 0.95)], r


print("pair filter, %d correspondences among %d queries, p50 / p95 over %d pairs (us); host leg timed twice, |a1 - a2| = the run's noise" % (N, int(1.6 * N), PAIRS))
for model in "EFH":
    scenes = [pair(model, 7000 + 10 * j) for j in range(NB)]
    dev = [tuple(torch.from_numpy(a).cuda() for a in s) for s in scenes]
    torch.cuda.synchronize()

    def old_inputs(j):
        m = dev[j][0].cpu().numpy()                    # copies + synchronisation
        fa = dev[j][1].cpu().numpy()
        fb = dev[j][2].cpu().numpy()
        q = np.nonzero((m >= 0) & (m < len(fb)))[0]
        return (track_host.get_ud_pixel(fa[q, :2].astype(np.float64), CAM_A), track_host.get_ud_pixel(fb[m[q], :2].astype(np.float64), CAM_B))

    def old_one(f):
        x1, x2 = old_inputs(0)
        return ctxs[0].two_view_acransac(model, x1, x2, (W, H), K1=K, K2=K, seed=f + 1)

    def old_batch(f):
        return abi.two_view_acransac_batch(ctxs, model, [old_inputs(j) + (K, K, (W, H), f + 1 + j) for j in range(NB)])

    def job(j, f):
        return dict(d_match=dev[j][0].data_ptr(), nq=len(scenes[j][0]), nt=len(scenes[j][2]), cam_a=CAM_A, cam_b=CAM_B,
                    d_feat_a=dev[j][1].data_ptr(), d_feat_b=dev[j][2].data_ptr(), img_wh=(W, H), seed=f + 1 + j)

    def new_one(f):
        return ctxs[0].pair_filter_dev(model, **job(0, f))

    def new_batch(f):
        return abi.pair_filter_batch_dev(ctxs, model, [job(j, f) for j in range(NB)])

    for what, old, new in (("1 pair    ", old_one, new_one), ("batch of %d" % NB, old_batch, new_batch)):
        if only_new:
            b, b95, r = p50(new)
            print("'%s' %s (b) device pairs p50 %8.1f  p95 %8.1f" % (model, what, b, b95))
            continue
        a1, a1_95, ra = p50(old)
        b, b95, rb = p50(new)
        a2, a2_95, _ = p50(old)
        ra0, rb0 = (ra[0], rb[0]) if isinstance(ra, list) else (ra, rb)
        same = np.array_equal(ra0["inliers"], rb0["inliers"])
        noise = abs(a1 - a2)
        print("'%s' %s (a) host gather p50 %8.1f / %8.1f (p95 %8.1f / %8.1f)  (b) device pairs p50 %8.1f (p95 %8.1f)  noise %6.1f  "
              "b - min(a) %+8.1f  %s   inliers %d%s" % (model, what, a1, a2, a1_95, a2_95, b, b95, noise, b - min(a1, a2),
                                                        "not slower" if b <= min(a1, a2) + noise else "SLOWER", len(rb0["inliers"]),
                                                        "" if same else "  (!! inliers differ)"))

# the pair kernel alone: one launch between two events on a stream of its own
match, fa, fb = pair("E", 7000)
d_m, d_fa, d_fb = (torch.from_numpy(a).cuda() for a in (match, fa, fb))
st = torch.cuda.Stream()
nq = len(match)
d_x1 = torch.empty(2 * nq, dtype=torch.float64, device="cuda"); d_x2 = torch.empty(2 * nq, dtype=torch.float64, device="cuda")
d_q = torch.empty(nq, dtype=torch.int32, device="cuda"); d_t = torch.empty(nq, dtype=torch.int32, device="cuda")
d_n = torch.empty(4, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
ts = []
for it in range(PAIRS + 10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    ctxs[0].pair_build_dev(d_x1.data_ptr(), d_x2.data_ptr(), d_q.data_ptr(), d_t.data_ptr(), d_n.data_ptr(), st.cuda_stream, d_match=d_m.data_ptr(),
                           nq=nq, nt=len(fb), cam_a=CAM_A, cam_b=CAM_B, d_feat_a=d_fa.data_ptr(), d_feat_b=d_fb.data_ptr())
    e1.record(st)
    e1.synchronize()
    ts.append(e0.elapsed_time(e1) * 1e3)
ts = np.sort(ts[10:])
print("pair kernel alone (event to event, one launch, %d queries -> %d pairs): p50 %.1f us" % (nq, int(d_n.cpu()[0]), ts[len(ts) // 2]))
for c in ctxs:
    c.close()

"""The bundle adjustment of the grown map against the grown build without it, from "every pair's d_match is ready on the device" to "the
context serves the new map", two ways in one process and run on the same pairs:
  (a) clc_map_init_grow_ba_batch_dev: filters, tracks, seed triangulation, every other camera resected and its tracks added, then the
      valid cameras' poses and every landmark adjusted (map_ba.hip), the grown map installed
  (b) clc_map_init_grow_batch_dev: the same without the adjustment
for CAMS cameras x ROWS rows (every pair of cameras, ~70 % of the rows matched, 2 % of them wrongly); p50 / p95 over CALLS calls each after 3
warm-up calls.  Leg (b) is timed TWICE (before and after leg (a)): the difference between its two p50s is the run's noise.  (a) - (b) is
what the step costs: one pixel launch, the start's three launches and one wait, then per round of four iterations twenty launches and
one wait.  No figure is a pass criterion.  Appends the table to profiles/map_ba.txt (`new` as a fourth argument starts the file afresh).
usage: time_map_ba.py [cams [rows [calls [new]]]]"""
import itertools
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch

from coloc_amd import Context, abi

CAMS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ROWS = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
CALLS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
NEW = len(sys.argv) > 4 and sys.argv[4] == "new"
W, H = 1280, 720
F0 = (1000.0, 640.0, 360.0)
DIST = [(0.0, 0.0, 0.0), (-0.28, 0.07, 0.0), (0.1, -0.02, 0.003)]
K = np.array([[F0[0], 0, F0[1]], [0, F0[0], F0[2]], [0, 0, 1.0]])


def distort(x, cam):
    f, pp, k = cam[0], np.array(cam[1:3]), cam[3:6]
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


rng = np.random.default_rng(7)
X = np.stack([rng.uniform(-5, 5, ROWS), rng.uniform(-3, 3, ROWS), rng.uniform(8, 20, ROWS)], 1)
cams, point_of, feats, descs = [], [], [], []
base = rng.integers(0, 256, (ROWS, 64), dtype=np.uint8)
for c in range(CAMS):
    cam = F0 + DIST[c % 3]
    a = rng.uniform(-0.06, 0.06) if c else 0.0
    Rc = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Cc = np.array([0.8 * c, 0.0, 0.0])
    perm = rng.permutation(ROWS)
    u = ((X[perm] - Cc) @ Rc.T) @ K.T
    f = np.zeros((ROWS, 4), dtype=np.float32)
    f[:, :2] = distort(u[:, :2] / u[:, 2:3] + rng.normal(0, 0.3, (ROWS, 2)), cam)
    d = base[perm].copy()
    d[np.arange(ROWS), rng.integers(0, 64, ROWS)] ^= 1
    cams.append(cam); point_of.append(perm); feats.append(f); descs.append(d)
row_of = [np.argsort(p) for p in point_of]
pair_cams = list(itertools.combinations(range(CAMS), 2))
matches = []
for a, b in pair_cams:
    m = np.full(ROWS, -1, dtype=np.int32)
    q = rng.choice(ROWS, int(0.7 * ROWS), replace=False)
    m[q] = row_of[b][point_of[a][q]]
    wrong = q[rng.random(len(q)) < 0.02]
    m[wrong] = rng.integers(0, ROWS, len(wrong))
    matches.append(m)

d_match = [torch.from_numpy(m).cuda() for m in matches]
d_feat = [torch.from_numpy(f).cuda() for f in feats]
d_desc = [torch.from_numpy(d).cuda() for d in descs]
torch.cuda.synchronize()
# (a grown map can hold a landmark per track: room for half of all rows)
ctxs = [Context(device=0, width=W, height=H, maxkp=max(ROWS * CAMS // 2, ROWS), detector=False) for _ in pair_cams]
jobs = lambda s: [dict(d_match=d_match[k].data_ptr(), nq=ROWS, nt=ROWS, cam_a=cams[a], cam_b=cams[b], d_feat_a=d_feat[a].data_ptr(), feat_stride_a=4,
                       d_feat_b=d_feat[b].data_ptr(), feat_stride_b=4, img_wh=(W, H), seed=s + k) for k, (a, b) in enumerate(pair_cams)]
dc = [dict(cam=cams[i], d_feat=d_feat[i].data_ptr(), feat_stride=4, d_desc=d_desc[i].data_ptr()) for i in range(CAMS)]


def adjusted(f):
    return abi.map_init_grow_ba_batch_dev(ctxs, jobs(1 + f), [ROWS] * CAMS, pair_cams, dc, seed=1 + f)[0]


def grown(f):
    return abi.map_init_grow_batch_dev(ctxs, jobs(1 + f), [ROWS] * CAMS, pair_cams, dc, seed=1 + f)[0]


def p50(fn):
    t = []
    for f in range(CALLS + 3):
        t0 = time.perf_counter()
        r = fn(f)
        t.append((time.perf_counter() - t0) * 1e6)
    t = np.sort(t[3:])
    return t[len(t) // 2], t[int(len(t) * 0.95)], r


b1, b1_95, rb = p50(grown)
a, a95, ra = p50(adjusted)
b2, b2_95, _ = p50(grown)
ba = ra["ba"]
noise = abs(b1 - b2)
lines = ["map ba, %d cameras x %d rows, %d pairs, %d tracks; grown map %d rows; the step: status %d, %d iterations, %d cameras, %d points, %d observations, "
         "cost %.6g -> %.6g (rmse %.3f px); p50 / p95 over %d calls (us); leg (b) timed twice, |b1 - b2| = the run's noise"
         % (CAMS, ROWS, len(pair_cams), ra["n_tracks"], ra["map_n"], ba["status"], ba["iterations"], ba["n_cams"], ba["n_points"], ba["n_obs"],
            ba["cost_initial"], ba["cost_final"], ba["rmse"], CALLS),
         "(a) clc_map_init_grow_ba_batch_dev p50 %10.1f (p95 %10.1f)" % (a, a95),
         "(b) clc_map_init_grow_batch_dev    p50 %10.1f / %10.1f (p95 %10.1f / %10.1f)  noise %8.1f" % (b1, b2, b1_95, b2_95, noise),
         "a - min(b) %+10.1f   = %10.1f per iteration%s"
         % (a - min(b1, b2), (a - min(b1, b2)) / max(ba["iterations"], 1), "" if ra["map_n"] == rb["map_n"] else "   (!! the maps differ)")]
print("\n".join(lines))
os.makedirs(os.path.join(R, "profiles"), exist_ok=True)
with open(os.path.join(R, "profiles", "map_ba.txt"), "w" if NEW else "a") as fh:
    fh.write("\n".join(lines) + "\n")
for c in ctxs:
    c.close()

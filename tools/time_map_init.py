"""ColoC::initMap / updateMap between the putative matches and setMapData, from "every pair's d_match is ready on the device" to "the
context serves the new map", two ways in one process and run:
  (a) clc_map_init_batch_dev: filters, tracks, seed triangulation and map gather on the device
  (b) the path a caller has without it: clc_pair_filter_batch_dev, the match lists and inliers copied out, the chirality vote on the host,
      the Python statement of the tracks and the seed triangulation (tests/map_host.py over the host build of map_math.h), then
      clc_set_map + clc_set_map_points
for CAMS cameras x ROWS rows (every pair of cameras, ~70 % of the rows matched, 2 % of them wrongly); p50 over CALLS calls each after 3
warm-up calls.  Leg (b) is timed TWICE (before and after leg (a)): the difference between its two p50s is the run's noise.  Leg (b)'s
host part is Python, so the table also gives the share of it that is NOT the Python statement (filters + uploads): what a C++ host
would at least pay.  Writes the table to profiles/map_init.txt (the committed file is two runs, one after the other: `3 2000 20` and
`8 1500 5`).
usage: time_map_init.py [cams [rows [calls]]]"""
import itertools
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch

import inter_geometry_host
import map_host
from coloc_amd import Context, abi

CAMS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ROWS = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
CALLS = int(sys.argv[3]) if len(sys.argv) > 3 else 30
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
ctxs = [Context(device=0, width=W, height=H, maxkp=ROWS, detector=False) for _ in pair_cams]
jobs = lambda s: [dict(d_match=d_match[k].data_ptr(), nq=ROWS, nt=ROWS, cam_a=cams[a], cam_b=cams[b], d_feat_a=d_feat[a].data_ptr(), feat_stride_a=4,
                       d_feat_b=d_feat[b].data_ptr(), feat_stride_b=4, img_wh=(W, H), seed=s + k) for k, (a, b) in enumerate(pair_cams)]
dc = [dict(cam=cams[i], d_feat=d_feat[i].data_ptr(), feat_stride=4, d_desc=d_desc[i].data_ptr()) for i in range(CAMS)]
host_cams = [dict(cam=cams[i], feat=feats[i]) for i in range(CAMS)]
split = {"filter": [], "statement": [], "install": []}


def device_path(f):
    return abi.map_init_batch_dev(ctxs, jobs(1 + f), [ROWS] * CAMS, pair_cams, dc)[0]


def host_path(f):
    t0 = time.perf_counter()
    filt = abi.pair_filter_batch_dev(ctxs, "E", jobs(1 + f))
    t1 = time.perf_counter()
    pairs, votes, counts = [], [], []
    for (a, b), r in zip(pair_cams, filt):
        v = None
        if len(r["inliers"]) >= 13:
            v = inter_geometry_host.relative(np.ascontiguousarray(r["x1"]), np.ascontiguousarray(r["x2"]), K, np.ascontiguousarray(r["M"]),
                                             np.ascontiguousarray(r["inliers"], dtype=np.int32))
            v = v if v["stage"] == 0 else None
        votes.append(v)
        counts.append(len(r["inliers"]) if v is not None else 0)
        if v is not None:
            pairs.append(dict(cam_a=a, cam_b=b, q=r["pair_q"][r["inliers"]], t=r["pair_t"][r["inliers"]], of=len(votes) - 1))
    seed = int(np.argmax(counts))
    Rt_a, Rt_b = abi.seed_poses(np.eye(3), np.zeros(3), votes[seed]["R"], map_host.pose_center(votes[seed]["R"], votes[seed]["t"]), 1.0)
    m = map_host.build_map([ROWS] * CAMS, pairs, host_cams, [p["of"] for p in pairs].index(seed), Rt_a, Rt_b)
    t2 = time.perf_counter()
    ctxs[0].set_map(descs[pair_cams[seed][0]][m["map_row"]])
    ctxs[0].set_map_points(m["X"])
    t3 = time.perf_counter()
    split["filter"].append((t1 - t0) * 1e6); split["statement"].append((t2 - t1) * 1e6); split["install"].append((t3 - t2) * 1e6)
    return dict(map_n=len(m["map_track"]), n_tracks=len(m["track_feat"]), X=m["X"], map_row=m["map_row"])


def p50(fn):
    t = []
    for f in range(CALLS + 3):
        t0 = time.perf_counter()
        r = fn(f)
        t.append((time.perf_counter() - t0) * 1e6)
    t = np.sort(t[3:])
    return t[len(t) // 2], t[int(len(t) * 0.95)], r


b1, b1_95, rb = p50(host_path)
a, a95, ra = p50(device_path)
b2, b2_95, _ = p50(host_path)
same = ra["map_n"] == rb["map_n"] and np.array_equal(ra["map_row"], rb["map_row"]) and np.array_equal(ra["X"], rb["X"])
med = {k: float(np.median(v)) for k, v in split.items()}
noise = abs(b1 - b2)
lines = ["map initialisation, %d cameras x %d rows, %d pairs, %d tracks, %d map rows, p50 / p95 over %d calls (us); leg (b) timed twice, |b1 - b2| = the run's noise"
         % (CAMS, ROWS, len(pair_cams), ra["n_tracks"], ra["map_n"], CALLS),
         "(a) clc_map_init_batch_dev p50 %10.1f (p95 %10.1f)" % (a, a95),
         "(b) filters + host statement + set_map / set_map_points p50 %10.1f / %10.1f (p95 %10.1f / %10.1f)  noise %8.1f" % (b1, b2, b1_95, b2_95, noise),
         "    of (b): filters %10.1f  Python statement %10.1f  uploads %10.1f   (filters + uploads alone: %10.1f)" % (med["filter"], med["statement"], med["install"], med["filter"] + med["install"]),
         "a - min(b) %+10.1f   %s%s" % (a - min(b1, b2), "not slower" if a <= min(b1, b2) + noise else "SLOWER", "" if same else "   (!! results differ)")]
print("\n".join(lines))
os.makedirs(os.path.join(R, "profiles"), exist_ok=True)
with open(os.path.join(R, "profiles", "map_init.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
for c in ctxs:
    c.close()

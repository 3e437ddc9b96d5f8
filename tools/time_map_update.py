"""ColoC::updateMap from "every pair's d_match is ready on the device and the context serves the OLD map" to "the context serves the NEW
map at the old map's scale", two ways:
  (a) clc_map_update_batch_dev: filters, tracks, seed triangulation, old-against-new sweep, scale, rescale and install on the device
  (b) the host tail a caller has without it: clc_map_init_batch_dev on a second context set with host outputs, clc_match_2nn_dev old
      against new plus the download of the matches, the numpy scale (tests/map_update_host.py), clc_set_map + clc_set_map_points
for CAMS cameras x ROWS rows (every pair of cameras, ~70 % of the rows matched, 2 % of them wrongly); the old map is a third of camera
0's rows at 2.5 x the world's scale, installed anew (untimed) before every call of either leg.  p50 over CALLS calls each after 3 warm-up
calls; leg (b) is timed TWICE (before and after leg (a)): the difference between its two p50s is the run's noise.
Without arguments the two configurations (3 x 2 000, 20 calls; 8 x 1 500, 5 calls) run one after the other, each in a child process of
its own under a time limit, and the tables go to profiles/map_update.txt; a configuration that fails or runs out of time ends the run.
usage: time_map_update.py [cams rows calls]"""
import itertools
import os
import subprocess
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(R, "profiles", "map_update.txt")

if len(sys.argv) < 4:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    open(OUT, "w").close()
    for cfg in (("3", "2000", "20"), ("8", "1500", "5")):
        rc = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__)] + list(cfg)).returncode
        if rc != 0:
            sys.exit("configuration %s ended with status %d: nothing more is started" % (" ".join(cfg), rc))
    sys.exit(0)

sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch

import map_update_host as mu
from coloc_amd import Context, abi

CAMS, ROWS, CALLS = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
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
# the old map: a third of camera 0's rows (one more bit flipped), their points at 2.5 x the world's scale
old_rows = np.sort(rng.choice(ROWS, ROWS // 3, replace=False))
old_desc = descs[0][old_rows].copy()
old_desc[np.arange(len(old_rows)), rng.integers(0, 64, len(old_rows))] ^= 2
old_X = X[point_of[0][old_rows]] * 2.5

d_match = [torch.from_numpy(m).cuda() for m in matches]
d_feat = [torch.from_numpy(f).cuda() for f in feats]
d_desc = [torch.from_numpy(d).cuda() for d in descs]
d_old = torch.from_numpy(old_desc).cuda()
d_old_match = torch.full((len(old_rows),), -5, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
ctxs = [Context(device=0, width=W, height=H, maxkp=ROWS, detector=False) for _ in pair_cams]
jobs = lambda s: [dict(d_match=d_match[k].data_ptr(), nq=ROWS, nt=ROWS, cam_a=cams[a], cam_b=cams[b], d_feat_a=d_feat[a].data_ptr(), feat_stride_a=4,
                       d_feat_b=d_feat[b].data_ptr(), feat_stride_b=4, img_wh=(W, H), seed=s + k) for k, (a, b) in enumerate(pair_cams)]
dc = [dict(cam=cams[i], d_feat=d_feat[i].data_ptr(), feat_stride=4, d_desc=d_desc[i].data_ptr()) for i in range(CAMS)]
split = {"init": [], "match": [], "scale": [], "install": []}


def old_map():
    ctxs[0].set_map(old_desc)
    ctxs[0].set_map_points(old_X)


def device_path(f):
    r = abi.map_update_batch_dev(ctxs, jobs(1 + f), [ROWS] * CAMS, pair_cams, dc, scale=3.0)[0]
    return dict(map_n=r["map_n"], X=r["X"], scale=r["align"]["scale"], n_common=r["align"]["n_common"], match=r["align"]["match"])


def host_path(f):
    t0 = time.perf_counter()
    r = abi.map_init_batch_dev(ctxs, jobs(1 + f), [ROWS] * CAMS, pair_cams, dc, scale=3.0)[0]
    t1 = time.perf_counter()
    lower = pair_cams[r["seed_pair"]][0]
    d_new = d_desc[lower][torch.from_numpy(r["map_row"]).cuda().long()].contiguous()
    ctxs[0].match_2nn_dev(d_old.data_ptr(), len(old_rows), d_new.data_ptr(), r["map_n"], 60, d_old_match.data_ptr(), None)
    ctxs[0].sync()
    m = d_old_match.cpu().numpy()
    t2 = time.perf_counter()
    al = mu.align(old_X, r["X"], m)
    t3 = time.perf_counter()
    ctxs[0].set_map(descs[lower][r["map_row"]])
    ctxs[0].set_map_points(al["X"])
    t4 = time.perf_counter()
    for k, v in zip(("init", "match", "scale", "install"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
        split[k].append(v * 1e6)
    return dict(map_n=r["map_n"], X=al["X"], scale=al["scale"], n_common=al["n_common"], match=al["match"])


def p50(fn):
    t = []
    for f in range(CALLS + 3):
        old_map()
        t0 = time.perf_counter()
        r = fn(f)
        t.append((time.perf_counter() - t0) * 1e6)
    t = np.sort(t[3:])
    return t[len(t) // 2], t[int(len(t) * 0.95)], r


b1, b1_95, rb = p50(host_path)
a, a95, ra = p50(device_path)
b2, b2_95, _ = p50(host_path)
same = ra["map_n"] == rb["map_n"] and ra["scale"] == rb["scale"] and np.array_equal(ra["match"], rb["match"]) and np.array_equal(ra["X"], rb["X"])
med = {k: float(np.median(v)) for k, v in split.items()}
noise = abs(b1 - b2)
lines = ["map update, %d cameras x %d rows, %d pairs, %d old rows, %d new rows, %d common, scale %.6f, p50 / p95 over %d calls (us); leg (b) timed twice, |b1 - b2| = the run's noise"
         % (CAMS, ROWS, len(pair_cams), len(old_rows), ra["map_n"], ra["n_common"], ra["scale"], CALLS),
         "(a) clc_map_update_batch_dev p50 %10.1f (p95 %10.1f)" % (a, a95),
         "(b) clc_map_init_batch_dev + match_2nn_dev + download + numpy scale + set_map / set_map_points p50 %10.1f / %10.1f (p95 %10.1f / %10.1f)  noise %8.1f" % (b1, b2, b1_95, b2_95, noise),
         "    of (b): init %10.1f  gather + sweep + download %10.1f  scale %10.1f  uploads %10.1f" % (med["init"], med["match"], med["scale"], med["install"]),
         "a - min(b) %+10.1f   %s%s" % (a - min(b1, b2), "not slower" if a <= min(b1, b2) + noise else "SLOWER", "" if same else "   (!! results differ)")]
print("\n".join(lines))
with open(OUT, "a") as fh:
    fh.write("\n".join(lines) + "\n")
for c in ctxs:
    c.close()

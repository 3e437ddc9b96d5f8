"""The inter-camera step, from "d_match is ready on the device" to "pose + covariance on the host", two ways in one process and run:
  (a) clc_inter_pose_dev / clc_inter_pose_batch_dev: temporary map, scale and first pose on the device
  (b) the path a caller has without them: clc_pair_filter_dev / clc_pair_filter_batch_dev, then clc_inter_pose_batch fed from its host
      outputs (first_feature from pair_q, map_index from the map match copied back)
at ~1 000 correspondences among 1 600 queries, ~30 % outliers, through the reference's chain and through the shortcut, for one pair and for
a batch of 8; p50 over PAIRS calls each after 10 warm-up calls.  Leg (b) is timed TWICE (before and after leg (a)): the difference between
its two p50s is the run's noise.  Writes the table to profiles/inter_pose_dev.txt as well.
usage: time_inter_pose.py [pairs]        both paths
       time_inter_pose.py new [pairs]    path (a) only -- the run to put under rocprofv3 --kernel-trace --stats"""
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
PAIRS = int(args[0]) if args else 200
N, NB = 1000, 8
W, H = 1280, 720
K = np.array([[1000.0, 0, 640], [0, 1000.0, 360], [0, 0, 1]])
CAM_A = (1000.0, 640.0, 360.0, -0.28, 0.07, 0.0)
CAM_B = (1000.0, 640.0, 360.0, 0.1, -0.02, 0.003)


def rot(ax, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax]


def distort(x, cam):
    f, pp, k = cam[0], np.array(cam[1:3]), cam[3:6]
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


def noisy(rows, flips, rng):
    d = rows.copy()
    for _ in range(flips):
        b = rng.integers(0, 512, len(d))
        d[np.arange(len(d)), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return d


def world(seed):
    """one world, two cameras, N correspondences (30 % of the destination's replaced), a map of 60 % of the points; the pair of
    tests/test_gpu_inter_pose_dev.py"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-5, 5, N), rng.uniform(-5, 5, N), rng.uniform(6, 18, N)], 1)
    Rs, ts = rot("y", rng.uniform(-0.1, 0.1)) @ rot("x", rng.uniform(-0.05, 0.05)), rng.uniform(-0.3, 0.3, 3)
    Rd = rot("y", rng.uniform(0.1, 0.25)) @ rot("z", rng.uniform(-0.05, 0.05)) @ Rs
    td = ts + np.array([rng.uniform(0.6, 1.2), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])

    def proj(Rm, t):
        u = (X @ Rm.T + t) @ K.T
        return u[:, :2] / u[:, 2:3]
    x1, x2 = proj(Rs, ts) + rng.normal(0, 0.4, (N, 2)), proj(Rd, td) + rng.normal(0, 0.4, (N, 2))
    out = rng.choice(N, int(0.3 * N), replace=False)
    x2[out] = np.stack([rng.uniform(0, W, len(out)), rng.uniform(0, H, len(out))], 1)
    order = rng.permutation(np.nonzero(rng.random(N) < 0.6)[0])
    map_X = X[order] + rng.normal(0, 0.002, (len(order), 3))
    map_index = np.full(N, -1, np.int32); map_index[order] = np.arange(len(order), dtype=np.int32)
    nq, nt = int(1.6 * N), int(1.3 * N)
    qs, rows = np.sort(rng.choice(nq, N, replace=False)), rng.choice(nt, N, replace=False)
    match = np.full(nq, -1, dtype=np.int32); match[qs] = rows
    fa = np.zeros((nq, 4), dtype=np.float32); fb = np.zeros((nt, 4), dtype=np.float32)
    fa[:, :2] = np.stack([rng.uniform(0, W, nq), rng.uniform(0, H, nq)], 1); fb[:, :2] = np.stack([rng.uniform(0, W, nt), rng.uniform(0, H, nt)], 1)
    fa[qs, :2] = distort(x1, CAM_A); fb[rows, :2] = distort(x2, CAM_B)
    mm = np.full(nq, -1, dtype=np.int32); mm[qs] = map_index
    point = synth.random_descriptors(N, seed=seed + 1)
    desc_a, desc_map = synth.random_descriptors(nq, seed=seed + 2), synth.random_descriptors(len(order), seed=seed + 3)
    desc_a[qs] = noisy(point, 12, rng)
    desc_map[map_index[order]] = noisy(point[order], 10, rng)
    return dict(match=match, fa=fa, fb=fb, mm=mm, desc_a=desc_a, desc_map=desc_map), map_X, np.c_[Rs, ts]


host, map_X, Rt_source = world(8100)
dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
torch.cuda.synchronize()
ctxs = [Context(device=0, detector=False, matcher=False) for _ in range(NB)]
for c in ctxs:
    c.set_map_points(map_X)


def p50(fn):
    t = []
    for f in range(PAIRS + 10):
        t0 = time.perf_counter()
        r = fn(f)
        t.append((time.perf_counter() - t0) * 1e6)
    t = np.sort(t[10:])
    return t[len(t) // 2], t[int(len(t) * 0.95)], r


def pair_kw(seed):
    return dict(d_match=dev["match"].data_ptr(), nq=len(host["match"]), nt=len(host["fb"]), cam_a=CAM_A, cam_b=CAM_B, d_feat_a=dev["fa"].data_ptr(),
                d_feat_b=dev["fb"].data_ptr(), img_wh=(W, H), seed=seed)


lines = ["inter-camera step, %d correspondences among %d queries, %d map points, p50 / p95 over %d calls (us); leg (b) timed twice, |b1 - b2| = the run's noise"
         % (N, len(host["match"]), len(map_X), PAIRS)]
print(lines[0])
for chain in (True, False):
    def new_job(seed):
        extra = dict(d_first_desc=dev["desc_a"].data_ptr(), d_map_desc=dev["desc_map"].data_ptr()) if chain else dict(d_map_match_a=dev["mm"].data_ptr())
        return dict(pair_kw(seed), Rt_source=Rt_source, **extra)

    def old_problem(f, seed):
        p = dict(x1=f["x1"], x2=f["x2"], K=K, wh=(W, H), seed=seed, Rt_source=Rt_source)
        if chain:
            p.update(d_first_desc=dev["desc_a"].data_ptr(), first_feature=f["pair_q"], d_map_desc=dev["desc_map"].data_ptr())
        else:
            p["map_index"] = dev["mm"].cpu().numpy()[f["pair_q"]]            # the map match comes back: a copy + synchronisation
        return p

    def new_one(f):
        return ctxs[0].inter_pose_dev(**new_job(f + 1))

    def new_batch(f):
        return abi.inter_pose_batch_dev(ctxs, [new_job(f + 1 + j) for j in range(NB)])

    def old_one(f):
        return abi.inter_pose_batch([ctxs[0]], [old_problem(ctxs[0].pair_filter_dev("E", **pair_kw(f + 1)), f + 1)], map_X)[0]

    def old_batch(f):
        fs = abi.pair_filter_batch_dev(ctxs, "E", [pair_kw(f + 1 + j) for j in range(NB)])
        return abi.inter_pose_batch(ctxs, [old_problem(fs[j], f + 1 + j) for j in range(NB)], map_X)

    name = "chain   " if chain else "shortcut"
    for what, old, new in (("1 pair    ", old_one, new_one), ("batch of %d" % NB, old_batch, new_batch)):
        if only_new:
            a, a95, r = p50(new)
            lines.append("%s %s (a) device p50 %8.1f  p95 %8.1f" % (name, what, a, a95))
            print(lines[-1])
            continue
        b1, b1_95, rb = p50(old)
        a, a95, ra = p50(new)
        b2, b2_95, _ = p50(old)
        ra0, rb0 = (ra[0], rb[0]) if isinstance(ra, list) else (ra, rb)
        same = ra0["stage"] == rb0["stage"] == 0 and np.array_equal(ra0["Rt"], rb0["Rt"]) and np.array_equal(ra0["cov"], rb0["cov"])
        noise = abs(b1 - b2)
        lines.append("%s %s (a) device p50 %8.1f (p95 %8.1f)  (b) filter + host step p50 %8.1f / %8.1f (p95 %8.1f / %8.1f)  noise %6.1f  a - min(b) %+8.1f  %s   "
                     "n_front %d n_common %d%s" % (name, what, a, a95, b1, b2, b1_95, b2_95, noise, a - min(b1, b2),
                                                   "not slower" if a <= min(b1, b2) + noise else "SLOWER", ra0["n_front"], ra0["n_common"],
                                                   "" if same else "  (!! results differ)"))
        print(lines[-1])
if not only_new:
    os.makedirs(os.path.join(R, "profiles"), exist_ok=True)
    with open(os.path.join(R, "profiles", "inter_pose_dev.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
for c in ctxs:
    c.close()

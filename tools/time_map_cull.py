#!/usr/bin/env python3
"""What the map's observation statistics and the cull cost (clc_map_observe_dev, clc_map_cull_dev), in one process and run:

  observe  one frame of 10 000 keypoints folded into the statistics of a map of 2 000 and of 10 000 rows: the enqueue (no host wait) and
           the two launches, between device events on the context's stream
  binned   clc_match_map_binned_dev of the same frame against the same map: the match the observe call rides behind
  cull     clc_map_cull_dev on a map of 10 000 rows dropping about 30 % of them (d_flagged), one list of 10 000 entries remapped, entry to
           return; the map is installed anew (untimed) before every call
  rebuild  clc_map_update_batch_dev at 3 cameras x 2 000 rows (the first shape of profiles/map_update.txt, tools/time_map_update.py's
           scene), host wall time, the old map installed anew (untimed) before every call: what a cull replaces when the map is full

The legs of a pair rotate call by call after a settle.  Before a time is taken the first observe call's counters and the first cull's remap
are checked against the host statement (tests/map_cull_host.py) at 2 000 rows.  No figure is a condition: this file reports.
usage: tools/time_map_cull.py [out.txt]   (default profiles/map_cull.txt; the text also goes to stdout)"""
import itertools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import map_cull_host as ch  # noqa: E402
from coloc_amd import Context, abi  # noqa: E402

NQ = 10000
MAPS = (2000, 10000)
CALLS, SETTLE = 30, 10
W, H = 1280, 720
CAM = (1000.0, 640.0, 360.0, 0.0, 0.0, 0.0)


def scene(nm, seed):
    """nm landmarks in front of the identity pose, four fifths of them inside the image; NQ keypoints, half of them on a landmark's
    projection with half a pixel of noise and tracking it"""
    rng = np.random.RandomState(seed)
    px = np.column_stack([rng.uniform(-0.1 * W, 1.1 * W, nm), rng.uniform(-0.1 * H, 1.1 * H, nm)])
    z = rng.uniform(4.0, 30.0, nm)
    X = np.column_stack([(px[:, 0] - CAM[1]) * z / CAM[0], (px[:, 1] - CAM[2]) * z / CAM[0], z])
    M = rng.randint(0, 256, (nm, 64)).astype(np.uint8)
    feat = np.column_stack([rng.uniform(0, W, NQ), rng.uniform(0, H, NQ)])
    track = np.full(NQ, -1, dtype=np.int32)
    rows = rng.choice(nm, min(NQ // 2, nm), replace=False)
    track[:len(rows)] = rows
    feat[:len(rows)] = px[rows] + rng.normal(0.0, 0.5, (len(rows), 2))
    Q = rng.randint(0, 256, (NQ, 64)).astype(np.uint8)
    Q[:len(rows)] = M[rows]
    return M, X, Q, feat.astype(np.float32), track


def timed(legs, s):
    for _ in range(SETTLE):
        for fn in legs.values():
            fn()
    names = list(legs)
    ev, wall = {k: [] for k in legs}, {k: [] for k in legs}
    for r in range(CALLS):
        for k in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(s)
            legs[k]()
            e1.record(s)
            wall[k].append((time.perf_counter() - t0) * 1e6)                       # the call's own host time: what the frame loop pays
            e1.synchronize()
            ev[k].append(e0.elapsed_time(e1) * 1e3)
    return ev, wall


def observe_legs(lines, nm):
    M, X, Q, feat, track = scene(nm, 11 + nm)
    ctx = Context(device=0, width=W, height=H, maxkp=max(nm, NQ), detector=False)
    ctx.set_map(M)
    ctx.set_map_points(X)
    d_q, d_feat, d_track = torch.from_numpy(Q).cuda(), torch.from_numpy(feat).cuda(), torch.from_numpy(track).cuda()
    d_match = torch.full((NQ,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.ExternalStream(ctx.stream)
    view = dict(n=NQ, cam=CAM, Rt=np.eye(3, 4), width=W, height=H, gate=3.0, margin=8.0, d_feat=d_feat.data_ptr(), feat_stride=2, d_track=d_track.data_ptr())

    def observe():
        ctx.map_observe_dev(**view)

    def binned():
        ctx.match_map_binned_dev(stream=ctx.stream, d_q=d_q.data_ptr(), nq=NQ, cam=CAM, Rt=np.eye(3, 4), radius=8.0, threshold=60, d_match=d_match.data_ptr(),
                                 d_feat=d_feat.data_ptr(), feat_stride=2)

    observe()
    got = ctx.map_stats()
    checked = "not held to the statement at this size"
    if nm <= 2000:
        st = ch.Stats()
        ch.observe(st, X, [dict(cam=CAM, Rt=np.eye(3, 4), feat=feat, track=track, count=None, width=W, height=H, gate=3.0, margin=8.0)])
        v, f, l = st.arrays()
        assert np.array_equal(got["visible"], v) and np.array_equal(got["found"], f) and np.array_equal(got["last_view"], l), "the entry differs from the statement"
        checked = "counters equal the host statement"
    ev, wall = timed({"observe": observe, "binned": binned}, s)
    lines.append("%d keypoints against a map of %d rows, gate 3 px, margin 8 px: %d rows in view, %d found (%s)"
                 % (NQ, nm, int(got["visible"].sum()), int(got["found"].sum()), checked))
    for k, what in (("observe", "clc_map_observe_dev: enqueue only, two launches"), ("binned", "clc_match_map_binned_dev, radius 8 px: enqueue only")):
        lines.append("  %-7s us per call, device events: median %8.2f  min %8.2f  max %8.2f; host wall of the call median %8.2f   (%s)"
                     % (k, float(np.median(ev[k])), min(ev[k]), max(ev[k]), float(np.median(wall[k])), what))
    ctx.close()


def cull_and_rebuild_legs(lines):
    nm = 10000
    M, X, _, _, track = scene(nm, 5)
    rng = np.random.RandomState(6)
    flagged = (rng.uniform(size=nm) < 0.3).astype(np.uint8)
    ctx = Context(device=0, width=W, height=H, maxkp=nm, detector=False)
    d_flag = torch.from_numpy(flagged).cuda()
    d_list = torch.from_numpy(track).cuda()
    torch.cuda.synchronize()

    def restore():
        ctx.set_map(M)
        ctx.set_map_points(X)
        d_list.copy_(torch.from_numpy(track))
        torch.cuda.synchronize()

    def cull():
        return ctx.map_cull_dev(d_flagged=d_flag.data_ptr(), lists=[(d_list.data_ptr(), NQ)], **ch.DEFAULT_RULE)

    restore()
    first = cull()
    want, kept = ch.remap(flagged != 0)
    assert np.array_equal(first["remap"], want) and first["n_kept"] == kept, "the entry differs from the statement"
    assert np.array_equal(d_list.cpu().numpy(), ch.remap_list(track, nm, want)), "the remapped list differs from the statement"

    # the rebuild: tools/time_map_update.py's scene at 3 cameras x 2 000 rows
    cams_n, rows = 3, 2000
    K = np.array([[CAM[0], 0, CAM[1]], [0, CAM[0], CAM[2]], [0, 0, 1.0]])
    g = np.random.default_rng(7)
    P = np.stack([g.uniform(-5, 5, rows), g.uniform(-3, 3, rows), g.uniform(8, 20, rows)], 1)
    point_of, feats, descs = [], [], []
    base = g.integers(0, 256, (rows, 64), dtype=np.uint8)
    for c in range(cams_n):
        ang = g.uniform(-0.06, 0.06) if c else 0.0
        Rc = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        perm = g.permutation(rows)
        u = ((P[perm] - np.array([0.8 * c, 0.0, 0.0])) @ Rc.T) @ K.T
        f = np.zeros((rows, 4), dtype=np.float32)
        f[:, :2] = u[:, :2] / u[:, 2:3] + g.normal(0, 0.3, (rows, 2))
        d = base[perm].copy()
        d[np.arange(rows), g.integers(0, 64, rows)] ^= 1
        point_of.append(perm); feats.append(f); descs.append(d)
    row_of = [np.argsort(p) for p in point_of]
    pair_cams = list(itertools.combinations(range(cams_n), 2))
    matches = []
    for ca, cb in pair_cams:
        m = np.full(rows, -1, dtype=np.int32)
        q = g.choice(rows, int(0.7 * rows), replace=False)
        m[q] = row_of[cb][point_of[ca][q]]
        matches.append(m)
    old_rows = np.sort(g.choice(rows, rows // 3, replace=False))
    old_desc = descs[0][old_rows].copy()
    old_desc[np.arange(len(old_rows)), g.integers(0, 64, len(old_rows))] ^= 2
    old_X = P[point_of[0][old_rows]] * 2.5
    d_match = [torch.from_numpy(m).cuda() for m in matches]
    d_feat = [torch.from_numpy(f).cuda() for f in feats]
    d_desc = [torch.from_numpy(d).cuda() for d in descs]
    torch.cuda.synchronize()
    ctxs = [Context(device=0, width=W, height=H, maxkp=rows, detector=False) for _ in pair_cams]
    jobs = lambda sd: [dict(d_match=d_match[k].data_ptr(), nq=rows, nt=rows, cam_a=CAM, cam_b=CAM, d_feat_a=d_feat[ca].data_ptr(), feat_stride_a=4,
                            d_feat_b=d_feat[cb].data_ptr(), feat_stride_b=4, img_wh=(W, H), seed=sd + k) for k, (ca, cb) in enumerate(pair_cams)]
    dc = [dict(cam=CAM, d_feat=d_feat[i].data_ptr(), feat_stride=4, d_desc=d_desc[i].data_ptr()) for i in range(cams_n)]

    def rebuild(f):
        ctxs[0].set_map(old_desc)
        ctxs[0].set_map_points(old_X)
        t0 = time.perf_counter()
        r = abi.map_update_batch_dev(ctxs, jobs(1 + f), [rows] * cams_n, pair_cams, dc, scale=3.0)[0]
        return (time.perf_counter() - t0) * 1e6, r

    t_cull, t_rebuild, res = [], [], None
    for f in range(CALLS + 3):
        for leg in (("cull", "rebuild") if f % 2 == 0 else ("rebuild", "cull")):
            if leg == "cull":
                restore()
                t0 = time.perf_counter()
                cull()
                t_cull.append((time.perf_counter() - t0) * 1e6)
            else:
                t, res = rebuild(f)
                t_rebuild.append(t)
    lines.append("a map of %d rows, %d dropped (d_flagged), one list of %d entries remapped; beside it the rebuild at %d cameras x %d rows (%d old rows, %d new rows)"
                 % (nm, first["n_dropped"], NQ, cams_n, rows, len(old_rows), res["map_n"]))
    for name, t, what in (("cull", t_cull, "clc_map_cull_dev, entry to return, remap checked against the statement"),
                          ("rebuild", t_rebuild, "clc_map_update_batch_dev, entry to return")):
        t = np.sort(t[3:])
        lines.append("  %-7s us per call, host wall: median %9.1f  min %9.1f  max %9.1f over %d calls after 3 warm ones   (%s)"
                     % (name, float(np.median(t)), t[0], t[-1], len(t), what))
    ctx.close()
    for c in ctxs:
        c.close()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "map_cull.txt")
    lines = ["the map's observation statistics beside the binned match they ride behind, and the cull beside the rebuild it replaces, %s" % torch.cuda.get_device_name(0),
             "device events on the context's stream around every enqueue-only call and host wall time, %d calls per leg, the legs rotating, after %d calls of each; "
             "one run; report only" % (CALLS, SETTLE)]
    for nm in MAPS:
        observe_legs(lines, nm)
    cull_and_rebuild_legs(lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

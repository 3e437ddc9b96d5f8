#!/usr/bin/env python3
"""What extending the map in place (clc_map_extend_dev) costs, in one process and run:

  whole    the call from entry to return -- F on the host, the guided prep and sweep, the mask, the one-to-one filter's three launches,
           the point launch, the append workgroup, the host's wait for its pinned word -- on two views of 2 000 and of 10 000 rows
           (tests/map_extend_host.py's scene: three quarters of the rows common, a quarter of those tracked) against maps of 2 000 and
           10 000 rows
  guided   clc_match_guided_dev alone on the same two views under the same F, and a stream synchronisation: the sweep the step stands
           behind.  whole - guided is what the new launches and the wait cost.
  rebuild  for scale, one line: clc_map_init_grow_batch_dev at 3 cameras x 2 000 rows (tools/time_map_grow.py's scene), host wall time --
           what producing landmarks costs today.

update_tracks is off and MatcherOptions.maxkp leaves room for every call of the run, so every call does the same work (the same rows are
appended again behind the last ones; nothing is restored between calls).  Device events on the context's stream around each call, and
host wall time beside them; the legs alternate call by call after a settle.  Before a time is taken the first call's lists are checked
against the host statement (2 000 rows) or its counts are printed (10 000 rows: the statement is a Python loop).  No figure is a
condition: this file reports.
usage: tools/time_map_extend.py [out.txt]   (default profiles/map_extend.txt; the text also goes to stdout)"""
import itertools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import map_extend_host as mh  # noqa: E402
from coloc_amd import Context, abi  # noqa: E402

ROWS = (2000, 10000)
MAPS = (2000, 10000)
CALLS, SETTLE = 30, 10


def view_kw(v, keep):
    d, f, t = torch.from_numpy(v["desc"]).cuda(), torch.from_numpy(v["feat"]).cuda(), torch.from_numpy(v["track"]).cuda()
    keep += [d, f, t]
    return dict(d_desc=d.data_ptr(), n=len(v["desc"]), cam=v["cam"], Rt=v["Rt"], d_feat=f.data_ptr(), feat_stride=2, d_track=t.data_ptr())


def extend_legs(lines, rows, map_n):
    views, _ = mh.make_views([rows, rows], seed=rows + map_n, map_n=map_n)
    M, X = mh.make_map(map_n, 3)
    ctx = Context(device=0, maxkp=map_n + (CALLS + SETTLE + 2) * rows, detector=False)
    ctx.set_map(M)
    ctx.set_map_points(X)
    keep = []
    a, b = view_kw(views[0], keep), view_kw(views[1], keep)
    d_match = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.ExternalStream(ctx.stream)
    F = abi.fundamental_from_poses(views[0]["cam"], views[0]["Rt"], views[1]["cam"], views[1]["Rt"])
    par = dict(band=mh.BAND, threshold=mh.THRESHOLD, max_distance=mh.CAP)

    def whole():
        return ctx.extend_map(a, b, update_tracks=False, **par)

    def guided():
        ctx.match_guided_dev(stream=ctx.stream, d_q=a["d_desc"], nq=rows, d_t=b["d_desc"], nt=rows, cam_a=views[0]["cam"], cam_b=views[1]["cam"], F=F,
                             band=mh.BAND, threshold=mh.THRESHOLD, d_match=d_match.data_ptr(), d_feat_a=a["d_feat"], feat_stride_a=2,
                             d_feat_b=b["d_feat"], feat_stride_b=2)
        ctx.sync()

    first = whole()
    if rows <= 2000:
        st = mh.statement(views[0], views[1], mh.BAND, mh.THRESHOLD, mh.CAP, map_n, map_n + rows, update_tracks=False)
        assert np.array_equal(first["new_q"], st["new_q"]) and np.array_equal(first["new_t"], st["new_t"]), "the entry differs from the statement"
        assert np.array_equal(first["X"].view(np.uint64), st["X"].view(np.uint64)), "the entry's points differ from the statement"
        checked = "lists and points equal the host statement"
    else:
        checked = "not held to the statement at this size"
    legs = {"whole": whole, "guided": guided}
    for _ in range(SETTLE):
        for fn in legs.values():
            fn()
    ev, wall = {k: [] for k in legs}, {k: [] for k in legs}
    for r in range(CALLS):
        for k in (("whole", "guided") if r % 2 == 0 else ("guided", "whole")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(s)
            legs[k]()
            e1.record(s)
            e1.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e6)
            ev[k].append(e0.elapsed_time(e1) * 1e3)
    lines.append("2 x %d rows against a map of %d rows, band %.1f px, threshold %d, cap %d: %d guided matches, %d landmarks added per call (%s)"
                 % (rows, map_n, mh.BAND, mh.THRESHOLD, mh.CAP, first["n_guided"], first["n_added"], checked))
    med = {}
    for k, what in (("whole", "clc_map_extend_dev, entry to return"), ("guided", "clc_match_guided_dev + a stream synchronisation")):
        med[k] = float(np.median(ev[k]))
        lines.append("  %-7s us per call, device events: median %8.2f  min %8.2f  max %8.2f; host wall median %8.2f   (%s)"
                     % (k, med[k], min(ev[k]), max(ev[k]), float(np.median(wall[k])), what))
    lines.append("  whole - guided (medians of the events): %.2f us" % (med["whole"] - med["guided"]))
    ctx.close()


def rebuild_leg(lines):
    """tools/time_map_grow.py's scene at 3 cameras x 2 000 rows"""
    cams_n, rows, calls = 3, 2000, 10
    W, H, F0 = 1280, 720, (1000.0, 640.0, 360.0)
    K = np.array([[F0[0], 0, F0[1]], [0, F0[0], F0[2]], [0, 0, 1.0]])
    rng = np.random.default_rng(7)
    X = np.stack([rng.uniform(-5, 5, rows), rng.uniform(-3, 3, rows), rng.uniform(8, 20, rows)], 1)
    cams, point_of, feats, descs = [], [], [], []
    base = rng.integers(0, 256, (rows, 64), dtype=np.uint8)
    for c in range(cams_n):
        ang = rng.uniform(-0.06, 0.06) if c else 0.0
        Rc = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        perm = rng.permutation(rows)
        u = ((X[perm] - np.array([0.8 * c, 0.0, 0.0])) @ Rc.T) @ K.T
        f = np.zeros((rows, 4), dtype=np.float32)
        f[:, :2] = u[:, :2] / u[:, 2:3] + rng.normal(0, 0.3, (rows, 2))
        d = base[perm].copy()
        d[np.arange(rows), rng.integers(0, 64, rows)] ^= 1
        cams.append(F0 + (0.0, 0.0, 0.0)); point_of.append(perm); feats.append(f); descs.append(d)
    row_of = [np.argsort(p) for p in point_of]
    pair_cams = list(itertools.combinations(range(cams_n), 2))
    matches = []
    for ca, cb in pair_cams:
        m = np.full(rows, -1, dtype=np.int32)
        q = rng.choice(rows, int(0.7 * rows), replace=False)
        m[q] = row_of[cb][point_of[ca][q]]
        matches.append(m)
    d_match = [torch.from_numpy(m).cuda() for m in matches]
    d_feat = [torch.from_numpy(f).cuda() for f in feats]
    d_desc = [torch.from_numpy(d).cuda() for d in descs]
    torch.cuda.synchronize()
    ctxs = [Context(device=0, width=W, height=H, maxkp=rows * cams_n // 2, detector=False) for _ in pair_cams]
    jobs = lambda sd: [dict(d_match=d_match[k].data_ptr(), nq=rows, nt=rows, cam_a=cams[ca], cam_b=cams[cb], d_feat_a=d_feat[ca].data_ptr(),
                            feat_stride_a=4, d_feat_b=d_feat[cb].data_ptr(), feat_stride_b=4, img_wh=(W, H), seed=sd + k)
                       for k, (ca, cb) in enumerate(pair_cams)]
    dc = [dict(cam=cams[i], d_feat=d_feat[i].data_ptr(), feat_stride=4, d_desc=d_desc[i].data_ptr()) for i in range(cams_n)]
    t, res = [], None
    for f in range(calls + 3):
        t0 = time.perf_counter()
        res = abi.map_init_grow_batch_dev(ctxs, jobs(1 + f), [rows] * cams_n, pair_cams, dc, seed=1 + f)[0]
        t.append((time.perf_counter() - t0) * 1e6)
    lines.append("for scale: clc_map_init_grow_batch_dev, %d cameras x %d rows, a map of %d rows rebuilt from the pair filters up: host wall median "
                 "%.1f us over %d calls after 3 warm ones" % (cams_n, rows, res["map_n"], float(np.median(t[3:])), calls))
    for c in ctxs:
        c.close()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "map_extend.txt")
    lines = ["the map extended in place beside the guided sweep it stands behind, %s" % torch.cuda.get_device_name(0),
             "device events on the context's stream around every call and host wall time beside them, %d calls per leg, the legs alternating, "
             "after %d calls of each; one run" % (CALLS, SETTLE)]
    for rows in ROWS:
        for map_n in MAPS:
            extend_legs(lines, rows, map_n)
    rebuild_leg(lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

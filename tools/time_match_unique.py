#!/usr/bin/env python3
"""What the one-to-one filter (clc_match_unique_dev: the claim words armed, a claim launch, a resolve launch) costs beside its producers,
in one process and run, with planted doubles so that the filter has work:

  pair   10k x 10k: clc_match_2nn_dev; clc_match_2nn_unique_dev (the sweep and the filter); the filter alone on a fixed (d_match, d_best);
         and a second clc_match_2nn_dev with the roles swapped -- what the mutual-nearest rule would have cost on top of the first sweep
  map    10k queries against 2 000 and 10 000 map rows, binned at 8 px: clc_match_map_binned_dev; clc_match_map_binned_unique_dev; the
         filter alone
  worst  10k queries that all claim ONE row: the filter alone

The filter works in place, so "the filter alone" restores d_match from a copy before every call; that copy is timed as a leg of its own
and is to be subtracted.  Device events on one stream around batches of warm calls, the legs rotating batch by batch after a settle;
the spread of the batches is reported with the medians.  Before a time is taken every composed result is checked against the producer's
lists through the host statement (tests/unique_host.py).  No figure is a condition: this file reports.
usage: tools/time_match_unique.py [out.txt]   (default profiles/match_unique.txt; the text also goes to stdout)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bin_host as bh  # noqa: E402
import guided_host as gh  # noqa: E402
import proj_host as ph  # noqa: E402
import unique_host as uh  # noqa: E402
from coloc_amd import Context  # noqa: E402

NQ = 10000
MAPS = (2000, 10000)
RADIUS = 8.0
THR = 40
BATCH, ROUNDS, SETTLE = 20, 20, 100


def near_copies(rng, rows, max_flip):
    """every row with at most max_flip bits flipped (positions drawn with replacement: a bit drawn twice flips back)"""
    out = rows.copy()
    n = len(rows)
    for _ in range(max_flip):
        on = rng.random(n) < 0.5
        bit = rng.integers(0, 512, n)
        out[np.arange(n), bit >> 3] ^= np.where(on, 1 << (bit & 7), 0).astype(np.uint8)
    return out


def timed(s, calls, legs):
    """{leg: [us per call of each batch]}: SETTLE calls of each, then ROUNDS rounds of one batch per leg, the order rotating"""
    for _ in range(SETTLE):
        for k in legs:
            calls[k]()
    s.synchronize()
    per = {k: [] for k in legs}
    for r in range(ROUNDS):
        for i in range(len(legs)):
            k = legs[(r + i) % len(legs)]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(BATCH):
                calls[k]()
            b.record(s)
            b.synchronize()
            per[k].append(a.elapsed_time(b) * 1e3 / BATCH)
    return per


def report(lines, per, legs, what):
    med = {k: float(np.median(per[k])) for k in legs}
    for k in legs:
        lines.append("  %-9s us per call: median %7.2f  min %7.2f  max %7.2f   (%s)" % (k, med[k], min(per[k]), max(per[k]), what[k]))
    return med


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "match_unique.txt")
    dev = torch.device("cuda", 0)
    ctx = Context(device=0, maxkp=NQ, detector=False)
    qpb = ctx.k2nn_plan_query(NQ, NQ)["queries_per_block"]
    formulation = {128: "popcount", 256: "matrix"}.get(qpb, "%d queries per block" % qpb)
    rng = np.random.default_rng(5)
    s = torch.cuda.Stream(device=dev)
    sp = s.cuda_stream
    lines = ["the one-to-one filter beside its producers (%s formulation of the pair sweep), %s" % (formulation, torch.cuda.get_device_name(0)),
             "device events on one stream, %d batches of %d warm calls each per leg, the legs rotating, after %d calls of each; one run"
             % (ROUNDS, BATCH, SETTLE)]

    def i32(n, v=-7):
        return torch.full((max(n, 1),), v, dtype=torch.int32, device=dev)

    def restore(dst, src):
        with torch.cuda.stream(s):
            dst.copy_(src, non_blocking=True)

    # -- the pair: T random, Q near-copies of rows 0 .. 8 499 and SECOND near-copies of rows 0 .. 1 499
    dup = 1500
    T = rng.integers(0, 256, (NQ, 64), dtype=np.uint8)
    Q = np.concatenate([near_copies(rng, T[:NQ - dup], 30), near_copies(rng, T[:dup], 40)])
    d_q, d_t = torch.from_numpy(Q).to(dev), torch.from_numpy(T).to(dev)
    d_plain, d_uni, d_swap, d_work, d_owner = i32(NQ), i32(NQ), i32(NQ), i32(NQ), i32(NQ)
    torch.cuda.synchronize()
    plain, best, _ = ctx.match_2nn(Q, T, THR, want_dist=True)
    want = uh.unique(plain, best, NQ)
    ctx.match_2nn_dev(d_q.data_ptr(), NQ, d_t.data_ptr(), NQ, THR, d_plain.data_ptr())
    ctx.match_2nn_unique_dev(d_q.data_ptr(), NQ, d_t.data_ptr(), NQ, THR, d_uni.data_ptr(), d_owner.data_ptr())
    ctx.sync()
    assert np.array_equal(d_plain.cpu().numpy(), plain), "clc_match_2nn_dev differs from clc_match_2nn"
    assert np.array_equal(d_uni.cpu().numpy(), want[0]) and np.array_equal(d_owner.cpu().numpy(), want[1]), "the composed pair entry differs from the statement"
    d_best = torch.from_numpy(best.view(np.int16)).to(dev)
    torch.cuda.synchronize()

    def filter_alone(src, bst, nt):
        restore(d_work, src)
        ctx.match_unique_dev(d_work.data_ptr(), bst.data_ptr(), NQ, nt, d_owner.data_ptr(), sp)

    legs = ("sweep", "composed", "filter", "copy", "swapped")
    what = {"sweep": "clc_match_2nn_dev", "composed": "clc_match_2nn_unique_dev: the sweep, then arm + claim + resolve",
            "filter": "a 40 KB device copy, then clc_match_unique_dev with d_owner", "copy": "that copy alone",
            "swapped": "clc_match_2nn_dev with the roles swapped: the mutual rule's second sweep"}
    calls = {"sweep": lambda: ctx.match_2nn_dev(d_q.data_ptr(), NQ, d_t.data_ptr(), NQ, THR, d_plain.data_ptr(), sp),
             "composed": lambda: ctx.match_2nn_unique_dev(d_q.data_ptr(), NQ, d_t.data_ptr(), NQ, THR, d_uni.data_ptr(), d_owner.data_ptr(), sp),
             "filter": lambda: filter_alone(d_plain, d_best, NQ), "copy": lambda: restore(d_work, d_plain),
             "swapped": lambda: ctx.match_2nn_dev(d_t.data_ptr(), NQ, d_q.data_ptr(), NQ, THR, d_swap.data_ptr(), sp)}
    per = timed(s, calls, legs)
    lines.append("pair %d x %d, threshold %d: %d accepted, %d train rows named more than once, %d kept by the filter"
                 % (NQ, NQ, THR, (plain >= 0).sum(), len(uh.doubled_rows(plain)), (want[0] >= 0).sum()))
    med = report(lines, per, legs, what)
    lines.append("  composed - sweep (medians): %.2f us; filter - copy: %.2f us; the swapped sweep: %.2f us -- the filter costs %s the mutual rule's second sweep"
                 % (med["composed"] - med["sweep"], med["filter"] - med["copy"], med["swapped"],
                    "LESS than" if med["composed"] - med["sweep"] < med["swapped"] else "MORE than"))

    # -- the map: the first 40 % of the queries sit on landmarks, the rows of the first 30 % taken again by the next 10 % (2 000 rows: by wrap)
    for nm in MAPS:
        M = rng.integers(0, 256, (nm, 64), dtype=np.uint8)
        mpix = np.column_stack([rng.uniform(0, gh.W, nm), rng.uniform(0, gh.H, nm)])
        X = np.array([ph.landmark(x, y, z) for (x, y), z in zip(mpix, rng.uniform(2.0, 10.0, nm))])
        Qm = rng.integers(0, 256, (NQ, 64), dtype=np.uint8)
        qpos = np.column_stack([rng.uniform(0, gh.W, NQ), rng.uniform(0, gh.H, NQ)]).astype(np.float32)
        on = np.arange(4 * NQ // 10)
        row = np.where(on < 3 * NQ // 10, on, on - 3 * NQ // 10) % nm
        Qm[on] = near_copies(rng, M[row], 30)
        qpos[on] = (mpix[row] + rng.uniform(-1.0, 1.0, (len(on), 2))).astype(np.float32)
        ctx.set_map(M)
        ctx.set_map_points(X)
        assert ctx.map_binned_plan(gh.CAM_EXACT, RADIUS)["plan"] == bh.BINNED
        d_mq, d_f = torch.from_numpy(Qm).to(dev), torch.from_numpy(qpos).to(dev)
        d_bm, d_um, d_mown = i32(NQ), i32(NQ), i32(nm)
        d_bb = torch.zeros((NQ,), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        job = dict(d_q=d_mq.data_ptr(), nq=NQ, cam=gh.CAM_EXACT, Rt=ph.IDENTITY, radius=RADIUS, threshold=THR, d_feat=d_f.data_ptr(), feat_stride=2)
        ctx.match_map_binned_dev(d_match=d_bm.data_ptr(), d_best=d_bb.data_ptr(), **job)
        ctx.match_map_binned_unique_dev(d_owner=d_mown.data_ptr(), d_match=d_um.data_ptr(), **job)
        ctx.sync()
        pm, pb = d_bm.cpu().numpy(), d_bb.cpu().numpy().view(np.uint16)
        wm = uh.unique(pm, pb, nm)
        assert np.array_equal(d_um.cpu().numpy(), wm[0]) and np.array_equal(d_mown.cpu().numpy(), wm[1]), "the composed binned entry differs from the statement at %d rows" % nm

        def map_filter():
            restore(d_work, d_bm)
            ctx.match_unique_dev(d_work.data_ptr(), d_bb.data_ptr(), NQ, nm, d_mown.data_ptr(), sp)

        legs = ("binned", "composed", "filter", "copy")
        what = {"binned": "clc_match_map_binned_dev with d_best", "composed": "clc_match_map_binned_unique_dev, d_best in the context's scratch",
                "filter": "a 40 KB device copy, then clc_match_unique_dev with d_owner", "copy": "that copy alone"}
        calls = {"binned": lambda: ctx.match_map_binned_dev(sp, d_match=d_bm.data_ptr(), d_best=d_bb.data_ptr(), **job),
                 "composed": lambda: ctx.match_map_binned_unique_dev(d_mown.data_ptr(), sp, d_match=d_um.data_ptr(), **job),
                 "filter": map_filter, "copy": lambda: restore(d_work, d_bm)}
        per = timed(s, calls, legs)
        lines.append("map %d x %d rows, radius %.1f px, threshold %d: %d accepted, %d landmarks taken more than once, %d kept by the filter"
                     % (NQ, nm, RADIUS, THR, (pm >= 0).sum(), len(uh.doubled_rows(pm)), (wm[0] >= 0).sum()))
        med = report(lines, per, legs, what)
        lines.append("  composed - binned (medians): %.2f us; filter - copy: %.2f us" % (med["composed"] - med["binned"], med["filter"] - med["copy"]))

    # -- the worst case: every query claims row 0
    d_zero = i32(NQ, 0)
    wb = rng.integers(0, 513, NQ).astype(np.uint16)
    d_wb = torch.from_numpy(wb.view(np.int16)).to(dev)
    d_wown = i32(8)
    torch.cuda.synchronize()

    def worst():
        restore(d_work, d_zero)
        ctx.match_unique_dev(d_work.data_ptr(), d_wb.data_ptr(), NQ, 8, d_wown.data_ptr(), sp)

    worst()
    s.synchronize()
    ww = uh.unique(np.zeros(NQ, np.int32), wb, 8)
    assert np.array_equal(d_work.cpu().numpy(), ww[0]) and np.array_equal(d_wown.cpu().numpy()[:8], ww[1]), "the worst case differs from the statement"
    legs = ("filter", "copy")
    per = timed(s, {"filter": worst, "copy": lambda: restore(d_work, d_zero)}, legs)
    lines.append("worst case: %d queries that all claim row 0 (one claim word takes every atomic)" % NQ)
    med = report(lines, per, legs, {"filter": "a 40 KB device copy, then clc_match_unique_dev", "copy": "that copy alone"})
    lines.append("  filter - copy (medians): %.2f us" % (med["filter"] - med["copy"]))
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A tracked frame's pose from the prediction (clc_track_prior_dev: track launch + ONE solve launch, one host wait) beside
clc_track_localize_dev with refine = 1 (track launch, the host's wait for the count, the a-contrario rounds with the host in the loop, the
refinement) on the SAME d_match, in one process and run, the two legs alternating batch by batch.

Two numbers per leg, because what the new entry removes are host waits: HOST WALL time from call to return (time.perf_counter around the
C call alone: the job structs are filled once, outside the clock) and DEVICE EVENTS on the context's stream around batches of calls.
Two frames: 1 000 tracks among 1 603 queries with 30 % wrong matches (the scene of tests/test_gpu_track_localize.py), and the guided
tracks of the rendered chain of tests/test_gpu_track_prior.py.  The prior is the pose clc_track_localize_dev returns for the frame and the
gate its error_max -- a tracker's steady state.  Before a time is taken the two poses are compared.  Report only: nothing is asserted
about a time.
usage: tools/time_track_prior.py [out.txt]   (default profiles/track_prior.txt; the text also goes to stdout)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
import track_host  # noqa: E402
from coloc_amd import Context, abi  # noqa: E402
from test_gpu_track_localize import _dev, _scattered_scene  # noqa: E402

BATCH, ROUNDS, SETTLE = 20, 40, 200


def measure(ctx, frame, lines, what):
    """frame: the keywords of the two entries that name the frame (d_match, nq, cam, d_kps | d_feat, d_count)"""
    lib = ctx.lib
    first = ctx.track_localize_dev(seed=7, refine=True, **frame)
    assert first["Rt"] is not None
    P, gate = first["Rt"], float(first["error_max"])
    got = ctx.track_prior_dev(Rt_prior=P, gate=gate, **frame)
    assert got["result"] == abi.TRACK_PRIOR_OK and got["n_tracks"] == first["n_tracks"]
    dR = np.degrees(np.arccos(np.clip((np.trace(got["Rt"][:, :3] @ P[:, :3].T) - 1) / 2, -1, 1)))
    dC = np.linalg.norm(got["Rt"][:, :3].T @ got["Rt"][:, 3] - P[:, :3].T @ P[:, 3])
    lines.append("%s: %d tracks; clc_track_localize_dev (refine): %d inliers, error_max %.3f px, %d iterations, rmse %.3f; "
                 "clc_track_prior_dev from its pose at that gate: %d inliers, %d rounds, %d iterations, converged %d, rmse %.3f; "
                 "the two poses differ by %.4f deg, centre %.2e" % (what, first["n_tracks"], len(first["inliers"]), first["error_max"],
                                                                   first["iterations"], first["rmse"], got["n_inliers"], got["rounds_run"],
                                                                   got["iterations"], got["converged"], got["rmse"], dR, dC))
    keep = []
    jl, jp = abi.TrackJob(), abi.TrackPriorJob()
    abi._track_fill(jl, keep, seed=7, refine=True, **frame)
    abi._track_prior_fill(jp, keep, Rt_prior=P, gate=gate, **frame)
    calls = {"localize": lambda: lib.clc_track_localize_dev(ctx.h, C.byref(jl)), "prior": lambda: lib.clc_track_prior_dev(ctx.h, C.byref(jp))}
    s = torch.cuda.ExternalStream(ctx.stream)
    for _ in range(SETTLE):
        for f in calls.values():
            assert f() == 0
    ctx.sync()
    wall = {k: [] for k in calls}
    dev = {k: [] for k in calls}
    order = list(calls)
    for r in range(ROUNDS):
        for i in range(2):
            k = order[(r + i) % 2]
            f = calls[k]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            t0 = time.perf_counter()
            for _ in range(BATCH):
                f()
            t1 = time.perf_counter()
            b.record(s)
            b.synchronize()
            wall[k].append((t1 - t0) * 1e6 / BATCH)
            dev[k].append(a.elapsed_time(b) * 1e3 / BATCH)
    for k, name in (("localize", "clc_track_localize_dev (refine = 1)"), ("prior", "clc_track_prior_dev")):
        lines.append("  %-36s host wall us per call: median %.1f  min %.1f  max %.1f   device events us per call: median %.1f  min %.1f  max %.1f"
                     % (name, np.median(wall[k]), min(wall[k]), max(wall[k]), np.median(dev[k]), min(dev[k]), max(dev[k])))
    lines.append("  prior / localize (medians): host wall %.3f, device events %.3f"
                 % (np.median(wall["prior"]) / np.median(wall["localize"]), np.median(dev["prior"]) / np.median(dev["localize"])))


def rendered_chain():
    """the rendered chain of tests/test_gpu_track_prior.py up to the guided d_match of the third view -> (contexts, frame keywords, keep-alive)"""
    w, h, cap, ppu = 640, 480, 2048, 100.0
    K = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1.0]])
    cams = [(520.0, 320.0, 240.0, 0.0, 0.0, 0.0), (520.0, 320.0, 240.0, -0.05, 0.01, 0.0), (520.0, 320.0, 240.0, 0.0, 0.0, 0.0)]
    tex = synth.plane_texture()
    ctxs = [Context(device=0, width=w, height=h, maxkp=cap, match_thresh=60, fast_thresh=60) for _ in range(3)]
    poses = [synth.look_at_plane_pose((7.0, 7.0), 5.2), synth.look_at_plane_pose((7.25, 6.85), 5.0, yaw=0.05, tilt=(0.03, -0.02)),
             synth.look_at_plane_pose((7.1, 6.95), 5.1, yaw=0.02, tilt=(0.01, -0.01))]
    imgs = [_dev(synth.render_plane(tex, ppu, K, R, t, w, h)) for R, t in poses]
    desc = [torch.zeros((cap, 64), dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_pair, d_plain, d_guided = (torch.full((cap,), -5, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    bufs = []
    for c, img, d in zip(ctxs, imgs, desc):
        c.pyramid_build_dev(img.data_ptr(), w, h, w, None)
        c.detect_dev(None)
        c.describe_detected_dev(d.data_ptr(), None)
        c.sync()
        bufs.append(c.detect_buffers())
    (ka, cnta, _), (kb, cntb, _), (kc, cntc, _) = bufs
    ctx = ctxs[0]
    ctx.match_2nn_dev(desc[0].data_ptr(), cap, desc[1].data_ptr(), cap, 60, d_pair.data_ptr(), None)
    ctx.sync()
    pair = dict(d_match=d_pair.data_ptr(), nq=cap, nt=cap, cam_a=cams[0], cam_b=cams[1], d_kps_a=ka, d_kps_b=kb, d_count_a=cnta, d_count_b=cntb,
                img_wh=(w, h), seed=3)
    dc = [dict(cam=cams[i], d_kps=k, d_desc=desc[i].data_ptr()) for i, k in enumerate((ka, kb))]
    got, _ = abi.map_init_batch_dev([ctx], [pair], [cap, cap], [(0, 1)], dc)
    assert got["entered"] == [True]
    frame = dict(nq=cap, cam=cams[2], d_kps=kc, d_count=cntc)
    ctx.match_map_dev(desc[2].data_ptr(), cap, 60, d_plain.data_ptr(), None)
    first = ctx.track_localize_dev(d_match=d_plain.data_ptr(), seed=7, **frame)
    ctx.match_map_guided_dev(d_q=desc[2].data_ptr(), Rt=first["Rt"], radius=4.0, threshold=60, d_match=d_guided.data_ptr(), **frame)
    ctx.sync()
    return ctxs, dict(d_match=d_guided.data_ptr(), **frame), (imgs, desc, d_pair, d_plain, d_guided)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "track_prior.txt")
    lines = ["a tracked frame's pose from the prediction beside the a-contrario solve on the same d_match, %s" % torch.cuda.get_device_name(0),
             "%d batches of %d warm calls per leg, the legs alternating, after %d calls of each; one run; host wall = perf_counter around the C "
             "calls of a batch, device events on the context's stream around the same batch" % (ROUNDS, BATCH, SETTLE)]
    cam = (1000.0, 640.0, 360.0) + track_host.DISTORTIONS[1]
    match, feat, map_X = _scattered_scene(1000, 5000, cam)
    ctx = Context(device=0, detector=False, matcher=False)
    ctx.set_map_points(map_X)
    d_match, d_feat = _dev(match), _dev(feat)
    measure(ctx, dict(d_match=d_match.data_ptr(), nq=len(match), cam=cam, d_feat=d_feat.data_ptr(), feat_stride=4), lines,
            "1 000 tracks among %d queries, 30 %% wrong matches" % len(match))
    ctx.close()
    ctxs, frame, keep = rendered_chain()
    measure(ctxs[0], frame, lines, "rendered chain, guided match at 4 px (640 x 480)")
    for c in ctxs:
        c.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

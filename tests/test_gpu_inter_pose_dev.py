"""The inter-camera step from device memory (include/coloc_hip.h: clc_inter_pose_dev, clc_inter_pose_batch_dev, clc_inter_front_dev)
against the host path it replaces on the same commit: clc_pair_filter_dev, then clc_inter_pose_batch fed from its host outputs.

Every comparison of values is EXACT (bit patterns): inter_front_kernel / inter_scale_kernel run the fp64 operations of
inter_geometry.cpp in the same order, and the refinement behind them is the same kernel on the same input bits."""
import numpy as np
import pytest

import synth
import track_host
from inter_scenes import K, NO_MODEL, NO_RELATIVE_POSE, NO_SCALE, WH, pair as _pair

pytestmark = pytest.mark.gpu

CAM_A = (1000.0, 640.0, 360.0) + track_host.DISTORTIONS[1]
CAM_B = (1000.0, 640.0, 360.0) + track_host.DISTORTIONS[2]


def _torch():
    import torch
    return torch


def _dev(a):
    torch = _torch()
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _light_ctx():
    from coloc_amd import Context
    return Context(device=0, detector=False, matcher=False)


def _distort(x, cam):
    f, pp, k = cam[0], np.array(cam[1:3]), cam[3:6]
    c = (x - pp) / f
    r2 = (c ** 2).sum(1, keepdims=True)
    return c * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) * f + pp


def _noisy(rows, flips, rng):
    d = rows.copy()
    for _ in range(flips):
        b = rng.integers(0, 512, len(d))
        d[np.arange(len(d)), b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return d


_WORLDS = {}


def _world(seed, n, map_n, in_map=0.6):
    """_pair scattered into what the device entries read, computed once per (seed, n, map_n) and left unchanged: n correspondences among
    1.6 n rows of camera A and 1.3 n rows of camera B (d_match, float feature blocks holding the distorted pixels), a global map of
    EXACTLY map_n points (the recipe's, cut or filled up with points no feature sees), camera A's match against it, and a descriptor per
    row of both cameras and of the map (a world point's descriptor seen with a few bits flipped)."""
    key = (seed, n, map_n, in_map)
    if key in _WORLDS:
        return _WORLDS[key]
    p = _pair(seed, n, in_map=in_map)
    rng = np.random.default_rng(seed + 7)
    nq, nt = int(1.6 * n) + 3, int(1.3 * n) + 5
    qs = np.sort(rng.choice(nq, n, replace=False))
    rows = rng.choice(nt, n, replace=False)
    match = np.full(nq, -1, dtype=np.int32)
    match[qs] = rows
    featA = np.zeros((nq, 4), dtype=np.float32)
    featA[:, :2] = np.stack([rng.uniform(0, WH[0], nq), rng.uniform(0, WH[1], nq)], 1)
    featA[qs, :2] = _distort(p["x1"], CAM_A)
    featB = np.stack([rng.uniform(0, WH[0], nt), rng.uniform(0, WH[1], nt)], 1).astype(np.float32)
    featB[rows] = _distort(p["x2"], CAM_B)
    m0 = len(p["map_X"])
    map_X = np.stack([rng.uniform(-5, 5, map_n), rng.uniform(-5, 5, map_n), rng.uniform(30, 40, map_n)], 1)
    map_X[:min(m0, map_n)] = p["map_X"][:map_n]
    map_index = np.where(p["map_index"] < map_n, p["map_index"], -1).astype(np.int32)
    map_match_a = np.full(nq, -1, dtype=np.int32)
    map_match_a[qs] = map_index
    point = synth.random_descriptors(n, seed=seed + 1)
    descA, descB, desc_map = (synth.random_descriptors(k, seed=seed + 2 + i) for i, k in enumerate((nq, nt, map_n)))
    descA[qs] = _noisy(point, 12, rng)
    descB[rows] = _noisy(point, 14, rng)
    seen = np.nonzero(map_index >= 0)[0]
    desc_map[map_index[seen]] = _noisy(point[seen], 10, rng)
    host = dict(match=match, featA=featA, featB=featB, map_X=map_X, map_match_a=map_match_a, descA=descA, descB=descB, desc_map=desc_map,
                Rt_source=p["Rt_source"], nq=nq, nt=nt, pair=p)
    dev = {k: _dev(host[k]) for k in ("match", "featA", "featB", "map_match_a", "descA", "descB", "desc_map")}
    _WORLDS[key] = (host, dev)
    return host, dev


def _pair_kw(h, d, seed, **more):
    return dict(d_match=d["match"].data_ptr(), nq=h["nq"], nt=h["nt"], cam_a=CAM_A, cam_b=CAM_B, d_feat_a=d["featA"].data_ptr(), feat_stride_a=4,
                d_feat_b=d["featB"].data_ptr(), feat_stride_b=2, img_wh=WH, seed=seed, **more)


def _dev_job(h, d, seed, chain, lower_is_b, **more):
    job = _pair_kw(h, d, seed, **more)
    job["Rt_source"] = h["Rt_source"]
    if chain:
        job.update(d_first_desc=(d["descB"] if lower_is_b else d["descA"]).data_ptr(), d_map_desc=d["desc_map"].data_ptr(), lower_is_b=lower_is_b)
    else:
        job.update(d_map_match_a=d["map_match_a"].data_ptr())
    return job


def _host_path(ctx, h, d, seed, chain, lower_is_b, map_match_a=None):
    """today's path: clc_pair_filter_dev, its host outputs into clc_inter_pose_batch"""
    from coloc_amd import abi
    f = ctx.pair_filter_dev("E", **_pair_kw(h, d, seed))
    prob = dict(x1=f["x1"], x2=f["x2"], K=K, wh=WH, seed=seed, Rt_source=h["Rt_source"])
    if chain:
        prob.update(d_first_desc=(d["descB"] if lower_is_b else d["descA"]).data_ptr(), first_feature=f["pair_t"] if lower_is_b else f["pair_q"],
                    d_map_desc=d["desc_map"].data_ptr())
    else:
        prob["map_index"] = (h["map_match_a"] if map_match_a is None else map_match_a)[f["pair_q"]]
    r = abi.inter_pose_batch([ctx], [prob], h["map_X"])[0]
    r["n_pairs"] = f["n_pairs"]
    return r


def _same(got, want, what):
    print(what, {k: (got[k], want[k]) for k in ("stage", "n_front", "n_common", "n_map_matches", "n_refined", "scale", "rmse")})
    assert got["status"] == 0 and want["status"] == 0, what
    for k in ("stage", "n_front", "n_common", "n_map_matches", "n_refined"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["inliers"], want["inliers"]), what
    for k in ("scale", "rmse", "Rt", "cov"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k, got[k], want[k])


# correspondences: inliers inside one wave / several waves / (2 000: about 1 400 inliers, 95 % of the points in the map) inliers, front
# points, common and kept features all across the 1 024-entry scan chunk, the scale terms across the chunk of the one-lane sum;
# map points: the chain's common-feature walk inside / across a chunk
@pytest.mark.parametrize("n,map_n,in_map", [(40, 300, 0.6), (150, 300, 0.6), (150, 2100, 0.6), (1300, 2100, 0.6), (2000, 2100, 0.95)])
def test_bit_identity_with_the_host_path(n, map_n, in_map):
    h, d = _world(9000 + n, n, map_n, in_map)
    ctx, ref = _light_ctx(), _light_ctx()
    try:
        ctx.set_map_points(h["map_X"])
        ok, most = 0, 0
        for chain in (False, True):
            for lower_is_b in (0, 1):
                seed = 3 + lower_is_b
                got = ctx.inter_pose_dev(**_dev_job(h, d, seed, chain, lower_is_b))
                want = _host_path(ref, h, d, seed, chain, lower_is_b)
                _same(got, want, (n, map_n, chain, lower_is_b))
                assert got["n_pairs"] == n
                ok += got["stage"] == 0
                most = max(most, len(got["inliers"]))
                if got["stage"] == 0:
                    assert 8 <= got["n_front"] <= len(got["inliers"]) and got["n_common"] >= 8 and got["n_refined"] > 0
                    assert (got["n_map_matches"] > 0) == chain
                if n == 2000:
                    assert len(got["inliers"]) > 1024 and got["n_front"] > 1024 and got["n_common"] > 1024, (len(got["inliers"]), got["n_front"], got["n_common"])
        assert most >= 13           # the front kernel ran (fewer inliers end at CLC_INTER_NO_MODEL on both sides)
        if n >= 150:
            assert ok == 4
    finally:
        ctx.close()
        ref.close()


def test_batch_equals_single():
    from coloc_amd import abi
    h, d = _world(9500, 600, 700)
    ctxs = [_light_ctx() for _ in range(4)]
    one = _light_ctx()
    try:
        for c in ctxs + [one]:
            c.set_map_points(h["map_X"])
        jobs = [_dev_job(h, d, 50 + i, chain=bool(i & 1), lower_is_b=i >> 1) for i in range(4)]
        for rep in range(2):                                        # (a second batch through the same contexts and blocks)
            got = abi.inter_pose_batch_dev(ctxs, jobs)
            for i in range(4):
                alone = one.inter_pose_dev(**jobs[i])
                assert alone["stage"] == 0
                _same(got[i], alone, ("batch", rep, i))
                assert np.array_equal(_bits(got[i]["E"]), _bits(alone["E"]))
    finally:
        for c in ctxs + [one]:
            c.close()


def test_stages():
    torch = _torch()
    h, d = _world(9600, 300, 300)
    ctx = _light_ctx()
    try:
        ctx.set_map_points(h["map_X"])
        # 9 correspondences: the filter keeps fewer than 13
        m9 = np.full(h["nq"], -1, dtype=np.int32)
        keep = np.nonzero(h["match"] >= 0)[0][:9]
        m9[keep] = h["match"][keep]
        d9 = _dev(m9)
        job = _dev_job(h, d, 1, False, 0)
        r = ctx.inter_pose_dev(**dict(job, d_match=d9.data_ptr()))
        assert r["status"] == 0 and r["n_pairs"] == 9 and r["stage"] == NO_MODEL and r["n_front"] == 0
        # no feature of the source frame is a map feature
        none = torch.full((h["nq"],), -1, dtype=torch.int32, device="cuda")
        far = _dev(np.where(h["map_match_a"] >= 0, h["map_match_a"] + 10 ** 6, -1).astype(np.int32))
        torch.cuda.synchronize()
        for mm in (none, far):
            r = ctx.inter_pose_dev(**dict(job, d_map_match_a=mm.data_ptr()))
            assert r["status"] == 0 and r["stage"] == NO_SCALE and r["n_front"] > 100 and r["n_common"] == 0, r["stage"]
            assert not r["Rt"].any() and not r["cov"].any() and r["scale"] == 0.0
        # the context is whole afterwards
        assert ctx.inter_pose_dev(**job)["stage"] == 0
        # wrong arguments
        from coloc_amd import CLCError, abi
        bad = [dict(job, d_first_desc=d["descA"].data_ptr()), dict(job, d_map_match_a=None),
               dict(job, d_first_desc=d["descA"].data_ptr(), d_map_desc=d["desc_map"].data_ptr()),          # both forms
               dict(job, d_map_match_a=d["map_match_a"].data_ptr() + 2), dict(job, d_feat_a=None)]
        for b in bad:
            with pytest.raises(CLCError) as e:
                ctx.inter_pose_dev(**b)
            assert e.value.status == abi.CLC_ERR_BAD_ARG
        empty = _light_ctx()
        try:
            with pytest.raises(CLCError) as e:
                empty.inter_pose_dev(**job)
            assert e.value.status == abi.CLC_ERR_STATE
        finally:
            empty.close()
    finally:
        ctx.close()


def _front_np(x1, x2, inliers, motions):
    """inter_relative's vote, term by term: per candidate the flags d1 > 0 and d2 > 0 in the inlier list's order"""
    def norm(x):
        n1 = (x[:, 1] - K[1, 2]) / K[1, 1]
        return (x[:, 0] - K[0, 2] - K[0, 1] * n1) / K[0, 0], n1
    p0, p1 = norm(x1[inliers])
    b0, b1 = norm(x2[inliers])
    flags = []
    for Rt in motions:
        a = [Rt[r, 0] * p0 + Rt[r, 1] * p1 + Rt[r, 2] * 1.0 for r in range(3)]
        t = Rt[:, 3]
        aa, bb = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], b0 * b0 + b1 * b1 + 1.0 * 1.0
        ab = a[0] * b0 + a[1] * b1 + a[2] * 1.0
        at, bt = a[0] * t[0] + a[1] * t[1] + a[2] * t[2], b0 * t[0] + b1 * t[1] + 1.0 * t[2]
        det = aa * bb - ab * ab
        det = np.where(np.abs(det) < 1e-18, 1e-18, det)
        d1, d2 = (-at * bb + bt * ab) / det, (-at * ab + bt * aa) / det
        flags.append((d1 > 0.0) & (d2 > 0.0))
    return flags


def test_front_kernel_alone():
    torch = _torch()
    p = _pair(9700, n=200, outliers=0.0)
    rng = np.random.default_rng(1)
    inliers = rng.permutation(200)[:150].astype(np.int32)             # an order of its own: the output follows the LIST, not the index
    R = p["Rd"] @ p["Rs"].T
    t = p["td"] - R @ p["ts"]
    t /= np.linalg.norm(t)
    R2 = (2.0 * np.outer(t, t) - np.eye(3)) @ R                       # the twisted pair
    true, behind = np.c_[R, t], np.c_[R, -t]
    four = np.stack([np.c_[R2, t], behind, np.c_[R2, -t], true])
    ctx = _light_ctx()
    try:
        p30 = dict(p, x2=_pair(9700, n=200)["x2"])                    # the same world with 30 % of the destination's features replaced
        clean, dirty = (_dev(p["x1"]), _dev(p["x2"])), (_dev(p30["x1"]), _dev(p30["x2"]))
        d_inl = _dev(inliers)
        cam = (1000.0, 640.0, 360.0, 0, 0, 0)

        def run(motions, pts=clean, d_inl=d_inl, n=200, ni=150):
            d_x1, d_x2 = pts
            Xt = torch.full((3 * ni,), np.nan, dtype=torch.float64, device="cuda")
            x2f = torch.full((2 * ni,), np.nan, dtype=torch.float64, device="cuda")
            corr = torch.full((ni,), -9, dtype=torch.int32, device="cuda")
            rec = torch.full((4,), -9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.inter_front_dev(d_x1.data_ptr(), d_x2.data_ptr(), n, d_inl.data_ptr(), ni, cam, cam, motions, Xt.data_ptr(), x2f.data_ptr(),
                                corr.data_ptr(), rec.data_ptr())
            ctx.sync()
            n_front, chosen, stage, ready = rec.cpu().tolist()
            assert ready == 1
            assert (corr.cpu().numpy()[n_front:] == -9).all() and torch.isnan(Xt[3 * n_front:]).all()      # nothing past the count
            return n_front, chosen, stage, corr.cpu().numpy()[:n_front]

        n_front, chosen, stage, _ = run(np.stack([true] * 4))
        assert (chosen, stage) == (0, 0) and n_front > 140            # the first maximum
        n_front, chosen, stage, _ = run(np.stack([behind] * 4))
        assert (n_front, chosen, stage) == (0, -1, NO_RELATIVE_POSE)
        n_front, chosen, stage, corr = run(four, dirty)
        flags = _front_np(p30["x1"], p30["x2"], inliers, four)
        counts = [int(f.sum()) for f in flags]
        assert chosen == int(np.argmax(counts)) == 3 and stage == 0 and n_front == counts[3] and 100 < n_front < 150      # a proper subset
        assert np.array_equal(corr, inliers[flags[3]])
        pos = np.argsort(inliers)[np.searchsorted(np.sort(inliers), corr)]          # where each kept correspondence stands in the list
        assert (np.diff(pos) > 0).all()
        # more than 1 024 given inliers: the vote's counts and the compaction's positions carry over from one pass of 1 024 to the next
        big = _pair(9710, n=1500)
        inl_big = rng.permutation(1500)[:1400].astype(np.int32)
        Rb = big["Rd"] @ big["Rs"].T
        tb = big["td"] - Rb @ big["ts"]
        tb /= np.linalg.norm(tb)
        Rb2 = (2.0 * np.outer(tb, tb) - np.eye(3)) @ Rb
        four_b = np.stack([np.c_[Rb2, tb], np.c_[Rb, -tb], np.c_[Rb, tb], np.c_[Rb2, -tb]])
        n_front, chosen, stage, corr = run(four_b, (_dev(big["x1"]), _dev(big["x2"])), _dev(inl_big), 1500, 1400)
        flags = _front_np(big["x1"], big["x2"], inl_big, four_b)
        counts = [int(f.sum()) for f in flags]
        assert chosen == int(np.argmax(counts)) == 2 and stage == 0 and n_front == counts[2] and 1024 < n_front < 1400
        assert np.array_equal(corr, inl_big[flags[2]])
    finally:
        ctx.close()


def test_after_stream_orders_the_call_behind_the_producer():
    """d_match and camera A's map match are written on torch's current stream behind a stretch of other work, with no host
    synchronisation before the call: only the event recorded on after_stream puts the pair launch -- and everything behind it -- there"""
    torch = _torch()
    h, d = _world(9800, 1000, 700)
    ctx = _light_ctx()
    try:
        ctx.set_map_points(h["map_X"])
        want = ctx.inter_pose_dev(**_dev_job(h, d, 1, False, 0))
        assert want["stage"] == 0
        d_match = torch.full((h["nq"],), -1, dtype=torch.int32, device="cuda")
        d_mm = torch.full((h["nq"],), -1, dtype=torch.int32, device="cuda")
        a = torch.randn(2048, 2048, device="cuda")
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            for _ in range(20):
                a = (a @ a) * 1e-3
            d_match.copy_(d["match"])
            d_mm.copy_(d["map_match_a"])
            job = _dev_job(h, d, 1, False, 0, after_stream=torch.cuda.current_stream().cuda_stream)
            got = ctx.inter_pose_dev(**dict(job, d_match=d_match.data_ptr(), d_map_match_a=d_mm.data_ptr()))
        _same(got, want, "after_stream")
        torch.cuda.synchronize()
    finally:
        ctx.close()

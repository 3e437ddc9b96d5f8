"""The track path and the pair path share one gather kernel skeleton and one gather-then-solve driver (coloc_amd/csrc/gather.hip,
pose_batch.hip: gather_solve) but keep a block each on the context.  What the sharing newly makes possible is state crossing from one
path into the other, so: the two paths alternated on the SAME contexts -- tracks, pairs 'F', other tracks, pairs 'E' -- must give, bit
for bit, what each call gives alone on fresh contexts.  Once as single calls on one context, once as batches of 3 on three.

Inputs: the generators of test_gpu_track_localize.py / test_gpu_pair_filter.py at 300 correspondences (about 30 % outliers, a few rounds
per solve), their query rows scattered over nq = 1 100 rows: two passes of the kernel's 1 024 threads, the second partial."""
import numpy as np
import pytest

import test_gpu_pair_filter as P
import test_gpu_track_localize as T
import track_host

pytestmark = pytest.mark.gpu

NQ, N = 1100, 300
CAM_T = T.CAM0 + track_host.DISTORTIONS[1]
CAM_A, CAM_B = P.F0 + track_host.DISTORTIONS[1], P.F0 + track_host.DISTORTIONS[2]


def _spread(match, feat, seed):
    """the generator's query rows, in their order, on NQ rows with accepted matches in both passes"""
    pos = np.sort(np.random.default_rng(seed).choice(NQ, len(match), replace=False))
    m = np.full(NQ, -1, dtype=np.int32)
    f = np.zeros((NQ, feat.shape[1]), dtype=np.float32)
    m[pos], f[pos] = match, feat
    assert (m[:1024] >= 0).any() and (m[1024:] >= 0).any() and (m >= 0).sum() == N
    return m, f


def _track_call(seeds):
    """one clc_track_localize(_batch)_dev call, len(seeds) jobs on one shared map -> f(ctxs) -> list of result dicts"""
    from coloc_amd import abi
    map_X = np.random.default_rng(seeds[0]).uniform(-5, 5, (N * len(seeds) + 50, 3)) + [0, 0, 12]
    dev = []
    for j, seed in enumerate(seeds):
        match, feat, _ = T._scattered_scene(N, seed, CAM_T, map_off=N * j, map_X=map_X)
        dev.append(tuple(T._dev(a) for a in _spread(match, feat, seed)))
    jobs = [dict(d_match=dm.data_ptr(), nq=NQ, cam=CAM_T, d_feat=df.data_ptr(), feat_stride=4, seed=seeds[j], refine=True)
            for j, (dm, df) in enumerate(dev)]

    def call(ctxs, _keep=dev):
        ctxs[0].set_map_points(map_X)
        got = [ctxs[0].track_localize_dev(**jobs[0])] if len(ctxs) == 1 else abi.track_localize_batch_dev(ctxs, jobs)
        assert all(r["n_tracks"] == N and r["Rt"] is not None and r["iterations"] > 0 and r["track_query"][-1] >= 1024 for r in got)
        return got
    return call


def _pair_call(model, seeds):
    from coloc_amd import abi
    dev, jobs = [], []
    for seed in seeds:
        match, fa, fb = P._scattered_pair(model, N, seed, CAM_A, CAM_B)
        match, fa = _spread(match, fa, seed)
        dev.append(tuple(P._dev(a) for a in (match, fa, fb)))
        jobs.append(P._job(match, fa, fb, CAM_A, CAM_B, *dev[-1], seed))

    def call(ctxs, _keep=dev):
        got = [ctxs[0].pair_filter_dev(model, **jobs[0])] if len(ctxs) == 1 else abi.pair_filter_batch_dev(ctxs, model, jobs)
        assert all(r["n_pairs"] == N and r["M"] is not None and r["iterations"] > 0 and r["pair_q"][-1] >= 1024 for r in got)
        return got
    return call


def _same(got, want, what):
    """every output: counts, index lists, mirrors, model, inliers, error_max, iterations, ... -- bit for bit"""
    assert got.keys() == want.keys(), what
    for k, w in want.items():
        g = got[k]
        if isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(T._bits(g), T._bits(w)), (what, k)
        else:
            assert type(g) is type(w) and g == w, (what, k, g, w)


@pytest.mark.parametrize("n_ctx", [1, 3])
def test_alternating_paths_equal_the_calls_alone(n_ctx):
    seeds = lambda s: [s + 10 * j for j in range(n_ctx)]
    calls = [("tracks", _track_call(seeds(8100))), ("pairs 'F'", _pair_call("F", seeds(8200))),
             ("other tracks", _track_call(seeds(8300))), ("pairs 'E'", _pair_call("E", seeds(8400)))]
    alone = []
    for _, call in calls:
        fresh = [T._light_ctx() for _ in range(n_ctx)]
        try:
            alone.append(call(fresh))
        finally:
            for c in fresh:
                c.close()
    ctxs = [T._light_ctx() for _ in range(n_ctx)]
    try:
        for (what, call), want in zip(calls, alone):
            for j, (g, w) in enumerate(zip(call(ctxs), want)):
                _same(g, w, (what, n_ctx, j))
    finally:
        for c in ctxs:
            c.close()

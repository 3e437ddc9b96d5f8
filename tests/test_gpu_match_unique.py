"""The one-to-one filter on the device (include/coloc_hip.h: clc_match_unique_dev, clc_match_unique_batch_dev, clc_match_2nn_unique_dev,
clc_match_map_unique_dev, clc_match_map_binned_unique_dev, clc_match_2nn_unique).  Every comparison is EXACT against the host statement
(tests/unique_host.py), for d_match and for d_owner.

The two kernels run 256 threads a workgroup, one thread per query (claim) or per query and train row (resolve), so the shapes straddle a
wave (63, 64, 65), a workgroup (257) and several workgroups (1000) on either side.  Where a test is about doubled train rows, that the
producer's plain result holds them is asserted first."""
import os

import numpy as np
import pytest

import bin_host as bh
import guided_host as gh
import map_host
import proj_host as ph
import unique_host as uh
import test_gpu_map_build as tmb                     # the tracks builder on the device from host pair lists
import test_gpu_map_guided as tg                     # the map matches' job buffers

pytestmark = pytest.mark.gpu

_dev, _torch = tg._dev, tg._torch
INT32_MIN = -2 ** 31


def _ctx(maxkp=4096, formulation=None):
    from coloc_amd import Context
    ctx = Context(device=0, detector=False, maxkp=maxkp)
    if formulation:
        ctx.set_k2nn_formulation(formulation)
    return ctx


class _Lists:
    """device copies of one job's lists, the outputs poisoned; nq / nt may be 0 (the buffers then hold one unused entry)"""

    def __init__(self, match, best, nt, owner=True):
        torch = _torch()
        self.nq, self.nt = len(match), nt
        self.match = _dev(np.concatenate([np.asarray(match, dtype=np.int32), np.array([-7], dtype=np.int32)]))
        self.best = _dev(np.concatenate([np.asarray(best, dtype=np.uint16), np.array([7], dtype=np.uint16)]).view(np.int16))
        self.owner = torch.full((nt + 1,), -7, dtype=torch.int32, device="cuda") if owner else None
        torch.cuda.synchronize()

    def kw(self):
        return dict(d_match=self.match.data_ptr(), d_best=self.best.data_ptr(), nq=self.nq, nt=self.nt,
                    d_owner=self.owner.data_ptr() if self.owner is not None else None)

    def result(self):
        m = self.match.cpu().numpy()
        assert m[self.nq] == -7                                               # nothing is written past the lists
        if self.owner is None:
            return m[:self.nq], None
        o = self.owner.cpu().numpy()
        assert o[self.nt] == -7
        return m[:self.nq], o[:self.nt]


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "match", int((got[0] != want[0]).sum()))
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "owner", int((got[1] != want[1]).sum()))


def _filter(ctx, match, best, nt, what, owner=True):
    job = _Lists(match, best, nt, owner)
    ctx.match_unique_dev(**job.kw())
    ctx.sync()
    got = job.result()
    _same(got, uh.unique(match, best, nt), what)
    return got


def _random_lists(rng, nq, nt):
    """random claims with many ties, a fifth of the entries -1"""
    match = rng.randint(0, nt, nq).astype(np.int32)
    match[rng.rand(nq) < 0.2] = -1
    best = rng.randint(0, 513, nq).astype(np.uint16)
    if rng.rand() < 0.5:
        best = (best // 32).astype(np.uint16)
    return match, best


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 257, 1000])
def test_filter_shapes_equal_the_statement(nq):
    rng = np.random.RandomState(100 + nq)
    ctx = _ctx()
    try:
        for nt in (1, 2, 64, 65, 300):
            match, best = _random_lists(rng, nq, nt)
            got = _filter(ctx, match, best, nt, (nq, nt))
            if nq >= 257 and nt <= 65:
                assert (got[0] >= 0).sum() < (match >= 0).sum()                # claims were lost: the filter had work
    finally:
        ctx.close()


def test_filter_cases():
    ctx = _ctx(maxkp=8192)
    try:
        _filter(ctx, np.full(300, -1, np.int32), np.zeros(300, np.uint16), 70, "all -1")
        # every query claims row 0: the smallest distance, then the lowest row
        rng = np.random.RandomState(3)
        best = rng.randint(5, 513, 4096).astype(np.uint16)
        best[[1234, 3000]] = 2
        got = _filter(ctx, np.zeros(4096, np.int32), best, 3, "every query claims row 0")
        assert got[1].tolist() == [1234, -1, -1] and (got[0] >= 0).sum() == 1
        got = _filter(ctx, np.zeros(4096, np.int32), np.full(4096, 9, np.uint16), 1, "every query claims row 0 at one distance")
        assert got[1].tolist() == [0]
        # equal distances on one row: the lowest query wins; a smaller distance beats a lower row
        got = _filter(ctx, [3, 3, 3, 1, 1], [7, 7, 7, 9, 8], 5, "ties")
        assert got[0].tolist() == [3, -1, -1, -1, 1] and got[1].tolist() == [-1, 4, -1, 0, -1]
        # distances 0 and 512 claim; rows nt, nt + 5, -2, INT32_MIN and a distance of 65535 beside a row do not: all become -1
        nt = 4
        match = np.array([0, 0, 1, 2, nt, nt + 5, -2, INT32_MIN, 3, -1], dtype=np.int32)
        best = np.array([512, 0, 512, 513, 1, 1, 1, 1, 65535, 0], dtype=np.uint16)
        got = _filter(ctx, match, best, nt, "sanitising")
        assert got[0].tolist() == [-1, 0, 1, -1, -1, -1, -1, -1, -1, -1] and got[1].tolist() == [1, 2, -1, -1]
        # d_owner null
        match, best = _random_lists(rng, 300, 65)
        _filter(ctx, match, best, 65, "no owner", owner=False)
        # nq == 0: d_match untouched, every owner -1; nt == 0: every entry -1
        got = _filter(ctx, np.zeros(0, np.int32), np.zeros(0, np.uint16), 70, "nq == 0")
        assert (got[1] == -1).all() and len(got[1]) == 70
        got = _filter(ctx, np.array([0, 5, -1, -2], np.int32), np.array([1, 2, 3, 4], np.uint16), 0, "nt == 0")
        assert (got[0] == -1).all()
        _filter(ctx, np.zeros(0, np.int32), np.zeros(0, np.uint16), 0, "nq == nt == 0")
    finally:
        ctx.close()


def test_called_twice_and_replayed_from_a_graph_no_stale_claim_survives():
    """the claim words are armed on every call: a second call with other lists in the same buffers, and a captured call replayed three
    times with new contents, equal the statement every time (eager once, capture on one stream, replays: tests/test_gpu_graph.py)"""
    torch = _torch()
    nq, nt = 1000, 257
    rng = np.random.RandomState(11)
    ctx = _ctx()
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.Stream(device=dev)
        sp = st.cuda_stream
        d_match = torch.zeros((nq,), dtype=torch.int32, device=dev)
        d_best = torch.zeros((nq,), dtype=torch.int16, device=dev)
        d_owner = torch.full((nt,), -7, dtype=torch.int32, device=dev)

        def fill(k):
            match, best = _random_lists(rng, nq, nt)
            if k % 2:
                match[match >= 0] = match[match >= 0] % 40                     # other rows claimed, most rows free
            d_match.copy_(torch.from_numpy(match)); d_best.copy_(torch.from_numpy(best.view(np.int16))); d_owner.fill_(-7)
            torch.cuda.synchronize()  # the fill runs on torch's stream, the library on another: order them
            return uh.unique(match, best, nt)

        def step():
            ctx.match_unique_dev(d_match.data_ptr(), d_best.data_ptr(), nq, nt, d_owner.data_ptr(), sp)

        for k in range(2):                                                      # called twice, eagerly
            want = fill(k)
            with torch.cuda.stream(st):
                step()
            torch.cuda.synchronize()
            _same((d_match.cpu().numpy(), d_owner.cpu().numpy()), want, ("eager", k))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            step()
        for k in range(3):
            want = fill(k + 1)
            g.replay()
            torch.cuda.synchronize()
            _same((d_match.cpu().numpy(), d_owner.cpu().numpy()), want, ("replay", k))
            assert (want[1] == -1).any() and (want[1] >= 0).any()
    finally:
        ctx.close()


def test_batch_of_unequal_jobs_equals_the_single_calls():
    rng = np.random.RandomState(21)
    shapes = [(1000, 300), (65, 2), (0, 64), (257, 0), (300, 1000)]
    ctx = _ctx()
    try:
        lists = [(_random_lists(rng, nq, max(nt, 1)) if nq else (np.zeros(0, np.int32), np.zeros(0, np.uint16))) + (nt,) for nq, nt in shapes]
        jobs = [_Lists(m, b, nt, owner=(i != 1)) for i, (m, b, nt) in enumerate(lists)]
        ctx.match_unique_batch_dev([j.kw() for j in jobs])
        ctx.sync()
        for i, (j, (m, b, nt)) in enumerate(zip(jobs, lists)):
            single = _Lists(m, b, nt, owner=(i != 1))
            ctx.match_unique_dev(**single.kw())
            ctx.sync()
            _same(j.result(), single.result(), ("batch == single", i))
            _same(j.result(), uh.unique(m, b, nt), ("batch == statement", i))
        ctx.match_unique_batch_dev([])                                          # nothing to do
    finally:
        ctx.close()


def _pair_with_doubles(nq, nt, dup, seed):
    """T: nt random rows; Q: near-copies (at most 30 bits) of rows 0 .. nq - dup - 1 and SECOND near-copies (at most 40 bits) of rows
    0 .. dup - 1 behind them"""
    rng = np.random.RandomState(seed)
    assert dup <= nq - dup <= nt
    T = rng.randint(0, 256, (nt, 64)).astype(np.uint8)
    Q = np.array([uh._flip(rng, T[i], 30) for i in range(nq - dup)] + [uh._flip(rng, T[i], 40) for i in range(dup)], dtype=np.uint8)
    return Q, T


@pytest.mark.parametrize("formulation", ["matrix", "popcount"])
def test_pair_entry_equals_the_host_match_and_the_statement(oracle, formulation):
    torch = _torch()
    ctx = _ctx(formulation=formulation)
    try:
        for nq, nt, dup in ((300, 257, 43), (1000, 1000, 100)):
            Q, T = _pair_with_doubles(nq, nt, dup, 10 * nq + nt)
            plain_o = oracle.k2nn(Q, T, 40)
            assert len(uh.doubled_rows(plain_o)) >= dup // 2, "the plain result must hold the planted doubles"
            plain, best, _ = ctx.match_2nn(Q, T, 40, want_dist=True)         # the host entry, with its distances
            assert np.array_equal(plain, plain_o)
            want = uh.unique(plain, best, nt)
            d_q, d_t = _dev(Q), _dev(T)
            d_match = torch.full((nq + 1,), -7, dtype=torch.int32, device="cuda")
            d_owner = torch.full((nt + 1,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.match_2nn_unique_dev(d_q.data_ptr(), nq, d_t.data_ptr(), nt, 40, d_match.data_ptr(), d_owner.data_ptr())
            ctx.sync()
            m, o = d_match.cpu().numpy(), d_owner.cpu().numpy()
            assert m[nq] == -7 and o[nt] == -7
            _same((m[:nq], o[:nt]), want, (formulation, nq, nt))
            assert (want[0] >= 0).sum() <= (plain >= 0).sum() - dup // 2 and len(uh.doubled_rows(m[:nq])) == 0
            # the host entry: the _dev entry's result
            hm, ho = ctx.match_unique(Q, T, 40)
            _same((hm, ho), want, (formulation, "host entry", nq, nt))
    finally:
        ctx.close()


def test_host_entry_re_sweeps_an_edited_published_block():
    """a block published under VERIFY and edited afterwards: the sweep on the published rows is repeated on the caller's rows, and the
    filter stands behind the sweep whose result is returned"""
    from coloc_amd import abi
    nq, nt, dup = 300, 257, 43
    Q, T = _pair_with_doubles(nq, nt, dup, 5)
    ctx = _ctx()
    try:
        abi.load_library().clc_desc_cache_clear()
        ctx.desc_cache_mode("verify")
        d_q = _dev(Q)
        handle = ctx.desc_cache_publish(Q, d_src=d_q.data_ptr())
        assert abi.desc_handle_live(handle)
        before = ctx.match_unique(Q, T, 40)                                    # the published rows serve
        assert abi.desc_handle_live(handle)
        rng = np.random.RandomState(6)
        for i in range(60, 120):                                                # rows 60 .. 119 become THIRD near-copies of rows 0 .. 59
            Q[i] = uh._flip(rng, T[i - 60], 20)
        plain, best, _ = _ctx_plain(Q, T)
        want = uh.unique(plain, best, nt)
        assert not np.array_equal(want[0], before[0]) and len(uh.doubled_rows(plain)) >= dup
        got = ctx.match_unique(Q, T, 40)
        assert not abi.desc_handle_live(handle)                                 # the lookup saw the edit: the block was uploaded and swept again
        _same(got, want, "edited block")
    finally:
        abi.load_library().clc_desc_cache_clear()
        ctx.close()


def _ctx_plain(Q, T):
    """clc_match_2nn on a context of its own with the cache off: the caller's rows, uploaded"""
    c = _ctx()
    try:
        c.desc_cache_mode("off")
        return c.match_2nn(Q, T, 40, want_dist=True)
    finally:
        c.close()


def test_map_entry_equals_match_map_dev_and_the_statement(oracle):
    torch = _torch()
    nq, nm, dup = 300, 257, 43
    Q, M = _pair_with_doubles(nq, nm, dup, 77)
    ctx = _ctx()
    try:
        ctx.set_map(M)
        d_q = _dev(Q)
        d_plain = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        d_match = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        d_owner = torch.full((nm,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.match_map_dev(d_q.data_ptr(), nq, 60, d_plain.data_ptr())
        ctx.match_map_unique_dev(d_q.data_ptr(), nq, 60, d_match.data_ptr(), d_owner.data_ptr())
        ctx.sync()
        plain_o, best, _ = oracle.k2nn(Q, M, 60, want_dist=True)
        plain = d_plain.cpu().numpy()
        assert np.array_equal(plain, plain_o) and len(uh.doubled_rows(plain)) >= dup // 2
        _same((d_match.cpu().numpy(), d_owner.cpu().numpy()), uh.unique(plain, best, nm), "map entry")
    finally:
        ctx.close()


def _binned_case(nq, nm, seed):
    """tests/proj_host.py's case with a SECOND keypoint half a pixel beside every fifth query, carrying a near-copy of its descriptor: two
    keypoints in one window that take the same landmark"""
    Q, M, qpos, X = ph.make_case(nq, nm, seed, behind=False)
    rng = np.random.RandomState(seed + 1)
    twins = np.arange(0, nq, 5)
    Q2 = np.concatenate([Q, np.array([gh._flip(rng, Q[i], 3) for i in twins], dtype=np.uint8)])
    qpos2 = np.concatenate([qpos, qpos[twins] + np.float32([0.5, 0.0])]).astype(np.float32)
    return Q2, M, qpos2, X


@pytest.mark.parametrize("radius,plan", [(3.0, bh.BINNED), (2000.0, bh.SWEEP)])
def test_binned_entry_equals_the_binned_match_and_the_statement(monkeypatch, radius, plan):
    torch = _torch()
    nq0, nm, thr = 300, 513, 20
    Q, M, qpos, X = _binned_case(nq0, nm, 41)
    nq = len(Q)
    ctx = tg._ctx(monkeypatch, M=M, X=X)
    try:
        assert ctx.map_binned_plan(gh.CAM_EXACT, radius)["plan"] == plan == bh.plan(gh.CAM_EXACT, radius, nm)
        prod = tg._Job(Q, nm, ph.IDENTITY, radius, thr, gh.CAM_EXACT, feat=qpos)
        ctx.match_map_binned_dev(**prod.kw)
        ctx.sync()
        p = prod.result()
        print("plan %d: %d accepted, %d doubled landmarks" % (plan, (p["match"] >= 0).sum(), len(uh.doubled_rows(p["match"]))))
        assert len(uh.doubled_rows(p["match"])) >= 5, "the producer's result must hold doubled landmarks"
        want = uh.unique(p["match"], p["best"], nm)
        for with_best in (True, False):
            job = tg._Job(Q, nm, ph.IDENTITY, radius, thr, gh.CAM_EXACT, feat=qpos)
            d_owner = torch.full((nm,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            kw = dict(job.kw) if with_best else {k: v for k, v in job.kw.items() if k != "d_best"}
            ctx.match_map_binned_unique_dev(d_owner=d_owner.data_ptr(), **kw)
            ctx.sync()
            got = job.result()
            _same((got["match"], d_owner.cpu().numpy()), want, (plan, with_best))
            assert np.array_equal(got["second"], p["second"]) and gh.same_bits(got["qpos"], p["qpos"]) and gh.same_bits(got["proj"], p["proj"])
            if with_best:
                assert np.array_equal(got["best"], p["best"])                   # the producer's own outputs are as it leaves them
            else:
                assert (job.best.cpu().numpy() == 7).all()                      # not the caller's array: the context's scratch
    finally:
        ctx.close()


def test_tracks_from_the_filtered_pair_lists():
    """the CPU recipe at a small n, through the device: clc_match_2nn_unique_dev per pair, then clc_tracks_build_dev over the lists equals
    the host tracks builder on them and has more tracks than over the plain lists"""
    torch = _torch()
    n, dup = 120, 20
    cams = uh.three_cameras(n, dup, 7)
    rows = [len(c) for c in cams]
    ctx = _ctx()
    try:
        d = [_dev(c) for c in cams]
        plain, filtered = [], []
        for a, b in uh.PAIRS:
            d_m = torch.full((rows[a],), -7, dtype=torch.int32, device="cuda")
            d_u = torch.full((rows[a],), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.match_2nn_dev(d[a].data_ptr(), rows[a], d[b].data_ptr(), rows[b], 40, d_m.data_ptr())
            ctx.match_2nn_unique_dev(d[a].data_ptr(), rows[a], d[b].data_ptr(), rows[b], 40, d_u.data_ptr())
            ctx.sync()
            plain.append(d_m.cpu().numpy())
            filtered.append(d_u.cpu().numpy())
            assert len(uh.doubled_rows(filtered[-1])) == 0
        assert sum(len(uh.doubled_rows(m)) for m in plain) >= dup
        t_plain = tmb._tracks_on_device(ctx, rows, uh.pair_lists(plain))
        t_unique = tmb._tracks_on_device(ctx, rows, uh.pair_lists(filtered))
        assert np.array_equal(t_plain, map_host.build_tracks(rows, uh.pair_lists(plain)))
        assert np.array_equal(t_unique, map_host.build_tracks(rows, uh.pair_lists(filtered)))
        print("n %d dup %d on the device: tracks %d -> %d" % (n, dup, len(t_plain), len(t_unique)))
        assert len(t_unique) > len(t_plain)
    finally:
        ctx.close()


def test_errors():
    from coloc_amd import CLCError, Context, abi
    torch = _torch()
    rng = np.random.RandomState(1)
    match, best = _random_lists(rng, 64, 10)
    job = _Lists(match, best, 10)
    kw = job.kw()
    ctx = _ctx()
    light = Context(device=0, detector=False, matcher=False)
    try:
        d_q = _dev(rng.randint(0, 256, (64, 64)).astype(np.uint8))
        ctx.set_map(np.zeros((10, 64), dtype=np.uint8))
        big = (1 << 22) + 1

        def refused(status, call, *args, **kws):
            with pytest.raises(CLCError) as e:
                call(*args, **kws)
            assert e.value.status == status, (call.__name__, args, kws)

        # more than 2^22 query rows: refused before anything is allocated or enqueued (nothing of that size exists here)
        refused(abi.CLC_ERR_CAPACITY, ctx.match_unique_dev, **dict(kw, nq=big))
        refused(abi.CLC_ERR_CAPACITY, ctx.match_unique_batch_dev, [kw, dict(kw, nq=big)])
        refused(abi.CLC_ERR_CAPACITY, ctx.match_2nn_unique_dev, d_q.data_ptr(), big, d_q.data_ptr(), 64, 40, kw["d_match"], kw["d_owner"])
        refused(abi.CLC_ERR_CAPACITY, ctx.match_map_unique_dev, d_q.data_ptr(), big, 40, kw["d_match"], kw["d_owner"])
        assert ctx.lib.clc_match_unique_dev(ctx.h, None, None) == abi.CLC_ERR_BAD_ARG                     # a null job
        # misaligned pointers, null lists, negative counts, a job count out of range
        for b in (dict(kw, d_match=kw["d_match"] + 2), dict(kw, d_best=kw["d_best"] + 1), dict(kw, d_owner=kw["d_owner"] + 2),
                  dict(kw, d_match=None), dict(kw, d_best=None), dict(kw, nq=-1), dict(kw, nt=-1)):
            refused(abi.CLC_ERR_BAD_ARG, ctx.match_unique_dev, **b)
            refused(abi.CLC_ERR_BAD_ARG, ctx.match_unique_batch_dev, [kw, b])
        refused(abi.CLC_ERR_BAD_ARG, ctx.match_unique_batch_dev, [kw] * (abi.MAX_TRACK_PAIRS + 1))
        refused(abi.CLC_ERR_BAD_ARG, ctx.match_2nn_unique_dev, d_q.data_ptr(), 64, d_q.data_ptr(), 64, 40, kw["d_match"] + 2, kw["d_owner"])
        refused(abi.CLC_ERR_BAD_ARG, ctx.match_2nn_unique_dev, d_q.data_ptr(), 64, d_q.data_ptr(), 64, 40, kw["d_match"], kw["d_owner"] + 2)
        refused(abi.CLC_ERR_BAD_ARG, ctx.match_2nn_unique_dev, d_q.data_ptr() + 8, 64, d_q.data_ptr(), 64, 40, kw["d_match"], kw["d_owner"])
        refused(abi.CLC_ERR_BAD_ARG, ctx.match_map_unique_dev, d_q.data_ptr(), 64, 40, kw["d_match"], kw["d_owner"] + 2)
        # a context without matcher options
        refused(abi.CLC_ERR_STATE, light.match_unique_dev, **kw)
        refused(abi.CLC_ERR_STATE, light.match_unique_batch_dev, [kw])
        refused(abi.CLC_ERR_STATE, light.match_2nn_unique_dev, d_q.data_ptr(), 64, d_q.data_ptr(), 64, 40, kw["d_match"], kw["d_owner"])
        refused(abi.CLC_ERR_STATE, light.match_map_unique_dev, d_q.data_ptr(), 64, 40, kw["d_match"], kw["d_owner"])
        refused(abi.CLC_ERR_STATE, light.match_unique, np.zeros((4, 64), np.uint8), np.zeros((4, 64), np.uint8))
        ctx.sync()
        got = job.result()
        assert np.array_equal(got[0], match) and (got[1] == -7).all()           # nothing was enqueued by any of them
        ctx.match_unique_dev(**kw)                                              # the context is usable afterwards
        ctx.sync()
        _same(job.result(), uh.unique(match, best, 10), "after the refusals")
    finally:
        ctx.close()
        light.close()

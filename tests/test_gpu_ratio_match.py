"""GPU parity of the distance-ratio matcher (CPUMatcher's rule, include/coloc_hip.h clc_match_ratio_*) against the CPU oracle:
per-query results bit for bit with orc_k2nn_omp_ex rule 1, the pair lists with orc_cpumatcher_pair, under both formulations of the
sweep.  The host half alone is tests/test_ratio_match_host.py."""
import ctypes as C

import numpy as np
import pytest

import synth
from test_ratio_match_host import pairs_without_positions, ratio_scene

pytestmark = pytest.mark.gpu

RATIOS = [0.6, 0.8, 1.0, 1.25]


@pytest.fixture(autouse=True, params=["matrix", "popcount"])
def k2nn_formulation(request, gpu_ctx):
    gpu_ctx.set_k2nn_formulation(request.param)
    yield request.param
    gpu_ctx.set_k2nn_formulation("matrix")


_want = {}


def oracle_ratio(oracle, Q, T, ratio, key=None):
    """orc_k2nn_omp_ex(rule = 1): per query the train row or -1 (cached across the two formulations when `key` is given)"""
    if key is not None and (key, ratio) in _want:
        return _want[(key, ratio)]
    m, _ = oracle.k2nn_omp(Q, T, rule=1, ratio=ratio)
    if key is not None:
        _want[(key, ratio)] = m
    return m


@pytest.mark.parametrize("nq,nt", [(1, 1), (5, 1), (5, 2), (257, 513), (1000, 3000), (4096, 4097), (10000, 10000)])
def test_ratio_indices_bit_identical(gpu_ctx, oracle, nq, nt):
    Q, T = synth.planted_descriptors(nq, nt, seed=100 + nq + nt, frac=0.5, max_flip=80)
    m2, b2, s2 = gpu_ctx.match_2nn(Q, T, 40, want_dist=True)
    for r in RATIOS:
        m, b, s = gpu_ctx.match_ratio(Q, T, r, want_dist=True)
        want = oracle_ratio(oracle, Q, T, r, key=(nq, nt))
        assert np.array_equal(m, want), "ratio %g" % r
        assert np.array_equal(b, b2) and np.array_equal(s, s2)          # the distances do not depend on the rule
        if r == 0.8 and nt >= 2 and nq >= 1000:
            assert 0 < int((want >= 0).sum()) < nq                       # both branches taken


def chosen_distances(d_list, seed=0):
    """query 0 = zeros; train row k has d_list[k] bits set (its Hamming distance to the query)"""
    rng = np.random.default_rng(seed)
    T = np.zeros((len(d_list), 64), np.uint8)
    for k, d in enumerate(d_list):
        bits = np.zeros(512, np.uint8)
        bits[rng.choice(512, size=d, replace=False)] = 1
        T[k] = np.packbits(bits)
    return np.zeros((1, 64), np.uint8), T


@pytest.mark.parametrize("d1,d2", [(16, 25), (9, 25), (64, 100), (15, 25), (17, 25), (36, 100), (37, 100), (0, 1), (0, 0)])
def test_float_rounding_boundaries(gpu_ctx, oracle, d1, d2):
    """(d1, d2) on the line d1 = r^2 d2 for r = 0.8 / 0.6: float rounding of r * r decides; the GPU must decide as the oracle does"""
    for order in ([d1, d2, 200, 300], [300, d2, 200, d1], [d2, 300, d1]):
        Q, T = chosen_distances(order)
        for r in RATIOS:
            m = gpu_ctx.match_ratio(Q, T, r)
            assert np.array_equal(m, oracle_ratio(oracle, Q, T, r)), (order, r)


def test_ties_for_the_minimum(gpu_ctx, oracle):
    """d1 == d2: never a match for r <= 1; for r > 1 the lowest index (d1 > 0); d1 == d2 == 0 never passes"""
    Q, T = chosen_distances([90, 40, 70, 40, 40])
    for r in RATIOS:
        m = gpu_ctx.match_ratio(Q, T, r)
        assert np.array_equal(m, oracle_ratio(oracle, Q, T, r))
        assert m[0] == (1 if r > 1.0 else -1)
    Q, T = chosen_distances([5, 0, 0])
    assert gpu_ctx.match_ratio(Q, T, 1.25)[0] == -1


def test_fewer_than_two_train_rows_and_empty_queries(gpu_ctx):
    Q, T = synth.planted_descriptors(300, 2, seed=5)
    for nt in (0, 1):
        for r in RATIOS + [1e6]:
            assert (gpu_ctx.match_ratio(Q, T[:nt], r) == -1).all()
    assert gpu_ctx.match_ratio(Q[:0], T, 0.8).shape == (0,)
    assert gpu_ctx.match_ratio_pairs([Q[:0], T], [(1, 0)])[0].shape == (0, 2)


def test_train_set_beyond_22_bit_index_uses_slab_merge(oracle, k2nn_formulation):
    """nt > 2^22: per-split slabs + the ordered merge kernel, whose accept line applies the ratio rule"""
    from coloc_amd import Context
    nt, nq = (1 << 22) + 4099, 96
    ctx = Context(device=0, width=160, height=120, maxkp=nt, detector=False)
    ctx.set_k2nn_formulation(k2nn_formulation)
    rng = np.random.default_rng(13)
    T = rng.integers(0, 256, size=(nt, 64), dtype=np.uint8)
    Q = rng.integers(0, 256, size=(nq, 64), dtype=np.uint8)
    for i in range(0, 64, 2):
        src = int(rng.integers(0, nt)) if i % 4 else nt - 1 - i
        Q[i] = T[src]
        Q[i, i % 64] ^= 0x11
    T[nt - 3] = T[5]; Q[64] = T[5]                  # exact duplicate pair 5 / nt-3 -> tie at distance 0 -> never a match
    assert ctx.k2nn_plan_query(nq, nt)["atomic_merge"] == 0      # slab mode
    for r in (0.8, 1.25):
        m = ctx.match_ratio(Q, T, r)
        assert np.array_equal(m, oracle_ratio(oracle, Q, T, r))
        assert (m[:64:2] >= 0).all() and m[64] == -1
    assert (ctx.match_ratio(Q, T[:1], 0.8) == -1).all()
    ctx.close()


def test_ratio_and_k2nn_interleaved_on_one_context(gpu_ctx, oracle):
    rng = np.random.default_rng(21)
    for it in range(12):
        nq, nt = int(rng.integers(1, 6000)), int(rng.integers(0, 6000))
        Q, T = synth.planted_descriptors(nq, nt, seed=200 + it, frac=0.5, max_flip=80)
        r = RATIOS[it % 4]
        assert np.array_equal(gpu_ctx.match_ratio(Q, T, r), oracle_ratio(oracle, Q, T, r)), (nq, nt, r)
        assert np.array_equal(gpu_ctx.match_2nn(Q, T, 40), oracle.k2nn(Q, T, 40)), (nq, nt)


@pytest.mark.parametrize("n_db,n_q", [(2, 1), (700, 500), (3000, 4000), (10000, 10000)])
def test_ratio_pairs_equal_cpumatcher(gpu_ctx, oracle, n_db, n_q):
    D, xy_db, Q, xy_q = ratio_scene(n_db, n_q, seed=n_db + n_q)
    for r in (0.8, 1.25):
        want, _ = oracle.cpumatcher_pair(D, xy_db, Q, xy_q, ratio=r)
        got = gpu_ctx.match_ratio_pairs([D, Q], [(0, 1)], r, xys=[xy_db, xy_q])[0]
        assert got.dtype == np.int32 and np.array_equal(got, want)
        got = gpu_ctx.match_ratio_pairs([D, Q], [(0, 1)], r)[0]
        assert np.array_equal(got, pairs_without_positions(oracle_ratio(oracle, Q, D, r)))


def cameras(counts, seed):
    """descriptor sets that see a common scene: each camera holds noisy copies (<= 40 flipped bits) of rows of one base set, some rows
    twice, plus rows of its own; positions on a coarse grid, so that (x_I, y_I, x_J, y_J) repeats occur"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(3000, 64), dtype=np.uint8)
    descs, xys = [], []
    for n in counts:
        d = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
        k = (2 * n) // 3
        src = rng.integers(0, base.shape[0], size=k)
        bits = np.unpackbits(base[src], axis=1)
        flip = rng.random(bits.shape) < rng.uniform(0, 40 / 512, size=(k, 1))
        d[:k] = np.packbits(bits ^ flip, axis=1)
        if n >= 8:
            d[n - n // 8:] = d[:n // 8]                       # repeated rows
        descs.append(d)
        xys.append(rng.integers(0, 48, size=(n, 2)).astype(np.float32))
    return descs, xys


def test_four_cameras_all_pairs_equal_per_pair_calls(gpu_ctx, oracle):
    descs, xys = cameras((1200, 900, 1, 1500), seed=40)
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    allp = gpu_ctx.match_ratio_pairs(descs, pairs, 0.8, xys=xys)
    for (i, j), got in zip(pairs, allp):
        one = gpu_ctx.match_ratio_pairs([descs[i], descs[j]], [(0, 1)], 0.8, xys=[xys[i], xys[j]])[0]
        want, _ = oracle.cpumatcher_pair(descs[i], xys[i], descs[j], xys[j], ratio=0.8)
        assert np.array_equal(got, one) and np.array_equal(got, want), (i, j)
        if i == 2:
            assert got.shape == (0, 2)                              # a one-row database: no second distance, no match
        elif 2 not in (i, j):
            assert len(got) > 50
    # the reverse orientation is another pair; an empty camera gives empty lists
    rev = gpu_ctx.match_ratio_pairs(descs, [(1, 0)], 0.8, xys=xys)[0]
    assert np.array_equal(rev, oracle.cpumatcher_pair(descs[1], xys[1], descs[0], xys[0], ratio=0.8)[0])
    empty = np.zeros((0, 64), np.uint8)
    got = gpu_ctx.match_ratio_pairs([descs[0], empty], [(0, 1), (1, 0)], 0.8, xys=[xys[0], np.zeros((0, 2), np.float32)])
    assert [g.shape for g in got] == [(0, 2), (0, 2)]


def test_camera_without_rows_needs_no_positions(gpu_ctx, oracle):
    """a camera with no regions passes NULL positions (what an empty std::vector hands over): its pairs are empty, the others unharmed"""
    descs, xys = cameras((1200, 0, 1500), seed=41)
    pairs = [(0, 1), (1, 0), (0, 2), (1, 2), (2, 1)]
    got = gpu_ctx.match_ratio_pairs(descs, pairs, 0.8, xys=[xys[0], None, xys[2]])
    want = oracle.cpumatcher_pair(descs[0], xys[0], descs[2], xys[2], ratio=0.8)[0]
    assert len(want) > 50 and np.array_equal(got[2], want)
    assert [g.shape for k, g in enumerate(got) if k != 2] == [(0, 2)] * 4
    # map tracking against an empty map, or with an empty frame: no match, no positions needed for the empty side
    from coloc_amd import Context
    ctx = Context(device=0, width=160, height=120, maxkp=4000, detector=False)
    ctx.set_map(descs[1])
    assert ctx.match_map_ratio(descs[0], 0.8, None, xys[0]).shape == (0, 2)
    ctx.set_map(descs[0])
    assert ctx.match_map_ratio(descs[1], 0.8, xys[0], None).shape == (0, 2)
    assert np.array_equal(ctx.match_map_ratio(descs[2], 0.8, xys[0], xys[2]),
                          oracle.cpumatcher_pair(descs[0], xys[0], descs[2], xys[2], ratio=0.8)[0])
    ctx.close()


def test_map_ratio_equals_cpumatcher(gpu_ctx, oracle):
    import torch
    M, xy_m, F, xy_f = ratio_scene(6000, 3500, seed=77)
    gpu_ctx.set_map(M)
    want, _ = oracle.cpumatcher_pair(M, xy_m, F, xy_f, ratio=0.8)
    assert np.array_equal(gpu_ctx.match_map_ratio(F, 0.8, xy_m, xy_f), want)
    m = oracle_ratio(oracle, F, M, 0.8)
    assert np.array_equal(gpu_ctx.match_map_ratio(F, 0.8), pairs_without_positions(m))
    # the _dev forms equal the per-query host form
    d_f = torch.from_numpy(F).cuda()
    d_m = torch.from_numpy(M).cuda()
    out = torch.full((F.shape[0],), -7, dtype=torch.int32, device="cuda:0")
    out2 = torch.full((F.shape[0],), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()      # the fills run on torch's stream, the library on its own (non-blocking) one: order them
    gpu_ctx.match_map_ratio_dev(d_f.data_ptr(), F.shape[0], 0.8, out.data_ptr())
    gpu_ctx.match_ratio_dev(d_f.data_ptr(), F.shape[0], d_m.data_ptr(), M.shape[0], 0.8, out2.data_ptr())
    gpu_ctx.sync()
    assert np.array_equal(out.cpu().numpy(), m) and np.array_equal(out2.cpu().numpy(), m)
    assert np.array_equal(gpu_ctx.match_ratio(F, M, 0.8), m)
    gpu_ctx.match_ratio_dev(d_f.data_ptr(), 0, d_m.data_ptr(), M.shape[0], 0.8, out.data_ptr())     # nq = 0: nothing enqueued
    gpu_ctx.sync()


def test_published_block_edited_after_publication(oracle):
    """VERIFY mode (the default): a block published with its device rows and edited afterwards is matched on its edited rows"""
    import torch
    from coloc_amd import Context
    from coloc_amd.abi import desc_cache_stats
    ctx = Context(device=0, width=160, height=120, maxkp=8000, detector=False)
    D, xy_db, Q, xy_q = ratio_scene(3000, 2500, seed=91)
    d_q = torch.from_numpy(Q).cuda()
    d_d = torch.from_numpy(D).cuda()
    torch.cuda.synchronize()
    ctx.desc_cache_publish(Q, d_src=C.c_void_p(d_q.data_ptr()))
    ctx.desc_cache_publish(D, d_src=C.c_void_p(d_d.data_ptr()))
    h0 = desc_cache_stats()[0]
    got = ctx.match_ratio_pairs([D, Q], [(0, 1)], 0.8, xys=[xy_db, xy_q])[0]
    assert np.array_equal(got, oracle.cpumatcher_pair(D, xy_db, Q, xy_q, ratio=0.8)[0])
    assert desc_cache_stats()[0] >= h0 + 2                                   # both sets read where they were published
    Q[100:400] = D[1000:1300]                                                # queries edited in place: exact copies of database rows
    D[0] ^= 0xFF
    got = ctx.match_ratio_pairs([D, Q], [(0, 1)], 0.8, xys=[xy_db, xy_q])[0]
    assert np.array_equal(got, oracle.cpumatcher_pair(D, xy_db, Q, xy_q, ratio=0.8)[0])
    assert np.array_equal(ctx.match_ratio(Q, D, 0.8), oracle_ratio(oracle, Q, D, 0.8))
    assert (ctx.match_ratio(Q, D, 0.8)[100:400] == np.arange(1000, 1300)).all()
    ctx.close()


def test_error_codes(gpu_ctx):
    from coloc_amd import CLCError
    Q, T = synth.planted_descriptors(50, 60, seed=3)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(CLCError) as e:
            gpu_ctx.match_ratio(Q, T, bad)
        assert e.value.status == 1
        with pytest.raises(CLCError) as e:
            gpu_ctx.match_ratio_pairs([T, Q], [(0, 1)], bad)
        assert e.value.status == 1
    xy = np.zeros((50, 2), np.float32)
    with pytest.raises(CLCError) as e:                      # positions for one side of a pair only
        gpu_ctx.match_ratio_pairs([T, Q], [(0, 1)], 0.8, xys=[None, xy])
    assert e.value.status == 1
    gpu_ctx.set_map(T)
    with pytest.raises(CLCError) as e:                      # positions for one side only
        gpu_ctx.match_map_ratio(Q, 0.8, None, xy)
    assert e.value.status == 1
    with pytest.raises(CLCError) as e:                      # pair naming a camera that does not exist
        gpu_ctx.match_ratio_pairs([T, Q], [(0, 2)], 0.8)
    assert e.value.status == 1
    big = np.zeros((20001, 64), np.uint8)                   # gpu_ctx: maxkp 20000
    with pytest.raises(CLCError) as e:
        gpu_ctx.match_ratio(big, T, 0.8)
    assert e.value.status == 2
    with pytest.raises(CLCError) as e:
        gpu_ctx.match_map_ratio(big, 0.8)
    assert e.value.status == 2
    from coloc_amd import Context
    fresh = Context(device=0, width=160, height=120, maxkp=100, detector=False)
    with pytest.raises(CLCError) as e:                      # before set_map
        fresh.match_map_ratio(Q, 0.8)
    assert e.value.status == 5
    fresh.close()

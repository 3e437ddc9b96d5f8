"""The matrix sweep's top-2 network (coloc_amd/csrc/k2nn_top2.h inside k2nn_sweep_mx_kernel) with the best and the second best train row in
every pair of positions: matches, best_out and second_out against a numpy brute force, exact, under both acceptance rules.

Train set: nt random rows of even weight (so that every pairwise distance D is even).  One query per ordered pair (i, j), i != j: row i
with D/2 - 1 of the bits in which it differs from row j flipped, so d(q, i) = D/2 - 1 and d(q, j) = D/2 + 1 (about 127 and 129) while
every other row stays about 256 away.  With nt = 32 the pair (i, j) runs over every pair of accumulator positions of a tile (register and
lane half); 31 / 33 / 63 / 64 / 65 / 97 rows add the partial last tile, the step back across tiles and the last tile's second chain, which
is folded in behind the loop."""
import functools

import numpy as np
import pytest

NTS = [32, 31, 33, 63, 64, 65, 97]
THRESHOLDS = [1, 2]            # second - best is 2 everywhere: accepted under 1, rejected under 2
RATIOS = [0.999, 0.8]          # best / second = 1 - 2 / second lies in 0.98 .. 0.99: accepted under 0.999^2, rejected under 0.64


@functools.lru_cache(maxsize=None)
def case(nt):
    """(Q, T, pairs, best distance, second distance) with the brute force held to the construction"""
    rng = np.random.default_rng(7000 + nt)
    Tb = rng.integers(0, 2, size=(nt, 512), dtype=np.uint8)
    Tb[:, 0] ^= (Tb.sum(axis=1) & 1).astype(np.uint8)                     # even weight -> even pairwise distances
    pairs = np.array([(i, j) for i in range(nt) for j in range(nt) if i != j])
    Qb = Tb[pairs[:, 0]].copy()
    for n, (i, j) in enumerate(pairs):
        differ = np.flatnonzero(Tb[i] != Tb[j])
        assert len(differ) % 2 == 0 and len(differ) >= 4
        Qb[n, rng.permutation(differ)[: len(differ) // 2 - 1]] ^= 1
    # brute force: every distance, the lowest index among equal ones
    qf, tf = Qb.astype(np.float32), Tb.astype(np.float32)
    dist = (qf @ (1.0 - tf).T + (1.0 - qf) @ tf.T).astype(np.int64)
    order = np.lexsort((np.broadcast_to(np.arange(nt), dist.shape), dist), axis=1)
    best_i, second_i = order[:, 0], order[:, 1]
    rows = np.arange(len(pairs))
    best_d, second_d = dist[rows, best_i], dist[rows, second_i]
    # the construction: best is row i, second is row j, two apart
    assert np.array_equal(best_i, pairs[:, 0]) and np.array_equal(second_i, pairs[:, 1])
    assert np.array_equal(second_d - best_d, np.full(len(pairs), 2)) and (np.sort(dist, axis=1)[:, 2] > second_d).all()
    Q, T = np.packbits(Qb, axis=1), np.packbits(Tb, axis=1)
    for a in (Q, T, pairs, best_d, second_d):
        a.setflags(write=False)
    return Q, T, pairs, best_d, second_d


def check(gpu_ctx, nt, sel):
    Q, T, pairs, best_d, second_d = case(nt)
    Q, want_i, bd, sd = Q[sel], pairs[sel, 0], best_d[sel], second_d[sel]
    gpu_ctx.set_k2nn_formulation("matrix")
    for thr in THRESHOLDS:
        m, b, s = gpu_ctx.match_2nn(Q, T, thr, want_dist=True)
        assert np.array_equal(m, np.where(sd - bd > thr, want_i, -1))
        assert np.array_equal(b, bd) and np.array_equal(s, sd)
    for ratio in RATIOS:
        m, b, s = gpu_ctx.match_ratio(Q, T, ratio, want_dist=True)
        r2 = np.float32(ratio) * np.float32(ratio)
        assert np.array_equal(m, np.where(bd.astype(np.float32) < r2 * sd.astype(np.float32), want_i, -1))
        assert np.array_equal(b, bd) and np.array_equal(s, sd)
    assert (m == -1).all()                                                 # (the last rule rejects, the one before accepts: both sides seen)


def test_construction_puts_best_and_second_in_every_pair_of_positions():
    """the 32-row case on the CPU: 992 queries, one per ordered pair of rows of the tile (asserted inside case())"""
    Q, T, pairs, best_d, second_d = case(32)
    assert len(Q) == 992 and len(set(map(tuple, pairs))) == 32 * 31
    assert best_d.min() >= 90 and second_d.max() <= 160


@pytest.mark.gpu
@pytest.mark.parametrize("nt", NTS)
def test_every_pair_of_rows(gpu_ctx, nt):
    check(gpu_ctx, nt, slice(None))


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [32, 97])
@pytest.mark.parametrize("nq", [1, 33, 257])
def test_clamped_query_rows_and_more_than_one_block(gpu_ctx, nt, nq):
    n = nt * (nt - 1)
    sel = np.random.default_rng(nq).permutation(n)[:nq]                    # nq of the pairs, anywhere in the tile(s)
    check(gpu_ctx, nt, sel)

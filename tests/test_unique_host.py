"""The one-to-one filter on the host (tests/unique_host.py): the properties the header states hold for the numpy statement, the g++ build
of coloc_amd/csrc/unique_math.h equals it on random and edge keys, and on three cameras with planted doubles the filtered pair lists give
the tracks builder (tests/map_host.py) strictly more tracks than the plain ones."""
import numpy as np

import map_host
import unique_host as uh


def _random_case(rng, nq, nt, kind):
    """match / best with random claims; kind 1 adds rows outside the train set and distances no producer writes"""
    match = rng.randint(-1, max(nt, 1), nq).astype(np.int32) if nt else np.full(nq, -1, dtype=np.int32)
    best = rng.randint(0, 513, nq).astype(np.uint16)
    if rng.rand() < 0.5:
        best = (best // 64).astype(np.uint16)                                 # many equal distances: ties
    if kind == 1 and nq:
        bad = rng.rand(nq) < 0.2
        match[bad] = rng.choice([nt, nt + 5, -2, -2 ** 31, 2 ** 31 - 1], bad.sum())
        far = rng.rand(nq) < 0.1
        best[far] = rng.choice([513, 1000, 65535], far.sum())
    return match, best


def _check_properties(match, best, nt):
    out, owner = uh.unique(match, best, nt)
    kept = np.nonzero(out >= 0)[0]
    claims = (match >= 0) & (match < nt) & (best <= 512)
    assert len(set(out[kept].tolist())) == len(kept)                          # one-to-one
    assert (owner[out[kept]] == kept).all()                                   # owner[match[q]] == q
    assert (out[kept] == match[kept]).all() and claims[kept].all()             # survivors are a subset of the claims
    assert set(out[kept].tolist()) == set(match[claims].tolist())             # exactly one survivor per claimed row
    assert (owner >= 0).sum() == len(kept) and (out[~claims] == -1).all()      # everything that is no claim is -1
    for t in set(match[claims].tolist()):                                     # the smallest distance, then the lowest query row
        qs = np.nonzero(claims & (match == t))[0]
        b = best[qs].min()
        assert owner[t] == qs[best[qs] == b].min()
    again, owner2 = uh.unique(out, best, nt)                                  # idempotent
    assert np.array_equal(again, out) and np.array_equal(owner2, owner)
    return out, owner


def test_the_statement_has_the_stated_properties():
    rng = np.random.RandomState(1)
    for nq in (0, 1, 2, 65, 300):
        for nt in (0, 1, 2, 64, 300):
            for kind in (0, 1):
                _check_properties(*_random_case(rng, nq, nt, kind), nt)


def test_ties_sanitising_and_edges():
    # equal distances on one row: the lowest query row; a smaller distance beats a lower row
    out, owner = uh.unique([3, 3, 3, 1, 1], [7, 7, 7, 9, 8], 5)
    assert out.tolist() == [3, -1, -1, -1, 1] and owner.tolist() == [-1, 4, -1, 0, -1]
    # distances 0 and 512 are claims, 513 and 65535 are not; rows nt, nt + 5, -2, INT32_MIN are no claims: all become -1
    nt = 4
    match = np.array([0, 0, 1, 2, nt, nt + 5, -2, -2 ** 31, 3, -1], dtype=np.int32)
    best = np.array([512, 0, 512, 513, 1, 1, 1, 1, 65535, 0], dtype=np.uint16)
    out, owner = _check_properties(match, best, nt)
    assert out.tolist() == [-1, 0, 1, -1, -1, -1, -1, -1, -1, -1] and owner.tolist() == [1, 2, -1, -1]
    # no queries: every owner -1; no train rows: every entry -1
    out, owner = uh.unique(np.zeros(0, np.int32), np.zeros(0, np.uint16), 3)
    assert len(out) == 0 and owner.tolist() == [-1, -1, -1]
    out, owner = uh.unique([0, 1, -1], [1, 2, 3], 0)
    assert out.tolist() == [-1, -1, -1] and len(owner) == 0


def test_unique_math_equals_the_statement():
    rng = np.random.RandomState(2)
    lib = uh.lib()
    assert (lib.unique_host_shift(), lib.unique_host_max_rows()) == (uh.SHIFT, uh.MAX_ROWS) and lib.unique_host_free_word() & 0xFFFFFFFF == 0xFFFFFFFF
    # keys: distance 0 and 512, row 0 and 2^22 - 1, and random ones
    best = np.concatenate([[0, 0, 512, 512, 1, 511], rng.randint(0, 513, 5000)]).astype(np.uint32)
    q = np.concatenate([[0, uh.MAX_ROWS - 1, 0, uh.MAX_ROWS - 1, 1, uh.MAX_ROWS - 2], rng.randint(0, uh.MAX_ROWS, 5000)]).astype(np.uint32)
    k, h = uh.cxx_keys(best, q)
    assert np.array_equal(k.astype(np.uint64), uh.key(best, q)) and np.array_equal(h, q.astype(np.int32))
    assert int(k.max()) == (512 << 22) + uh.MAX_ROWS - 1 < 0xFFFFFFFF        # the armed word is no key
    order = np.lexsort((q, best))                                             # the key's order is (distance, row)'s
    assert (np.diff(k[order].astype(np.int64)) >= 0).all()
    # the claim test and the whole filter, random and edge inputs
    for nq in (0, 1, 65, 300, 1000):
        for nt in (0, 1, 2, 65, 300):
            for kind in (0, 1):
                match, bst = _random_case(rng, nq, nt, kind)
                assert np.array_equal(uh.cxx_claims(match, bst, nt), (match >= 0) & (match < nt) & (bst <= 512))
                want = uh.unique(match, bst, nt)
                got = uh.cxx_unique(match, bst, nt)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (nq, nt, kind)


def test_filtered_pair_lists_give_more_tracks(oracle):
    """three cameras, threshold 40, A with `dup` second near-copies: every doubled train row costs the plain lists a whole track"""
    n, dup, thr = 300, 40, 40
    cams = uh.three_cameras(n, dup, 7)
    rows = [len(c) for c in cams]
    plain, filtered = [], []
    for a, b in uh.PAIRS:
        m, best, _ = oracle.k2nn(cams[a], cams[b], thr, want_dist=True)
        plain.append(m.copy())
        filtered.append(uh.unique(m, best, rows[b])[0])
    assert sum(len(uh.doubled_rows(m)) for m in plain) >= dup                 # the plain matches hold the planted doubles
    for m in filtered:
        assert len(uh.doubled_rows(m)) == 0                                   # every pair list after the filter is one-to-one
    t_plain = map_host.build_tracks(rows, uh.pair_lists(plain))
    t_unique = map_host.build_tracks(rows, uh.pair_lists(filtered))
    print("n %d dup %d: matches kept %d -> %d, tracks %d -> %d" % (n, dup, sum((m >= 0).sum() for m in plain), sum((m >= 0).sum() for m in filtered),
                                                                  len(t_plain), len(t_unique)))
    assert len(t_unique) > len(t_plain)

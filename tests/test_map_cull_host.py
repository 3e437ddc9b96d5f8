"""coloc_amd/csrc/cull_math.h in its g++ build (tests/host/map_cull_lib.cpp) against the Python statement (tests/map_cull_host.py): the
rule on random counters and on its edges, the rectangle test on its borders and NaN, the remap, and the invariants the statement keeps."""
import numpy as np

import map_cull_host as ch
import proj_host as ph

TOP = 0xFFFFFFFF


def _py_rule(visible, found, last_view, epoch, flagged, rule):
    cl = [ch.clause(int(v), int(f), int(l), epoch, bool(flagged[i]) if flagged is not None else False, rule["min_visible"], rule["num"],
                    rule["den"], rule["max_idle"]) for i, (v, f, l) in enumerate(zip(visible, found, last_view))]
    return np.array(cl, dtype=np.uint8)


def _same_rule(visible, found, last_view, epoch, flagged, rule):
    want = _py_rule(visible, found, last_view, epoch, flagged, rule)
    clause, drops = ch.cxx_rule(visible, found, last_view, epoch, flagged, **rule)
    assert np.array_equal(clause, want), (visible, found, last_view, epoch, rule)
    assert np.array_equal(drops, want != ch.KEPT)
    return want


def test_rule_on_random_counters():
    rng = np.random.RandomState(3)
    seen = np.zeros(4, dtype=np.int64)
    for trial in range(40):
        n = 257
        big = trial % 4 == 3                                                   # counters all over the 32-bit range
        visible = rng.randint(0, 2 ** 32 if big else 40, n, dtype=np.uint64).astype(np.uint32)
        found = (visible * rng.uniform(0.0, 1.0, n)).astype(np.uint32)
        epoch = int(rng.randint(0, 2 ** 32, dtype=np.uint64)) if big else int(rng.randint(0, 100))
        last_view = ((epoch - rng.randint(0, 30, n)) & TOP).astype(np.uint32)
        flagged = (rng.uniform(size=n) < 0.1).astype(np.uint8) if trial % 2 else None
        rule = dict(min_visible=int(rng.randint(1, 12)), num=int(rng.randint(0, 5)), den=int(rng.randint(1, 9)), max_idle=int(rng.randint(0, 20)))
        want = _same_rule(visible, found, last_view, epoch, flagged, rule)
        assert (found <= visible).all()
        seen += np.bincount(want, minlength=4)
    assert (seen >= 100).all(), seen                                           # every clause, and kept rows, well represented


def test_rule_edges():
    rule = dict(min_visible=8, num=1, den=4, max_idle=0)
    assert rule == ch.DEFAULT_RULE == ch.cxx_default_rule()
    # visible == min_visible - 1 is young, visible == min_visible is judged
    assert list(_same_rule([7, 8], [0, 0], [0, 0], 5, None, rule)) == [ch.KEPT, ch.RATIO]
    # found * den == num * visible exactly: kept; one less: dropped
    assert list(_same_rule([8, 8, 12, 12], [2, 1, 3, 2], [0] * 4, 5, None, rule)) == [ch.KEPT, ch.RATIO, ch.KEPT, ch.RATIO]
    # counters near 2^32 - 1: the 32-bit products wrap (3 * (2^32 - 1) mod 2^32 = 2^32 - 3 < 2 * (2^32 - 2) mod 2^32 = 2^32 - 4 is false, the
    # 64-bit products say 3 (2^32 - 2) >= 2 (2^32 - 1): kept; and a case the wrapped products would keep
    r3 = dict(min_visible=1, num=2, den=3, max_idle=0)
    assert list(_same_rule([TOP, TOP, TOP], [TOP - 1, TOP, 0x55555555 * 2 - 1], [0] * 3, 0, None, r3)) == [ch.KEPT, ch.KEPT, ch.RATIO]
    wrap = dict(min_visible=1, num=1, den=0x10000, max_idle=0)
    assert ((0x10000 * 0x10000) & TOP) == 0                                   # found * den wraps to 0 in 32 bits
    assert list(_same_rule([0x10001], [0x10000], [0], 0, None, wrap)) == [ch.KEPT]
    # the idle clause: the epoch wraps, the difference does not; max_idle == 0 switches it off
    idle = dict(min_visible=8, num=1, den=4, max_idle=3)
    assert list(_same_rule([0] * 4, [0] * 4, [TOP, TOP - 1, 2, 1], 2, None, idle)) == [ch.KEPT, ch.IDLE, ch.KEPT, ch.KEPT]      # idle 3, 4, 0, 1
    assert list(_same_rule([0, 0], [0, 0], [5, 1], 5, None, idle)) == [ch.KEPT, ch.IDLE]
    assert list(_same_rule([0, 0], [0, 0], [5, 1], 5, None, rule)) == [ch.KEPT, ch.KEPT]
    # a flagged young row goes, and flagged is the first clause
    assert list(_same_rule([0, 8], [0, 0], [0, 0], 0, [1, 1], rule)) == [ch.FLAGGED, ch.FLAGGED]
    assert list(_same_rule([0, 8], [0, 0], [0, 0], 0, [0, 0], rule)) == [ch.KEPT, ch.RATIO]
    # ratio before idle
    assert list(_same_rule([8], [0], [0], 9, None, idle)) == [ch.RATIO]


def test_in_view_borders_and_nan():
    lo, hi_x, hi_y = ch.bounds(640, 480, 4.0)
    assert (lo, hi_x, hi_y) == (np.float32(4.0), np.float32(635.0), np.float32(475.0))
    assert np.array_equal(ch.cxx_bounds(640, 480, 4.0), np.array([lo, hi_x, hi_y], dtype=np.float32))
    below, above = np.nextafter(np.float32(4.0), np.float32(0.0)), np.nextafter(np.float32(635.0), np.float32(1000.0))
    nan = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
    uv = np.array([[lo, 100.0], [below, 100.0], [hi_x, 100.0], [above, 100.0], [100.0, lo], [100.0, below], [100.0, hi_y],
                   [100.0, np.nextafter(hi_y, np.float32(1000.0))], [nan, nan], [nan, 100.0], [100.0, nan], [np.inf, 100.0], [100.0, 100.0]], dtype=np.float32)
    want = np.array([1, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 1], dtype=bool)
    assert np.array_equal(ch.in_view(uv, lo, hi_x, hi_y), want)
    assert np.array_equal(ch.cxx_in_view(uv, lo, hi_x, hi_y), want)
    rng = np.random.RandomState(5)
    uv = rng.uniform(-50, 700, (2000, 2)).astype(np.float32)
    assert np.array_equal(ch.cxx_in_view(uv, lo, hi_x, hi_y), ch.in_view(uv, lo, hi_x, hi_y))
    # a landmark without a projection (behind the camera) is never in view
    xy, ok = ph.project(np.eye(3, 4), (512.0, 320.0, 240.0), np.array([[0.0, 0.0, -5.0], [0.0, 0.0, 5.0]]))
    assert list(ok) == [False, True] and list(ch.cxx_in_view(xy, lo, hi_x, hi_y)) == [False, True]


def test_remap_and_lists():
    rng = np.random.RandomState(9)
    for n in (0, 1, 63, 64, 65, 1025):
        for p in (0.0, 1.0, 0.3):
            drops = rng.uniform(size=n) < p
            want, kept = ch.remap(drops)
            got, got_kept = ch.cxx_remap(drops)
            assert np.array_equal(got, want) and got_kept == kept
            assert kept + int(drops.sum()) == n
            k = want[want >= 0]
            assert np.array_equal(k, np.arange(kept))                          # strictly ascending over the kept rows, no gap
            assert ch.cxx_remap_valid(want) == kept
            lst = np.concatenate([rng.randint(-3, n + 3, 50), [-1, n, n - 1, -2 ** 31]]).astype(np.int32)
            assert np.array_equal(ch.cxx_remap_list(lst, n, want), ch.remap_list(lst, n, want))
    assert ch.cxx_remap_valid(np.array([0, 2, -1], dtype=np.int32)) == -1
    assert ch.cxx_remap_valid(np.array([1, 0], dtype=np.int32)) == -1
    assert ch.cxx_remap_valid(np.array([-2, 0], dtype=np.int32)) == -1
    assert ch.cxx_remap_valid(np.array([-1, 0, -1, 1], dtype=np.int32)) == 2


def test_statement_invariants():
    """a run of observes, extensions (cover) and culls: found <= visible, counts add up, the state follows the rows"""
    rng = np.random.RandomState(11)
    cam = (512.0, 320.0, 240.0, 0.0, 0.0, 0.0)
    n = 120
    X = np.column_stack([rng.uniform(-6, 6, n), rng.uniform(-4, 4, n), rng.uniform(4, 12, n)])
    X[::9, 2] *= -1.0                                                          # behind the camera
    M = rng.randint(0, 256, (n, 64)).astype(np.uint8)
    st = ch.Stats()
    proj = ph.project(np.eye(3, 4), cam, X)[0]
    for frame in range(10):
        rows = rng.choice(n, 60, replace=False)
        feat = np.where(np.isnan(proj[rows]), 0.0, proj[rows]).astype(np.float32)
        feat[::3] += 9.0                                                       # outside the gate
        view = dict(cam=cam, Rt=np.eye(3, 4), feat=feat, track=rows.astype(np.int32), count=None, width=640, height=480, gate=2.0, margin=0.0)
        counts = ch.observe(st, X, [view])
        assert st.epoch == frame + 1 and counts[0][1] <= counts[0][0]
        assert all(f <= v for f, v in zip(st.found, st.visible))
        if frame == 5:                                                         # rows appended between two observes
            X = np.vstack([X, X[:7] + 0.01])
            M = np.vstack([M, M[:7]])
            st.cover(len(X))
            assert st.visible[-7:] == [0] * 7 and st.last_view[-7:] == [6] * 7
            n = len(X)
            proj = ph.project(np.eye(3, 4), cam, X)[0]
    res =ch.cull(st, M, X, dict(min_visible=4, num=1, den=2, max_idle=6))
    assert res["n_kept"] + res["n_dropped"] == n and res["n_dropped"] == res["n_flagged"] + res["n_ratio"] + res["n_idle"]
    assert res["n_ratio"] > 0 and res["n_idle"] > 0 and res["n_kept"] > 0
    assert st.rows == res["n_kept"] == len(st.visible) == len(res["M"]) == len(res["X"])
    kept = np.nonzero(res["remap"] >= 0)[0]
    assert np.array_equal(res["remap"][kept], np.arange(len(kept))) and np.array_equal(res["X"], X[kept])

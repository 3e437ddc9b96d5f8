"""The statement of the map match guided by a predicted pose on the host (tests/proj_host.py over the g++ build of
coloc_amd/csrc/proj_math.h): the projection and the gate on exactly representable cases, the planted classes, and the invariant that ties
the result to plain K2NN.  The device entries are held to this statement bit for bit in tests/test_gpu_map_guided.py."""
import numpy as np

import guided_host as gh
import proj_host as ph


def test_exact_projections_and_landmarks_without_one():
    """gh.CAM_EXACT under the identity pose: half-integer pixels at power-of-two depths project exactly; z <= 0, a NaN and an overflow
    have no projection"""
    pix = np.array([[100.5, 50.0], [320.0, 240.0], [0.5, 479.5], [639.5, 0.5]])
    X = np.array([ph.landmark(x, y, z) for (x, y), z in zip(pix, (1.0, 4.0, 16.0, 0.5))])
    xy, ok = ph.project(ph.IDENTITY, gh.CAM_EXACT, X)
    assert ok.all() and xy.tolist() == pix.tolist()
    bad = np.array([ph.landmark(100.5, 50.0, -2.0), [0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [np.nan, 0.0, 1.0], [1e300, 0.0, 1.0], [0.0, 0.0, np.inf]])
    xy, ok = ph.project(ph.IDENTITY, gh.CAM_EXACT, bad)
    assert not ok.any() and (xy.view(np.uint32) == gh.NONE_BITS).all()
    for q in ([100.5, 50.0], [0.0, 0.0]):
        assert not ph.gate(q, xy, np.float32(1e30)).any()
    # a translation along the axis brings the point behind the camera into view, and moves the one in front out of it
    Rt = ph.IDENTITY.copy()
    Rt[2, 3] = 4.0
    xy, ok = ph.project(Rt, gh.CAM_EXACT, np.array([[0.0, 0.0, -2.0], [0.0, 0.0, -4.0], [0.0, 0.0, -8.0]]))
    assert ok.tolist() == [True, False, False] and xy[0].tolist() == [320.0, 240.0]


def test_the_3_4_5_edge():
    """dx = 3, dy = 4, radius = 5: d2 = fma(3, 3, 16) = 25 = r2 is INSIDE; dy = 4.5 is outside; a NaN on either side is outside"""
    q = np.array([100.5, 200.0], dtype=np.float32)
    xy = np.array([[103.5, 204.0], [97.5, 196.0], [103.5, 204.5], [100.5, 205.0], [100.5, 205.5], [105.5, 200.0], [106.0, 200.0]], dtype=np.float32)
    r2 = ph.r2_of(5.0)
    assert r2 == np.float32(25.0)
    assert ph.gate(q, xy, r2).tolist() == [True, True, False, True, False, True, False]
    none = np.array([gh.NONE_BITS] * 2, dtype=np.uint32).view(np.float32)
    assert not ph.gate(none, xy, r2).any() and not ph.gate(q, np.array([none, [none[0], 200.0]]), r2).any()
    # through the statement, with the projections of landmarks
    X = np.array([ph.landmark(x, y, 2.0) for x, y in xy])
    Qd = np.zeros((1, 64), dtype=np.uint8)
    st = ph.statement(Qd, np.zeros((len(X), 64), dtype=np.uint8), X, ph.IDENTITY, 5.0, 0, gh.CAM_EXACT, feat=q.reshape(1, 2))
    assert gh.same_bits(st["proj"], xy) and gh.same_bits(st["qpos"], q.reshape(1, 2))
    assert st["cand"][0].tolist() == [True, True, False, True, False, True, False]


def test_sentinels_and_the_lone_candidate():
    """one candidate: second = 100000, accepted whatever the distance; none: best = 100000 -> -1; a tie inside the radius: rejected"""
    M = np.zeros((4, 64), dtype=np.uint8)
    M[1] = 0xFF                                                              # distance 512 from a zero query
    Q = np.zeros((3, 64), dtype=np.uint8)
    X = np.array([ph.landmark(10.0, 100.0, 1.0), ph.landmark(10.0, 200.0, 2.0), ph.landmark(10.5, 100.5, 4.0), ph.landmark(10.0, 300.0, 8.0)])
    qpos = np.array([[11.0, 200.0], [11.0, 400.0], [10.0, 100.0]], dtype=np.float32)
    st = ph.statement(Q, M, X, ph.IDENTITY, 2.0, 40, gh.CAM_EXACT, feat=qpos)
    assert st["cand"].sum(1).tolist() == [1, 0, 2]
    assert st["match"].tolist() == [1, -1, -1]
    assert st["best_raw"].tolist() == [512, 100000, 0] and st["second_raw"].tolist() == [100000, 200000, 0]
    assert st["best"].tolist() == [512, 65535, 0] and st["second"].tolist() == [65535, 65535, 0]
    # rows at or past a count hold NaNs and are answered -1
    st = ph.statement(Q, M, X, ph.IDENTITY, 2.0, 40, gh.CAM_EXACT, feat=qpos, count=1)
    assert st["match"].tolist() == [1, -1, -1] and (st["qpos"][1:].view(np.uint32) == gh.NONE_BITS).all() and not st["cand"][1:].any()


def test_every_class_occurs():
    for nq in (127, 128, 129, 300):
        for nm in (33, 513, 1500):
            Q, M, qpos, X = ph.make_case(nq, nm, 1000 * nq + nm)
            assert np.array_equal(gh.ud_positions(gh.CAM_EXACT, feat=qpos), qpos.astype(np.float64))
            st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
            c = ph.classes(st, Q, M, 20)
            assert ph.all_classes_occur(c), (nq, nm, c)
            # every projection that exists is a half-integer pixel: the projection was exact
            ok = ~(st["proj"].view(np.uint32) == gh.NONE_BITS).all(1)
            assert np.array_equal(st["proj"][ok] * 2, np.round(st["proj"][ok] * 2)) and (~ok).sum() == c["copy_behind"] > 0


def test_the_invariant_on_random_inputs():
    """for every query whose plain K2NN match lies inside the radius, the guided match is that same row; with a radius larger than the
    image diagonal and every landmark in front the statement is plain K2NN's over all queries"""
    for seed, nq, nm in ((1, 150, 400), (2, 64, 33), (3, 200, 900)):
        Q, M, qpos, X = ph.make_case(nq, nm, seed, behind=False)
        assert (X[:, 2] > 0).all()
        pm, pb, ps = gh.plain(Q, M, 20)
        st = ph.statement(Q, M, X, ph.IDENTITY, 3.0, 20, gh.CAM_EXACT, feat=qpos)
        inside = np.array([pm[q] >= 0 and st["cand"][q, pm[q]] for q in range(nq)])
        assert inside.sum() > 5
        assert np.array_equal(st["match"][inside], pm[inside])
        wide = ph.statement(Q, M, X, ph.IDENTITY, 2000.0, 20, gh.CAM_EXACT, feat=qpos)
        assert wide["cand"].all()
        assert np.array_equal(wide["match"], pm) and np.array_equal(wide["best_raw"], pb) and np.array_equal(wide["second_raw"], ps)
        if nm >= 400:
            assert (st["match"] != pm).any()                                 # the gate recovers (or drops) something

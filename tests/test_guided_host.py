"""The guided match's statement on the host (tests/guided_host.py over the g++ build of coloc_amd/csrc/guided_math.h): the gate on
exactly representable cases, degenerate lines, and the invariant that ties the guided result to plain K2NN.  The device entries are
held to this statement bit for bit in tests/test_gpu_guided_match.py."""
import numpy as np

import guided_host as gh


def test_gate_on_exactly_representable_cases():
    """F = [[0,0,0],[0,0,-1],[0,1,0]]: the line of (u, v) is (0, -1, v) and n = 1, so e = v_a - y_b with no rounding anywhere.
    band = 2.0: |e| == 2.0 is a candidate, 2.5 is not."""
    uv = np.array([[100.5, 50.5], [7.0, 300.0]])
    L, ok = gh.lines(gh.F_ROWS, uv)
    assert ok.all()
    assert L.tolist() == [[0.0, -1.0, 50.5], [0.0, -1.0, 300.0]]
    xy = np.array([[3.0, 50.5], [600.0, 52.5], [9.5, 48.5], [1.0, 53.0], [1.0, 48.0], [300.0, 52.0]], dtype=np.float32)
    assert gh.gate(L[0], xy, 2.0).tolist() == [True, True, True, False, False, True]
    assert gh.gate(L[1], np.array([[0.0, 302.0], [0.0, 302.5], [0.0, 297.5], [0.0, 298.0]], dtype=np.float32), 2.0).tolist() == [True, False, False, True]


def test_positions_of_the_exact_camera_come_through_unchanged():
    feat = np.array([[0.5, 0.5], [320.0, 240.0], [639.5, 479.5], [100.5, 50.0]], dtype=np.float32)
    assert np.array_equal(gh.ud_positions(gh.CAM_EXACT, feat=feat), feat.astype(np.float64))


def test_degenerate_lines_have_no_candidates():
    uv = np.array([[10.0, 20.0], [300.0, 200.0]])
    xy = np.array([[10.0, 20.0], [0.0, 0.0], [300.0, 200.0]], dtype=np.float32)
    Fnan = gh.F_ROWS.copy()
    Fnan[1, 2] = np.nan
    Finf = gh.F_ROWS.copy()
    Finf[1, 2], Finf[2, 1] = -np.inf, np.inf                                 # n is not finite
    for F in (np.zeros((3, 3)), Fnan, Finf):
        L, ok = gh.lines(F, uv)
        assert not ok.any()
        assert (L.view(np.uint32) == gh.NONE_BITS).all()
        for q in range(2):
            assert not gh.gate(L[q], xy, 1e30).any()
    # a line whose normal vanishes for ONE query only: F x = (0, 0, .) at the epipole
    F = np.array([[0.0, -1.0, 20.0], [1.0, 0.0, -10.0], [-20.0, 10.0, 0.0]])       # [e]_x with e = (10, 20, 1)
    L, ok = gh.lines(F, uv)
    assert ok.tolist() == [False, True]
    Q = np.zeros((2, 64), dtype=np.uint8)
    T = np.zeros((3, 64), dtype=np.uint8)
    st = gh.statement(Q, T, F, 5.0, 0, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=uv.astype(np.float32), feat_b=xy)
    assert st["cand"][0].sum() == 0 and st["match"][0] == -1 and st["best"][0] == 65535 and st["second"][0] == 65535


def test_sentinels_and_the_lone_candidate():
    """one candidate: second = 100000, accepted whatever the distance; none: best = 100000 -> -1; a tie inside the band: rejected"""
    T = np.zeros((4, 64), dtype=np.uint8)
    T[1] = 0xFF                                                              # distance 512 from a zero query
    Q = np.zeros((3, 64), dtype=np.uint8)
    tpos = np.array([[10.0, 100.0], [10.0, 200.0], [50.0, 100.5], [10.0, 300.0]], dtype=np.float32)
    qpos = np.array([[5.0, 200.0], [5.0, 400.0], [5.0, 100.0]], dtype=np.float32)
    st = gh.statement(Q, T, gh.F_ROWS, 2.0, 40, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
    assert st["cand"].sum(1).tolist() == [1, 0, 2]
    assert st["match"].tolist() == [1, -1, -1]
    assert st["best_raw"].tolist() == [512, 100000, 0] and st["second_raw"].tolist() == [100000, 200000, 0]
    assert st["best"].tolist() == [512, 65535, 0] and st["second"].tolist() == [65535, 65535, 0]


def test_the_invariant_on_random_inputs():
    """for every query whose plain K2NN match lies in the band, the guided match is that same row; with a band wider than the image
    diagonal the guided result is plain K2NN's over all queries"""
    for seed, nq, nt in ((1, 150, 400), (2, 64, 33), (3, 200, 900)):
        Q, T, qpos, tpos = gh.make_case(nq, nt, seed)
        pm, pb, ps = gh.plain(Q, T, 20)
        st = gh.statement(Q, T, gh.F_ROWS, 3.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
        inband = np.array([pm[q] >= 0 and st["cand"][q, pm[q]] for q in range(nq)])
        assert inband.sum() > 5
        assert np.array_equal(st["match"][inband], pm[inband])
        wide = gh.statement(Q, T, gh.F_ROWS, 2000.0, 20, gh.CAM_EXACT, gh.CAM_EXACT, feat_a=qpos, feat_b=tpos)
        assert wide["cand"].all()
        assert np.array_equal(wide["match"], pm) and np.array_equal(wide["best_raw"], pb) and np.array_equal(wide["second_raw"], ps)
        if nt >= 400:
            c = gh.classes(st, Q, T, 20)
            assert min(c["none"], c["one"], c["many"], c["best_outside"], c["tie"]) > 0 and c["tie_rejected"], c
            assert (st["match"] != pm).any()                                 # the guide recovers (or drops) something

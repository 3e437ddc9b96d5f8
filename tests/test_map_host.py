"""The yardsticks of the device map build without a GPU: tests/map_host.py (the Python statement of the tracks) against a brute-force
component search, and the host build of coloc_amd/csrc/map_math.h (tests/host/map_math_lib.cpp) -- the arithmetic the device is held to
bit for bit -- against numpy's SVD, the acceptance rule and the pose composition."""
import itertools

import numpy as np

import map_host

DLT_MEASURED = 5.98e-12     # measured: see test_host_dlt_against_the_svd_null_vector


def _brute_tracks(rows, edges):
    """components by repeated flooding over an adjacency matrix of ALL nodes; edges = [((cam, row), (cam, row)), ...]"""
    first = np.concatenate([[0], np.cumsum(rows)])
    n = int(first[-1])
    adj = np.zeros((n, n), dtype=bool)
    used = np.zeros(n, dtype=bool)
    for (ca, ra), (cb, rb) in edges:
        if not (0 <= ra < rows[ca] and 0 <= rb < rows[cb]):
            continue
        u, v = first[ca] + ra, first[cb] + rb
        adj[u, v] = adj[v, u] = True
        used[u] = used[v] = True
    seen = np.zeros(n, dtype=bool)
    out = []
    for s in range(n):                                      # ascending smallest node = ascending (camera, row)
        if seen[s] or not used[s]:
            continue
        comp = np.zeros(n, dtype=bool)
        comp[s] = True
        while True:
            grown = comp | adj[comp].any(0)
            if (grown == comp).all():
                break
            comp = grown
        seen |= comp
        nodes = np.nonzero(comp)[0]
        cams = np.searchsorted(first, nodes, side="right") - 1
        if len(nodes) >= 2 and len(set(cams.tolist())) == len(nodes):
            row = np.full(len(rows), -1, dtype=np.int32)
            row[cams] = nodes - first[cams]
            out.append(row)
    return np.array(out, dtype=np.int32).reshape(-1, len(rows))


def _pairs_of(edges):
    by = {}
    for (ca, ra), (cb, rb) in edges:
        by.setdefault((ca, cb), []).append((ra, rb))
    return [dict(cam_a=a, cam_b=b, q=[e[0] for e in es], t=[e[1] for e in es]) for (a, b), es in by.items()]


HAND = {
    "chain through three cameras": ([4, 4, 4], [((0, 1), (1, 2)), ((1, 2), (2, 3))]),
    "direct conflict: two queries name one train": ([4, 4, 4], [((0, 0), (1, 1)), ((0, 2), (1, 1)), ((0, 3), (1, 3))]),
    "transitive conflict A5-B7, B7-C2, C2-A9": ([10, 10, 10], [((0, 5), (1, 7)), ((1, 7), (2, 2)), ((0, 9), (2, 2)), ((0, 1), (1, 1))]),
    "duplicates and an out-of-range row": ([3, 3], [((0, 0), (1, 0)), ((0, 0), (1, 0)), ((0, 2), (1, 5)), ((0, 1), (1, 2))]),
    "id order follows the smallest node, not the edge order": ([5, 5, 5], [((1, 4), (2, 4)), ((0, 3), (2, 0)), ((0, 0), (1, 1))]),
    "nothing": ([3, 3], []),
}


def test_statement_against_brute_force_on_hand_built_cases():
    for name, (rows, edges) in HAND.items():
        got = map_host.build_tracks(rows, _pairs_of(edges))
        want = _brute_tracks(rows, edges)
        assert got.shape == want.shape and np.array_equal(got, want), (name, got, want)
    t = map_host.build_tracks(*[HAND["transitive conflict A5-B7, B7-C2, C2-A9"][0], _pairs_of(HAND["transitive conflict A5-B7, B7-C2, C2-A9"][1])])
    assert t.tolist() == [[1, 1, -1]]
    t = map_host.build_tracks([5, 5, 5], _pairs_of(HAND["id order follows the smallest node, not the edge order"][1]))
    assert t.tolist() == [[0, 1, -1], [3, -1, 0], [-1, 4, 4]]


def test_statement_against_brute_force_on_random_graphs():
    rng = np.random.default_rng(5)
    for trial in range(40):
        n_cams = int(rng.integers(2, 6))
        rows = [int(v) for v in rng.integers(1, 9, n_cams)]
        edges = []
        for a, b in itertools.combinations(range(n_cams), 2):
            for _ in range(int(rng.integers(0, 7))):
                edges.append(((a, int(rng.integers(0, rows[a] + 1))), (b, int(rng.integers(0, rows[b] + 1)))))
        order = rng.permutation(len(edges))
        edges = [edges[i] for i in order]
        got = map_host.build_tracks(rows, _pairs_of(edges))
        want = _brute_tracks(rows, edges)
        assert got.shape == want.shape and np.array_equal(got, want), (trial, rows, edges)


def test_edges_of_a_pair_count_and_index():
    p = dict(cam_a=0, cam_b=1, q=[0, 1, 2, 3], t=[3, 2, 1, 0])
    assert [a.tolist() for a in map_host.pair_edges(dict(p, count=2))] == [[0, 1], [3, 2]]
    assert [a.tolist() for a in map_host.pair_edges(dict(p, index=[3, -1, 0, 9]))] == [[3, 0], [0, 3]]


CAM = (1000.0, 640.0, 360.0)


def _rot(rng, deg):
    w = rng.normal(size=3)
    w *= np.deg2rad(deg) * rng.uniform(0.2, 1.0) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def dlt_scenes():
    """two-view scenes for the DLT: baselines 0.05 .. 2, depths 5 .. 80 (so some points are near-degenerate: a 0.05 baseline seen from
    80 away), noise-free and with 0.5 px noise.  -> [(P1, P2, x1, x2, X_true)]"""
    rng = np.random.default_rng(11)
    out = []
    for baseline in (0.05, 0.1, 0.25, 0.5, 1.0, 2.0):
        for noise in (0.0, 0.5):
            R = _rot(rng, 8.0)
            C = rng.normal(size=3)
            C[2] *= 0.2
            C *= baseline / np.linalg.norm(C)
            Rt1 = np.hstack([np.eye(3), np.zeros((3, 1))])
            Rt2 = np.hstack([R, (-R @ C)[:, None]])
            P1, P2 = map_host.projection(CAM, Rt1), map_host.projection(CAM, Rt2)
            n = 300
            Z = rng.uniform(5.0, 80.0, n)
            X = np.stack([rng.uniform(-0.5, 0.5, n) * Z, rng.uniform(-0.3, 0.3, n) * Z, Z], 1)
            x = []
            for P in (P1, P2):
                h = np.hstack([X, np.ones((n, 1))]) @ P.T
                x.append(h[:, :2] / h[:, 2:] + noise * rng.normal(size=(n, 2)))
            out.append((P1, P2, x[0], x[1], X))
    return out


def dlt_deviation():
    """the largest |X_host - X_svd| / |X_svd| over dlt_scenes(), X_svd = hnormalized(numpy.linalg.svd's null vector of the SAME design
    matrix)"""
    worst = 0.0
    for P1, P2, x1, x2, _ in dlt_scenes():
        X, ok = map_host.triangulate(P1, P2, x1, x2)
        assert ok.all()
        for i in range(len(x1)):
            D = map_host.design(P1, x1[i], P2, x2[i])
            v = np.linalg.svd(D)[2][3]
            Xs = v[:3] / v[3]
            worst = max(worst, float(np.linalg.norm(X[i] - Xs) / np.linalg.norm(Xs)))
    return worst


def test_host_dlt_against_the_svd_null_vector():
    """MEASURED on the build machine (x86-64, numpy's bundled LAPACK): the largest relative deviation of the host DLT from the SVD null
    vector over dlt_scenes() is 5.98e-12 = DLT_MEASURED (DESIGN.md records the same figure).  Asserted: 4 x that value -- the margin is for LAPACK
    builds that differ between machines; the statement itself is deterministic.  Both sides factor the same 4 x 4 matrix and both
    are backward stable, so the deviation is of the order eps x its condition (largest over third singular value), which grows as the
    baseline shrinks against the depth."""
    worst = dlt_deviation()
    print("host DLT against the SVD null vector: largest relative deviation %.3e (bound %.3e)" % (worst, 4 * DLT_MEASURED))
    assert worst <= 4 * DLT_MEASURED


def test_noise_free_points_come_back():
    for P1, P2, x1, x2, X in dlt_scenes()[::2]:
        got, ok = map_host.triangulate(P1, P2, x1, x2)
        assert ok.all() and np.abs(got - X).max() < 1e-5 * 80


def test_design_matrix_is_the_one_stated():
    rng = np.random.default_rng(2)
    P1, P2 = rng.normal(size=(3, 4)), rng.normal(size=(3, 4))
    x1, x2 = rng.normal(size=2), rng.normal(size=2)
    want = np.stack([x1[0] * P1[2] - P1[0], x1[1] * P1[2] - P1[1], x2[0] * P2[2] - P2[0], x2[1] * P2[2] - P2[1]])
    assert np.array_equal(map_host.design(P1, x1, P2, x2), want)


def test_acceptance_rule_as_written():
    """dropped iff behind BOTH cameras, or |X[2]| > 100 (Reconstructor.hpp:227-231)"""
    I = np.hstack([np.eye(3), np.zeros((3, 1))])
    flip = np.hstack([np.diag([-1.0, 1.0, -1.0]), np.array([[0.0], [0.0], [1.0]])])       # looks down -z from z = 1
    assert map_host.accepted(I, I, [0, 0, 5.0])
    assert not map_host.accepted(I, I, [0, 0, -5.0])                 # behind both
    assert map_host.accepted(I, flip, [0, 0, -5.0])                  # behind the first only: kept
    assert map_host.accepted(I, flip, [0, 0, 5.0])                   # behind the second only: kept
    assert map_host.accepted(I, I, [0, 0, 100.0]) and not map_host.accepted(I, I, [0, 0, np.nextafter(100.0, 200.0)])
    assert map_host.accepted(I, flip, [0, 0, -100.0]) and not map_host.accepted(I, flip, [0, 0, -100.5])
    assert map_host.accepted(I, I, [0, 0, 0.0])                      # depth 0 is not < 0


def test_seed_poses_and_the_python_binding_agree():
    from coloc_amd import abi
    rng = np.random.default_rng(3)
    for _ in range(10):
        Ro, Rrel = _rot(rng, 40.0), _rot(rng, 20.0)
        Co, Crel, scale = rng.normal(size=3), rng.normal(size=3), float(rng.uniform(0.2, 3.0))
        a, b = map_host.seed_poses(Ro, Co, Rrel, Crel, scale)
        pa, pb = abi.seed_poses(Ro, Co, Rrel, Crel, scale)
        assert np.array_equal(a.view(np.uint64), pa.view(np.uint64)) and np.array_equal(b.view(np.uint64), pb.view(np.uint64))
        # relativePoseToAbsolute as written: R = R_rel R_origin, C = C_origin + scale C_rel, t = -R C
        assert np.allclose(a, np.hstack([Ro, (-Ro @ Co)[:, None]]), atol=1e-15)
        R = Rrel @ Ro
        assert np.allclose(b, np.hstack([R, (-R @ (Co + scale * Crel))[:, None]]), atol=1e-14)
        t = rng.normal(size=3)
        assert np.allclose(map_host.pose_center(Ro, t), -Ro.T @ t, atol=1e-15)

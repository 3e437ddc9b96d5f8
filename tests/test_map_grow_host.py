"""The grow statements of coloc_amd/csrc/map_math.h (their g++ build, tests/host/map_grow_lib.cpp) against numpy, and the Python statement
of the whole grow (tests/map_grow_host.py) on hand-placed tracks, one per branch.  No GPU."""
import itertools

import numpy as np

import map_grow_host
import map_host

F0 = (1000.0, 640.0, 360.0, 0.0, 0.0, 0.0)
K0 = np.array([[1000.0, 0, 640.0], [0, 1000.0, 360.0], [0, 0, 1.0]])


def _look(C):
    """[R|t] of a camera at C looking along +z"""
    return np.hstack([np.eye(3), -np.asarray(C, dtype=np.float64)[:, None]])


def _project(Rt, X):
    u = K0 @ (Rt[:, :3] @ X + Rt[:, 3])
    return u[:2] / u[2]


def test_the_constant_is_cos_two_degrees():
    assert map_grow_host.lib().map_grow_host_cos_2deg() == np.cos(np.deg2rad(2.0))


def test_angle_decision_agrees_with_arccos():
    rng = np.random.default_rng(1)
    n = 10000
    a = rng.normal(size=(n, 3)) * rng.uniform(0.5, 3.0, (n, 1))
    axis = np.cross(a, rng.normal(size=(n, 3)))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.where(rng.random(n) < 0.5, rng.uniform(1.9, 2.1, n), rng.uniform(0.0, 30.0, n))
    th = np.deg2rad(ang)[:, None]
    an = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = (an * np.cos(th) + np.cross(axis, an) * np.sin(th)) * rng.uniform(0.5, 3.0, (n, 1))          # Rodrigues, axis orthogonal to a
    deg = np.rad2deg(np.arccos(np.clip((a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)), -1.0, 1.0)))
    keep = np.abs(deg - 2.0) > 1e-9
    assert keep.sum() > 9900
    got = map_grow_host.angle_over_2deg(a, b)
    assert np.array_equal(got[keep], (deg > 2.0)[keep])
    assert got.any() and not got.all() and (np.abs(deg - 2.0) < 0.01).sum() > 100


def test_grow_point_agrees_with_numpy_svd():
    rng = np.random.default_rng(2)
    Rt_i, Rt_j = _look([0.0, 0.0, 0.0]), _look([1.5, 0.1, -0.05])
    P_i, P_j = K0 @ Rt_i, K0 @ Rt_j
    worst = 0.0
    for _ in range(200):
        X = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(8, 20)])
        x_i, x_j = _project(Rt_i, X), _project(Rt_j, X)
        ok, got = map_grow_host.grow_point(F0, F0, Rt_i, Rt_j, x_i, x_j)
        assert ok
        A = np.stack([x_i[0] * P_i[2] - P_i[0], x_i[1] * P_i[2] - P_i[1], x_j[0] * P_j[2] - P_j[0], x_j[1] * P_j[2] - P_j[1]])
        v = np.linalg.svd(A)[2][-1]
        worst = max(worst, np.abs(got - v[:3] / v[3]).max() / np.abs(X).max())
        assert np.abs(got - X).max() < 1e-6
    assert worst < 1e-9, worst


def test_observation_rule():
    Rt = _look([0.0, 0.0, 6.0])
    assert map_grow_host.observation_ok(Rt, [0.0, 0.0, 7.0]) and not map_grow_host.observation_ok(Rt, [0.0, 0.0, 6.0])
    assert not map_grow_host.observation_ok(Rt, [0.0, 0.0, 4.0])
    assert map_grow_host.observation_ok(Rt, [0.0, 0.0, 999.9]) and not map_grow_host.observation_ok(Rt, [0.0, 0.0, 1000.0])
    assert not map_grow_host.observation_ok(_look([0.0, 0.0, -2000.0]), [0.0, 0.0, -1000.0])


def hand_case():
    """7 cameras looking along +z, the seed pair is (1, 4); one track per branch.  -> (rows, pairs, cams, seed index, poses, row_of)
    with row_of[name][camera] = the row of the named point in that camera."""
    centre = {0: [0.5, 0, 0], 1: [0.0, 0, 0], 2: [1.7, 0, 0], 3: [1.4, 0, 0], 4: [2.0, 0, 0], 5: [1.0, 0, 6.0], 6: [80.0, 0, 0]}
    poses = {c: _look(v) for c, v in centre.items()}
    points = [("A", [1.0, 0.5, 10.0], [0, 1, 2, 3, 4, 5, 6]),      # a seed landmark every camera holds: camera 0 takes its descriptor over
              ("G", [0.6, -0.4, 12.0], [1, 4]),                    # a seed landmark nobody else holds
              ("B", [1.7, 0.3, 10.0], [2, 3, 4]),                  # camera 2: (2, 4) under 2 degrees; camera 3: (3, 2) under, (3, 4) over
              ("D", [1.0, 0.2, 4.0], [1, 4, 5]),                   # a seed landmark BEHIND camera 5 (which stands at z = 6)
              ("E", [40.0, 0.0, 1200.0], [2, 6]),                  # accepted but for |X[2]| >= 1000
              ("E2", [40.0, 0.1, 900.0], [2, 6])]                  # the same rays' twin below 1000
    feats = {c: [] for c in centre}
    row_of = {}
    edges = {}
    for name, X, seen in points:
        row_of[name] = {}
        for c in seen:
            row_of[name][c] = len(feats[c])
            feats[c].append(_project(poses[c], np.array(X)))
        for a, b in zip(seen[:-1], seen[1:]):
            edges.setdefault((a, b), []).append((row_of[name][a], row_of[name][b]))
    cams, rows = [], []
    for c in sorted(centre):
        f = np.zeros((len(feats[c]), 4), dtype=np.float32)
        f[:, :2] = np.array(feats[c])
        cams.append(dict(cam=F0, feat=f))
        rows.append(len(f))
    pair_cams = sorted(edges)
    pairs = [dict(cam_a=a, cam_b=b, q=[e[0] for e in edges[(a, b)]], t=[e[1] for e in edges[(a, b)]]) for a, b in pair_cams]
    return rows, pairs, cams, pair_cams.index((1, 4)), poses, row_of


def _track_of(table, row_of, name):
    c, r = next(iter(row_of[name].items()))
    return int(np.nonzero(table[:, c] == r)[0][0])


def test_hand_placed_branches():
    rows, pairs, cams, seed, poses, row_of = hand_case()
    asked = []

    def pose_of(I, lst):
        asked.append((I, lst["track"].tolist()))
        return poses[I]

    g = map_grow_host.grow_map(rows, pairs, cams, seed, poses[1], poses[4], pose_of)
    table = g["track_feat"]
    assert len(table) == 6 and g["order"] == [0, 2, 3, 5, 6] and g["status"] == [0] * 7
    t = {n: _track_of(table, row_of, n) for n in row_of}
    obs = g["state_obs"]
    assert g["n_seed_rows"] == 3 and sorted(g["seed_tracks"].tolist()) == sorted([t["A"], t["G"], t["D"]])
    # a landmark that exists gains every camera that resects in front of it
    assert obs[t["A"]] == 0b1111111 and obs[t["G"]] == 0b0010010
    # camera 2: its only valid partner, camera 4, is under 2 degrees away -> nothing; camera 3: camera 2 is visited and fails, camera 4
    # succeeds; all three are candidates
    assert asked[1] == (2, [t["A"]]) and asked[2] == (3, [t["A"]]) and t["B"] not in asked[3][1]
    assert obs[t["B"]] == 0b0011100
    assert np.abs(g["state_X"][t["B"]] - [1.7, 0.3, 10.0]).max() < 1e-3
    # behind camera 5: its bit stays clear, and the landmark was in its resection list all the same
    assert obs[t["D"]] == 0b0010010 and t["D"] in asked[3][1] and asked[3][0] == 5
    # |X[2]| >= 1000 drops a point every other part of the rule accepts; its twin at 900 stays
    assert t["E"] not in obs and obs[t["E2"]] == 0b1000100
    assert abs(g["state_X"][t["E2"]][2] - 900.0) < 1.0
    # the map: ascending track id, the lowest camera's row; camera 0 (below the seed's cam_a = 1) takes over track A
    assert g["map_track"].tolist() == sorted([t["A"], t["G"], t["B"], t["D"], t["E2"]]) and g["n_added"] == 2
    row = {int(tr): (int(c), int(r)) for tr, c, r in zip(g["map_track"], g["map_cam"], g["map_row"])}
    assert row[t["A"]] == (0, row_of["A"][0]) and row[t["G"]] == (1, row_of["G"][1]) and row[t["B"]] == (2, row_of["B"][2])
    assert row[t["D"]] == (1, row_of["D"][1]) and row[t["E2"]] == (2, row_of["E2"][2])
    assert g["map_obs"].tolist() == [obs[int(tr)] for tr in g["map_track"]]


def test_failed_cameras_are_skipped():
    rows, pairs, cams, seed, poses, row_of = hand_case()
    g = map_grow_host.grow_map(rows, pairs, cams, seed, poses[1], poses[4], lambda I, lst: None if I in (0, 2) else poses[I])
    t = {n: _track_of(g["track_feat"], row_of, n) for n in row_of}
    assert g["status"] == [map_grow_host.GROW_NO_POSE, 0, map_grow_host.GROW_NO_POSE, 0, 0, 0, 0]
    assert g["state_obs"][t["A"]] == 0b1111010                       # cameras 0 and 2 added nothing
    assert g["state_obs"][t["B"]] == 0b0011000                       # camera 3 meets camera 4 alone
    assert t["E2"] not in g["state_obs"]                             # camera 6 finds no valid partner
    # a camera none of whose tracks has a landmark: no resection list
    keep = [p for p in pairs if 5 not in (p["cam_a"], p["cam_b"])]
    g = map_grow_host.grow_map(rows, keep, cams, [(p["cam_a"], p["cam_b"]) for p in keep].index((1, 4)), poses[1], poses[4], lambda I, lst: poses[I])
    assert g["status"][5] == map_grow_host.GROW_NO_TRACKS and 5 not in g["poses"]

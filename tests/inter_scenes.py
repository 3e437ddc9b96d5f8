"""Synthetic camera pairs for the inter-camera step, shared by tests/test_gpu_inter_pose_dev.py (device against host) and
tests/test_inter_geometry_host.py (host against the committed bits), and the fixed cases of the latter."""
import numpy as np

K = np.array([[1000.0, 0, 640], [0, 1000.0, 360], [0, 0, 1]])
K_SKEWED = np.array([[1000.0, 2.5, 640], [0, 950.0, 360], [0, 0, 1]])         # fx != fy and a skew: the general K of the host path
WH = (1280, 720)
NO_MODEL, NO_RELATIVE_POSE, NO_SCALE = 1, 2, 3


def rot(ax, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax]


def pair(seed, n=900, outliers=0.3, noise=0.4, in_map=0.6, K=K):
    """the recipe of tests/test_gpu_two_view_batch.py: a world of n points, a source and a destination camera, n correspondences (30 % of
    the destination's replaced), a global map that holds 60 % (in_map) of the points in a shuffled order"""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(6, 18, n)], 1)
    Rs, ts = rot("y", rng.uniform(-0.1, 0.1)) @ rot("x", rng.uniform(-0.05, 0.05)), rng.uniform(-0.3, 0.3, 3)
    Rd = rot("y", rng.uniform(0.1, 0.25)) @ rot("z", rng.uniform(-0.05, 0.05)) @ Rs
    td = ts + np.array([rng.uniform(0.6, 1.2), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])

    def proj(R, t):
        u = (X @ R.T + t) @ K.T
        return u[:, :2] / u[:, 2:3]
    x1 = proj(Rs, ts) + rng.normal(0, noise, (n, 2))
    x2 = proj(Rd, td) + rng.normal(0, noise, (n, 2))
    out = rng.choice(n, int(outliers * n), replace=False)
    x2[out] = np.stack([rng.uniform(0, WH[0], len(out)), rng.uniform(0, WH[1], len(out))], 1)
    in_map = rng.random(n) < in_map
    order = rng.permutation(np.nonzero(in_map)[0])
    map_X = X[order] + rng.normal(0, 0.002, (len(order), 3))
    map_index = np.full(n, -1, np.int32)
    map_index[order] = np.arange(len(order), dtype=np.int32)
    return dict(x1=x1, x2=x2, map_index=map_index, Rt_source=np.c_[Rs, ts], Rs=Rs, ts=ts, Rd=Rd, td=td, map_X=map_X, replaced=np.sort(out))


# ---- the host path's fixed cases (tests/golden/inter_geometry_host.npz) -------------------------------------------------------------
# A "front" case is one call of inter_relative: a scene, E from its true relative pose, an inlier list.  A "scale" case is one call of
# inter_scale_pose on a front case's temporary map with a list of common features derived from it by `form`.
#   name -> (seed, n, which inliers, expected stage)
FRONT_CASES = {
    "n60a": (9101, 60, "mixed", 0), "n60b": (9102, 60, "mixed", 0), "n200a": (9103, 200, "mixed", 0), "n200b": (9104, 200, "mixed", 0),
    "n900a": (9105, 900, "mixed", 0), "n900b": (9106, 900, "mixed", 0),
    "few_inliers": (9103, 200, "twelve", NO_MODEL),          # fewer than 13 inliers
    "all_replaced": (9107, 60, "replaced", NO_RELATIVE_POSE),  # 13 replaced points: fewer than 8 in front of both cameras under any motion
    "skewed": (9108, 200, "mixed", 0),                       # K_SKEWED: every term of the pixel normalisation counts
}
#   name -> (front case, form, expected stage).  Forms: "shortcut" ascending front position, "chain" ascending map point (both orders the
#   callers produce), "odd" / "even" the shortcut list cut to that many entries (the two branches of the median), "seven" its first seven,
#   "twin" the shortcut list with one entry repeated: two identical consecutive temporary points, the term the d2 > 1e-9f guard drops
SCALE_CASES = {f + "_" + form: (f, form, 0) for f in ("n60a", "n60b", "n200a", "n200b", "n900a", "n900b") for form in ("shortcut", "chain")}
SCALE_CASES.update({"odd": ("n200a", "odd", 0), "even": ("n200a", "even", 0), "seven": ("n200a", "seven", NO_SCALE), "twin": ("n200b", "twin", 0)})


def front_inputs(name):
    seed, n, which, _ = FRONT_CASES[name]
    Kc = K_SKEWED if name == "skewed" else K
    p = pair(seed, n, K=Kc)
    R = p["Rd"] @ p["Rs"].T
    t = p["td"] - R @ p["ts"]
    t = t / np.linalg.norm(t)
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    kept = np.setdiff1d(np.arange(n), p["replaced"])
    if which == "mixed":            # every true correspondence and a few replaced ones: the vote and the screen both reject something
        inliers = np.sort(np.concatenate([kept, p["replaced"][:max(4, n // 15)]]))
    elif which == "twelve":
        inliers = kept[:12]
    else:
        inliers = p["replaced"][:13]
    return dict(x1=np.ascontiguousarray(p["x1"]), x2=np.ascontiguousarray(p["x2"]), K=Kc.copy(), E=np.ascontiguousarray(E),
                inliers=inliers.astype(np.int32), pair=p)


def common_pairs(form, corr, map_index, map_n):
    """(m, 2) int32: (global map point, temporary map point) in the order the rule walks them"""
    gi = map_index[corr]
    ok = np.nonzero((gi >= 0) & (gi < map_n))[0]
    com = np.stack([gi[ok], ok], 1).astype(np.int32)             # the shortcut: ascending front position
    if form == "chain":
        com = com[np.argsort(com[:, 0], kind="stable")]          # commonFeatures of the sweep: ascending map point
    elif form in ("odd", "even"):
        com = com[:len(com) - ((len(com) & 1) != (form == "odd"))]
    elif form == "seven":
        com = com[:7]
    elif form == "twin":
        j = len(com) // 2
        com = np.concatenate([com[:j + 1], com[j:]])
    return np.ascontiguousarray(com)

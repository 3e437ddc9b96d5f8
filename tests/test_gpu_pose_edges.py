"""The single-pose refinement, its covariance and the scoring kernels on inputs the rest of the suite never offers them: skewed and
anisotropic K, R = I exactly, tiny rotations, rotations up to exact half turns, N from 3 to one-more-than-a-pass of the 512-thread
loop, an active Huber tail, rank-deficient masks -- against the 50-digit reference tests/pose_mp.py.

Every row of CASES runs checks a-d (test_case); e-h are tests of their own.  With -s each test prints the worst value next to its bound.

Bounds (none fitted to the kernel's output):
  a  start pose honoured (zero-noise rows, started AT the true pose): iterations == 0, t returned bit for bit, and
     max |R_out - R_in| <= 16 x max(yardstick, 2^-53), yardstick = the float64 numpy statement exp(log(R_in)) - R_in of
     tests/test_so3_host.py (same rule, same table).
  b  ||A^-1 g||_inf <= 1e-5 at the returned pose, A and g from the reference at 50 digits (the suite's bound on [w|t],
     tests/test_gpu_pnp.py, now against the true minimiser), and cost(p) <= cost(newton_polish(p)) (1 + 1e-9) + 1e-9.
  c  max |cov - A^-1| <= 256 cond2(D A D) 2^-53 max |A^-1|, D = diag(A)^-1/2, A^-1 the reference's AT THE RETURNED POSE; the plain
     float64 numpy evaluation beside it must stay within a quarter of that.  Symmetry: the six columns of the inverse come from six
     independent triangular solves, so the code guarantees cov == cov.T neither bitwise nor to an ulp, only to the inversion's own
     error: |cov - cov.T| <= 2 x the bound above.
  d  rmse == sqrt(cost_ref(p) / (2 n_used)) to 1e-9 relative (n_used is not an output of clc_pnp_refine: it is checked through rmse),
     0 <= iterations <= max_iter.
"""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import pose_mp as pm
from test_so3_host import np_exp, np_log, np_dexp, HALF_TURNS

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
PI = math.pi

KS = {
    "suite": np.array([[1000.0, 0, 320], [0, 1000, 240], [0, 0, 1]]),
    "fx900_fy1100": np.array([[900.0, 0, 320], [0, 1100, 240], [0, 0, 1]]),
    "skew3.5": np.array([[1000.0, 3.5, 320], [0, 1000, 240], [0, 0, 1]]),
    "skew-40_aniso": np.array([[900.0, -40, 320], [0, 1100, 240], [0, 0, 1]]),
    "pp_100_650": np.array([[1000.0, 0, 100], [0, 1000, 650], [0, 0, 1]]),
}


def _axis(seed):
    a = np.random.default_rng(seed).standard_normal(3)
    return a / np.linalg.norm(a)


def _rot(angle, axis):
    return pm.to_float(pm.exp_so3(angle * np.asarray(axis, dtype=np.float64)))


ROTS = {
    "I": np.eye(3),
    "1e-10": _rot(1e-10, _axis(1)), "1e-8": _rot(1e-8, _axis(2)), "1e-5": _rot(1e-5, _axis(3)),
    "1rad": _rot(1.0, _axis(4)), "2.5rad": _rot(2.5, _axis(5)),
    "pi-1e-3": _rot(PI - 1e-3, _axis(6)), "pi-1e-6": _rot(PI - 1e-6, _axis(7)),
    "half_e3": HALF_TURNS["e3"], "half_1-10": HALF_TURNS["(1,-1,0)/sqrt2"], "half_01-1": HALF_TURNS["(0,1,-1)/sqrt2"],
}
NS = [3, 4, 6, 7, 63, 64, 65, 511, 512, 513, 600]

# (id, K, rotation, N, noise px, outlier fraction, huber_a)
CASES = []
for _k in KS:
    for _r in ROTS:
        CASES.append(("K-%s-R-%s" % (_k, _r), _k, _r, 600, 0.5, 0.0, 16.0))
for _r in ("I", "2.5rad"):
    for _n in NS:
        CASES.append(("N-%d-R-%s" % (_n, _r), "skew-40_aniso", _r, _n, 0.5, 0.0, 16.0))
for _r in ("I", "2.5rad", "half_1-10"):
    for _a in (16.0, 2.0, 0.0):
        CASES.append(("huber-%g-R-%s" % (_a, _r), "skew3.5", _r, 600, 0.5, 0.2, _a))
for _r in ROTS:
    CASES.append(("exact-R-%s" % _r, "suite", _r, 600, 0.0, 0.0, 16.0))
for _r in ("I", "2.5rad"):
    CASES.append(("exact-N-3-R-%s" % _r, "skew-40_aniso", _r, 3, 0.0, 0.0, 16.0))


def test_the_case_table_is_complete():
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)) == 5 * 11 + 2 * 11 + 9 + 11 + 2
    assert {(c[1], c[2]) for c in CASES if c[3] == 600 and c[4] == 0.5 and c[5] == 0.0} >= {(k, r) for k in KS for r in ROTS}
    assert {c[3] for c in CASES if c[0].startswith("N-")} == set(NS)
    assert {c[6] for c in CASES if c[5] > 0} == {16.0, 2.0, 0.0} and {c[2] for c in CASES if c[4] == 0.0} >= set(ROTS)


def scene(K, R, n, noise, outliers, seed):
    """n points 4 - 20 units in front of the camera [R | t]; observations with Gaussian noise, a fraction replaced by gross outliers."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(4, 20, n)
    Xc = np.stack([rng.uniform(-0.25, 0.25, n) * z, rng.uniform(-0.2, 0.2, n) * z, z], 1)
    t = np.array([0.3, -0.2, 0.5])
    X = (Xc - t) @ R
    uvw = (X @ R.T + t) @ K.T
    x = uvw[:, :2] / uvw[:, 2:3] + noise * rng.standard_normal((n, 2))
    n_out = int(outliers * n)
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        x[idx] += rng.uniform(40, 200, (n_out, 2)) * rng.choice([-1.0, 1.0], (n_out, 2))
    return X, x, np.concatenate([R, t[:, None]], 1)


def perturbed(Rt, seed):
    a = _axis(seed + 1000)
    d = _axis(seed + 2000)
    return np.concatenate([_rot(0.02, a) @ Rt[:, :3], (Rt[:, 3] + 0.05 * d)[:, None]], 1)


def _params(Rt):
    """[log R | t] of a float64 pose, the logarithm taken at 50 digits."""
    return pm.log_so3(Rt[:, :3]) + pm.vec(Rt[:, 3])


def _np_normal_matrix(p, X, x, K, a):
    """The same A = sum w J^T J in plain float64 numpy (analytic J from the yardstick's rotation derivative)."""
    w, t = p[:3], p[3:]
    R, dR = np_exp(w), np_dexp(w)
    Xc = X @ R.T + t
    uvw = Xc @ K.T
    r = x - uvw[:, :2] / uvw[:, 2:3]
    s = (r ** 2).sum(1)
    wgt = np.where(s <= a * a, 1.0, a / np.sqrt(np.maximum(s, 1e-300)))
    iz = 1.0 / Xc[:, 2]
    xn, yn = Xc[:, 0] * iz, Xc[:, 1] * iz
    P = np.zeros((len(X), 2, 3))
    P[:, 0, 0] = K[0, 0] * iz; P[:, 0, 1] = K[0, 1] * iz; P[:, 0, 2] = -(K[0, 0] * xn + K[0, 1] * yn) * iz
    P[:, 1, 1] = K[1, 1] * iz; P[:, 1, 2] = -K[1, 1] * yn * iz
    D = np.concatenate([np.einsum("kij,nj->nik", dR, X), np.broadcast_to(np.eye(3), (len(X), 3, 3))], 2)
    J = np.einsum("nab,nbk->nak", P, D)
    return np.einsum("n,nai,naj->ij", wgt, J, J)


def _start_bound(R):
    return 16.0 * max(np.abs(np_exp(np_log(R)) - R).max(), EPS)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case(gpu_ctx, case):
    cid, kname, rname, n, noise, outliers, huber = case
    K, R = KS[kname], ROTS[rname]
    seed = CASES.index(case)
    X, x, Rt_true = scene(K, R, n, noise, outliers, 7000 + seed)
    a_eff = huber if huber > 0 else 16.0
    rec = []
    if noise == 0.0:
        # a: the start pose is honoured
        Rt_a, _, rmse_a, it_a = gpu_ctx.pnp_refine(X, x, K, Rt_true, huber_a=huber)
        dev, bound = np.abs(Rt_a[:, :3] - R).max(), _start_bound(R)
        rec.append("a: iterations %d, |R_out - R_in| %.2e <= %.2e, rmse %.2e" % (it_a, dev, bound, rmse_a))
        assert it_a == 0, rec
        assert np.array_equal(Rt_a[:, 3], Rt_true[:, 3]) and dev <= bound, rec
    Rt, cov, rmse, it = gpu_ctx.pnp_refine(X, x, K, perturbed(Rt_true, seed), huber_a=huber, max_iter=50)
    assert np.isfinite(Rt).all() and np.isfinite(cov).all()
    p = _params(Rt)
    # b: the minimum
    d, A, g, cost = pm.newton_step(p, X, x, K, a_eff)
    step = float(max(abs(v) for v in d))
    q, _ = pm.newton_polish(p, X, x, K, a_eff)
    cost_min = pm.huber_cost(q, X, x, K, a_eff)
    rec.append("b: |A^-1 g| %.2e <= 1e-5, cost %.12g vs minimum %.12g" % (step, float(cost), float(cost_min)))
    assert step <= 1e-5, rec
    assert cost <= cost_min * (1 + mpf(10) ** -9) + mpf(10) ** -9, rec
    if n == 3 and noise == 0.0:
        assert rmse <= 1e-6, rec
    # c: the covariance at the returned pose.  Next to a half turn the pose has two angle-axis vectors of length about pi (w and
    # w (1 - 2 pi / |w|)), the covariance is a statement in one chart, and only R is returned: the chart the kernel stopped in is the
    # one of the two its covariance belongs to -- both are tried there, the better one counts (the same one for the numpy evaluation).
    charts = [(p, A)]
    th = mp.sqrt(sum(v * v for v in p[:3]))
    if th > mp.pi - mpf("0.1"):
        p2 = [v * (1 - 2 * mp.pi / th) for v in p[:3]] + p[3:]
        charts.append((p2, pm.normal_equations(p2, X, x, K, a_eff)[0]))
    best = None
    for pc, Ac in charts:
        Ainv = pm.to_float(mp.inverse(Ac))
        Af = pm.to_float(Ac)
        Dh = 1.0 / np.sqrt(np.diag(Af))
        cond = float(np.linalg.cond(Af * Dh[:, None] * Dh[None, :]))
        bound = 256.0 * cond * EPS * np.abs(Ainv).max()
        err_np = np.abs(np.linalg.inv(_np_normal_matrix(pm.to_float(pc), X, x, K, a_eff)) - Ainv).max()
        err_gpu = np.abs(cov - Ainv).max()
        if best is None or err_gpu / bound < best[0] / best[2]:
            best = (err_gpu, err_np, bound, cond)
    err_gpu, err_np, bound, cond = best
    rec.append("c: |cov - A^-1| %.2e (numpy %.2e) <= %.2e, cond %.2e, asymmetry %.2e" % (err_gpu, err_np, bound, cond, np.abs(cov - cov.T).max()))
    assert err_np <= bound / 4, rec
    assert err_gpu <= bound, rec
    assert np.abs(cov - cov.T).max() <= 2 * bound, rec
    # d: rmse, iterations
    rmse_ref = float(mp.sqrt(cost / (2 * n)))
    rec.append("d: rmse %.12g vs %.12g, iterations %d" % (rmse, rmse_ref, it))
    # (absolute floor: a float64 residual is obs - proj of numbers of size max |x|, so it -- and an rmse made of such -- is not
    # resolved below a few ulp of that; it matters only where the minimum is zero: exact data, N = 3)
    assert abs(rmse - rmse_ref) <= 1e-9 * rmse_ref + 64 * EPS * np.abs(x).max(), rec
    assert 0 <= it <= 50, rec
    print("\n%-28s %s" % (cid, " | ".join(rec)))


def test_e_rank_deficient_masks_and_argument_rules(gpu_ctx):
    from coloc_amd.abi import CLCError, CLC_ERR_BAD_ARG
    K, R = KS["skew-40_aniso"], ROTS["2.5rad"]
    X, x, Rt_true = scene(K, R, 600, 0.5, 0.0, 7900)
    Rt0 = perturbed(Rt_true, 77)
    full = gpu_ctx.pnp_refine(X, x, K, Rt0)
    assert full[1].any()                                  # the record a failed inversion must not leave standing
    for keep in (0, 1, 2):
        mask = np.zeros(600, dtype=np.uint8)
        mask[[17, 400][:keep]] = 1
        Rt, cov, rmse, it = gpu_ctx.pnp_refine(X, x, K, Rt0, mask=mask)
        print("\ne: mask leaves %d: max |cov| %.3e, rmse %.3e, iterations %d" % (keep, np.abs(cov).max(), rmse, it))
        assert np.isfinite(Rt).all() and np.isfinite(rmse) and 0 <= it <= 50
        assert not cov.any(), "rank-deficient normal matrix passed as positive definite"
        if keep == 0:
            assert rmse == 0.0 and np.array_equal(Rt[:, 3], Rt0[:, 3]) and np.abs(Rt[:, :3] - Rt0[:, :3]).max() <= _start_bound(Rt0[:, :3])
        else:
            # n_used == mask count, through rmse = sqrt(cost / (2 n_used)) at the returned pose
            c = pm.huber_cost(_params(Rt), X, x, K, 16.0, mask=mask)
            assert abs(rmse - float(mp.sqrt(c / (2 * keep)))) <= 1e-9 * rmse + 1e-12
    for n in (0, 1, 2):
        with pytest.raises(CLCError) as ei:
            gpu_ctx.pnp_refine(X[:n], x[:n], K, Rt0)
        assert ei.value.status == CLC_ERR_BAD_ARG
    r0 = gpu_ctx.pnp_refine(X, x, K, Rt0, max_iter=0)
    r50 = gpu_ctx.pnp_refine(X, x, K, Rt0, max_iter=50)
    assert np.array_equal(r0[0], r50[0]) and np.array_equal(r0[1], r50[1]) and r0[2:] == r50[2:]
    r1 = gpu_ctx.pnp_refine(X, x, K, Rt0, max_iter=1)
    assert 0 <= r1[3] <= 1 and np.isfinite(r1[0]).all()


@pytest.mark.parametrize("kname", list(KS))
def test_f_scoring_kernels_equal_the_oracle(gpu_ctx, oracle, kname):
    K = KS[kname]
    for H in (1, 3, 257):
        for n in (1, 255, 256, 257, 600):
            rng = np.random.default_rng(31 * H + n)
            X, x, _ = scene(K, np.eye(3), n, 0.5, 0.0, 8000 + n)
            X = X + np.array([0.3, -0.2, 0.5])             # world frame = camera frame of hypothesis 0 = [I | 0]
            behind = rng.choice(n, n // 10, replace=False)
            X[behind, 2] *= -1.0
            X[0] = [1.0, 2.0, 0.0]                         # on the principal plane of hypothesis 0: u / 0
            if n > 1:
                X[1] = [0.0, 0.0, 0.0]                     # 0 / 0
            Rt = [np.concatenate([np.eye(3), np.zeros((3, 1))], 1)]
            pool = [ROTS["2.5rad"], ROTS["half_1-10"], ROTS["1e-8"]]
            for h in range(1, H):
                Rh = _rot(0.05 * rng.random(), _axis(h)) @ (pool[h % 3] if h % 5 == 0 else np.eye(3))
                Rt.append(np.concatenate([Rh, 0.05 * rng.standard_normal((3, 1))], 1))
            Rt = np.array(Rt).reshape(H, 12)
            e = gpu_ctx.pnp_residuals(Rt, X, x, K)
            eo = oracle.pnp_residuals(Rt, X, x, K)
            assert np.isinf(eo[0, 0]) and (n == 1 or np.isnan(eo[0, 1]))
            assert np.array_equal(e, eo, equal_nan=True), (H, n)
            cnt, cost = gpu_ctx.pnp_score(Rt, X, x, K, 16.0)
            cnt_o, cost_o = oracle.pnp_score(eo, 16.0)
            assert np.array_equal(cnt, cnt_o) and np.isfinite(cost).all(), (H, n)
            assert np.allclose(cost, cost_o, rtol=1e-12, atol=0), (H, n)
            assert np.array_equal(cnt, (np.nan_to_num(eo, nan=np.inf) < 16.0).sum(1))      # NaN / inf are no inliers


@pytest.mark.parametrize("kname,rname", [("skew-40_aniso", "2.5rad"), ("suite", "half_1-10")])
def test_g_fused_paths_equal_the_plain_one(gpu_ctx, kname, rname):
    from coloc_amd import Context
    from coloc_amd.abi import pnp_localize_batch
    K, R = KS[kname], ROTS[rname]
    X, x, Rt_true = scene(K, R, 600, 0.5, 0.2, 8100)
    rng = np.random.default_rng(4)
    samples = np.stack([rng.choice(600, 3, replace=False) for _ in range(256)]).astype(np.int32)
    Rt0, mask0, _ = gpu_ctx.pnp_ransac(X, x, K, samples=samples, thr2=16.0)
    assert Rt0 is not None and np.abs(Rt0 - Rt_true).max() < 0.05
    Rt1, cov1, rmse1, _ = gpu_ctx.pnp_refine(X, x, K, Rt0, mask=mask0)
    Rt2, cov2, mask2, rmse2 = gpu_ctx.pnp_localize(X, x, K, samples=samples, thr2=16.0)
    assert np.array_equal(mask0, mask2) and np.array_equal(Rt1, Rt2) and np.array_equal(cov1, cov2) and rmse1 == rmse2
    a = gpu_ctx.pnp_acransac(X, x, K, seed=3)
    assert a["Rt"] is not None
    Rt3, cov3, rmse3, _ = gpu_ctx.pnp_refine(X, x, K, a["Rt"], mask=a["mask"])
    r = gpu_ctx.pnp_acransac(X, x, K, seed=3, refine=True)
    assert np.array_equal(r["inliers"], a["inliers"])
    assert np.array_equal(r["Rt"], Rt3) and np.array_equal(r["cov"], cov3) and r["rmse"] == rmse3
    ctxs = [Context(device=0, detector=False, matcher=False) for _ in range(3)]
    try:
        got = pnp_localize_batch(ctxs, [(X, x, K)] * 3, max_iteration=256, seeds=[3, 3, 3], refine=True)
        for gb in got:
            assert np.array_equal(gb["Rt"], Rt3) and np.array_equal(gb["cov"], cov3) and gb["rmse"] == rmse3
    finally:
        for c in ctxs:
            c.close()
    assert np.abs(Rt3 - Rt_true).max() < 5e-3


def test_g_inter_pose_from_a_half_turn_source():
    """clc_inter_pose_batch with Rt_source an exact half turn about (1,-1,0)/sqrt2: the world of the existing test re-expressed in a frame
    in which the source camera's rotation is that signed permutation matrix; same bounds as test_inter_pose_batch_lands_on_the_destination_pose."""
    from coloc_amd import Context
    from coloc_amd.abi import inter_pose_batch
    from test_gpu_two_view_batch import _pair
    p = _pair(300, n=1000)
    P = HALF_TURNS["(1,-1,0)/sqrt2"]
    S = p["Rt_source"]
    G = S[:, :3].T @ P                                    # rows: X' = X G  (X' = P^T Rs X), so that Rs X = P X'
    q = dict(p)
    q["map_X"] = p["map_X"] @ G
    q["Rt_source"] = np.c_[P, S[:, 3]]
    Rd = p["Rd"] @ G
    ctx = Context(device=0, detector=False, matcher=False)
    try:
        r = inter_pose_batch([ctx], [q], q["map_X"])[0]
    finally:
        ctx.close()
    assert r["status"] == 0 and r["stage"] == 0, r["stage"]
    Rt = r["Rt"]
    ang = np.degrees(np.arccos(np.clip((np.trace(Rt[:, :3] @ Rd.T) - 1) / 2, -1, 1)))
    Cd, Ce = -Rd.T @ p["td"], -Rt[:, :3].T @ Rt[:, 3]
    print("\ng: inter-pose from a half-turn source: angle %.3f deg, centre %.3f, rmse %.3f" % (ang, np.linalg.norm(Ce - Cd), r["rmse"]))
    assert ang < 0.6 and np.linalg.norm(Ce - Cd) < 0.2
    assert 0 < r["rmse"] < 2.0 and np.all(np.linalg.eigvalsh(r["cov"]) > 0)


def test_h_pose_entry_points_refuse_a_K_that_is_not_upper_triangular_with_unit_last_row(gpu_ctx):
    """The contract: the pose solvers read K as { fx, skew, cx; 0, fy, cy; 0, 0, 1 }; anything else is CLC_ERR_BAD_ARG (the residual and
    score entry points apply all nine entries and accept any K)."""
    from coloc_amd.abi import CLCError, CLC_ERR_BAD_ARG
    K = KS["skew-40_aniso"]
    X, x, Rt_true = scene(K, ROTS["1rad"], 64, 0.5, 0.0, 8200)
    K3 = K.copy(); K3[1, 0] = 1e-3
    samples = np.array([[0, 1, 2]], dtype=np.int32)
    for bad in (2.0 * K, K3):
        for call in (lambda: gpu_ctx.pnp_refine(X, x, bad, Rt_true), lambda: gpu_ctx.pnp_localize(X, x, bad),
                     lambda: gpu_ctx.pnp_acransac(X, x, bad, refine=True), lambda: gpu_ctx.pnp_p3p(X, x, bad, samples),
                     lambda: gpu_ctx.pnp_ransac(X, x, bad), lambda: gpu_ctx.pnp_acransac(X, x, bad)):
            with pytest.raises(CLCError) as ei:
                call()
            assert ei.value.status == CLC_ERR_BAD_ARG
        assert np.isfinite(gpu_ctx.pnp_residuals(Rt_true.reshape(1, 12), X, x, bad)).all()
    assert gpu_ctx.pnp_refine(X, x, K, Rt_true)[3] >= 0

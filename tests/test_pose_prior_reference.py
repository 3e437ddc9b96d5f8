"""The pose-from-the-prediction rule (include/coloc_hip.h, THE RULE of clc_track_prior_dev): its float64 statement
tests/pose_prior_host.py against the 50-digit reference tests/pose_prior_mp.py on the case table tests/pose_prior_cases.py.  CPU only.

For every case:
  the INPUT CONDITION, asserted on the reference alone: at every reference round no track has sq within [0.95 g2, 1.05 g2] and none has
  |zc| < 1e-6.  The band is wide because rule b below bounds the returned parameters only to 1e-5, about 5e-3 px at these focals; a seed
  that violates it is a wrong fixture and is replaced in the table, not tolerated here.
  With the condition met the float64 statement must give the reference's masks round by round, its rounds_run, converged and result, and
  its pose must satisfy rule b of tests/test_gpu_pose_edges.py as it stands, with A and g from the reference over the final mask:
  ||A^-1 g||_inf <= 1e-5 and cost <= cost(newton_polish(p)) (1 + 1e-9) + 1e-9.
"""
import numpy as np
import pytest
from mpmath import mpf

import pose_mp as pm
import pose_prior_cases as pc
import pose_prior_host as ph
import pose_prior_mp as ppm


def rule_b(p, X, x, K, a, mask, rec):
    """Rule b of test_gpu_pose_edges.py at parameters p (50 digits) over `mask`; returns (A, cost) of the reference at p."""
    d, A, g, cost = pm.newton_step(p, X, x, K, a, mask=mask)
    step = float(max(abs(v) for v in d))
    q, _ = pm.newton_polish(p, X, x, K, a, mask=mask)
    cost_min = pm.huber_cost(q, X, x, K, a, mask=mask)
    rec.append("b: |A^-1 g| %.2e <= 1e-5, cost %.12g vs minimum %.12g" % (step, float(cost), float(cost_min)))
    assert step <= 1e-5, rec
    assert cost <= cost_min * (1 + mpf(10) ** -9) + mpf(10) ** -9, rec
    return A, cost


def test_the_case_table_is_complete():
    assert len(pc.IDS) == len(set(pc.IDS))
    regular = [c for c in pc.CASES if c[6] == "regular" and c[3] > 3]
    assert {c[3] for c in regular} == {4, 8, 64, 511, 512, 513, 1025, 2000}
    assert {c[4] for c in regular} == {0.0, 0.1, 0.3}
    assert any(c[3] == 3 for c in pc.CASES) and any(c[6] == "behind" for c in pc.CASES)
    for cid in pc.IDS:
        c = pc.build(cid)
        uvw = (c["X"] @ c["Rt_true"][:, :3].T + c["Rt_true"][:, 3]) @ c["K"].T
        e = np.linalg.norm(c["x"] - uvw[:, :2] / uvw[:, 2:3], axis=1)
        assert (e[~c["outliers"]] <= 0.5 * pc.GATE + 1e-9).all() and (e[c["outliers"]] >= 4 * pc.GATE - 0.5 * pc.GATE - 1e-9).all()
    b = pc.build("behind-64")
    assert ((b["X"] @ b["Rt_prior"][:, :3].T + b["Rt_prior"][:, 3])[:, 2] < 0).all()


@pytest.mark.parametrize("cid", pc.IDS)
def test_float64_statement_equals_the_reference(cid):
    c = pc.build(cid)
    ref = pc.reference_live(cid)
    bad = ppm.band_violations(ref)
    assert not bad, "wrong fixture (replace the seed): tracks in the band / next to the principal plane: %r" % bad[:5]
    got = ph.solve(c["X"], c["x"], c["K"], c["Rt_prior"], pc.GATE, pc.HUBER)
    rec = ["%s: rounds %d, converged %d, result %d, masks %s" % (cid, ref["rounds_run"], ref["converged"], ref["result"],
                                                              [int(m.sum()) for m in ref["masks"]])]
    assert len(got["masks"]) == len(ref["masks"]), rec
    for k, (a, b) in enumerate(zip(got["masks"], ref["masks"])):
        assert np.array_equal(a, b), (rec, "round %d" % k, np.flatnonzero(a != b))
    assert np.array_equal(got["mask"], ref["mask"]) and got["n_inliers"] == ref["n_inliers"], rec
    assert (got["rounds_run"], got["converged"], got["result"]) == (ref["rounds_run"], ref["converged"], ref["result"]), rec
    if ref["rounds_run"] == 0:
        assert np.array_equal(got["Rt"], c["Rt_prior"]) and not got["cov"].any(), rec
    else:
        # the pose minimises over the last mask a round ran on: the final mask where it is stable, else the one before it
        rule_b(pm.vec(got["p"]), c["X"], c["x"], c["K"], pc.HUBER, ref["mask"] if ref["converged"] else ref["masks"][-2], rec)
    # the record the GPU tests read is this solve's
    assert pc._golden().get(cid) == pc.record(cid, ref), "tests/golden/pose_prior_reference.json is stale: run tools/make_pose_prior_reference.py"
    print("\n" + " | ".join(rec))

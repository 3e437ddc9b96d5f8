"""The a-contrario 3-D similarity on the GPU (clc_sim3_acransac, clc_sim3_minimal: coloc_amd/csrc/acransac.hip kind 4 + sim3_math.h)
against the host build of the same header and the sequential statement on top of it (tests/sim3_host.py): every output, the
floating-point ones bit for bit.  The sizes are those at which the sort changes shape: one wave, several waves, and 1 -> 2 -> 4
elements per thread."""
import numpy as np
import pytest

import sim3_cases
import sim3_host
from coloc_amd import abi

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check(got, want):
    for k in ("found", "n_inliers", "iterations", "valid", "refit"):
        assert got[k] == want[k], k
    assert np.array_equal(got["inliers"], want["inliers"]) and np.array_equal(got["mask"], want["mask"])
    for k in ("A", "R", "t"):
        assert _same_bits(got[k], want[k]), k
    for k in ("s", "min_nfa", "error_max"):
        assert _same_bits([got[k]], [want[k]]), (k, got[k], want[k])


def test_minimal_equals_the_host_build_on_the_case_list(gpu_ctx):
    cases = sim3_cases.minimal_cases()
    x = np.concatenate([c[1] for c in cases])
    y = np.concatenate([c[2] for c in cases])
    smp = np.arange(3 * len(cases), dtype=np.int32).reshape(-1, 3)
    dev = gpu_ctx.sim3_minimal(x, y, smp)
    host = sim3_host.minimal_of_samples(x, y, smp)
    differ = [c[0] for c, d, h in zip(cases, dev, host) if not _same_bits(d, h)]
    assert not differ, differ
    for c, mo in zip(cases, dev):
        assert np.isnan(mo).all() == (c[3] == "nan"), c[0]


def test_minimal_equals_the_host_build_on_random_samples(gpu_ctx):
    sc = sim3_cases.planted_scene(500, 0.3, 77, noise=1e-3, duplicates=20)
    rng = np.random.default_rng(8)
    smp = np.stack([rng.choice(len(sc["x"]), 3, replace=False) for _ in range(256)]).astype(np.int32)
    smp[5] = [3, 3, 9]                                                 # a repeated correspondence: degenerate
    dev = gpu_ctx.sim3_minimal(sc["x"], sc["y"], smp)
    assert _same_bits(dev, sim3_host.minimal_of_samples(sc["x"], sc["y"], smp)) and np.isnan(dev[5]).all()
    assert np.isfinite(dev).all(1).sum() >= 250
    # an index that names no correspondence gives no model
    bad = np.array([[0, 1, len(sc["x"])], [-1, 2, 3]], dtype=np.int32)
    assert np.isnan(gpu_ctx.sim3_minimal(sc["x"], sc["y"], bad)).all()


@pytest.mark.parametrize("n", [4, 7, 64, 65, 300, 1024, 1025, 2049])
def test_acransac_equals_the_sequential_statement(gpu_ctx, n):
    dup = 0 if n < 64 else 5
    sc = sim3_cases.planted_scene(n - dup, 0.3, 500 + n, noise=1e-4, duplicates=dup)
    assert len(sc["x"]) == n
    got = gpu_ctx.sim3_acransac(sc["x"], sc["y"], max_iteration=256, seed=n)
    want = sim3_host.acransac(sc["x"], sc["y"], max_iteration=256, seed=n)
    _check(got, want)
    assert got["found"] == (n >= 64)
    if got["found"]:
        assert got["refit"] == 1 and abs(got["s"] - 2.5) < 1e-3 and not (got["mask"] & ~sc["planted"]).any()
    # two runs on one input give the same bits
    _check(gpu_ctx.sim3_acransac(sc["x"], sc["y"], max_iteration=256, seed=n), got)


def test_acransac_under_an_upper_bound(gpu_ctx):
    sc = sim3_cases.planted_scene(300, 0.3, 901, noise=1e-4)
    for precision in (1e-2, 1e-9):
        _check(gpu_ctx.sim3_acransac(sc["x"], sc["y"], max_iteration=128, seed=5, precision=precision),
               sim3_host.acransac(sc["x"], sc["y"], max_iteration=128, seed=5, precision=precision))


def test_pure_outliers_spend_every_iteration(gpu_ctx):
    rng = np.random.default_rng(9)
    x, y = rng.uniform(-10, 10, (40, 3)), rng.uniform(-10, 10, (40, 3))
    got = gpu_ctx.sim3_acransac(x, y, max_iteration=256, seed=3)
    _check(got, sim3_host.acransac(x, y, max_iteration=256, seed=3))
    assert not got["found"] and got["iterations"] == 256 and got["n_inliers"] == 0 and not got["mask"].any()
    assert got["s"] == 1.0 and np.array_equal(got["R"], np.eye(3)) and not got["t"].any()


def test_no_solve_cases_and_capacity(gpu_ctx):
    rng = np.random.default_rng(10)
    x, y = rng.uniform(-10, 10, (40, 3)), rng.uniform(-10, 10, (40, 3))
    got = gpu_ctx.sim3_acransac(x[:3], y[:3])
    _check(got, sim3_host.acransac(x[:3], y[:3]))
    assert not got["found"] and got["iterations"] == 0
    flat = y.copy()
    flat[:, 1] = -2.0                                                  # a flat box of old points: V = 0
    got = gpu_ctx.sim3_acransac(x, flat)
    _check(got, sim3_host.acransac(x, flat))
    assert not got["found"] and got["iterations"] == 0 and got["s"] == 1.0
    big = np.zeros((16385, 3))
    with pytest.raises(abi.CLCError) as e:
        gpu_ctx.sim3_acransac(big, big)
    assert e.value.status == abi.CLC_ERR_CAPACITY
    # the context still serves afterwards
    sc = sim3_cases.planted_scene(64, 0.3, 12)
    assert gpu_ctx.sim3_acransac(sc["x"], sc["y"], seed=12)["found"]

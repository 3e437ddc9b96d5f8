"""The device's minimal two-view solvers against the high-precision reference (tests/twoview_mp.py, tests/golden/twoview_reference.npz,
tests/golden/fivept_reference.npz): the two rules of DESIGN.md section 11, one clc_two_view_minimal call per class of
tests/twoview_cases.py (S = the class size), judged by the same evaluate and the same asserts as the host build in
tests/test_twoview_reference.py.  The backward error of every returned model is one 3 x 3 SVD at 60 digits; the forward rule is float
arithmetic against the reference models as hi + lo pairs.
acr_round_kernel solves its samples with the same acr_twoview_sample_root body, and tests/test_gpu_two_view_models.py::
test_equals_sequential_oracle ties the filter's in-loop solve to clc_two_view_minimal bit for bit (the oracle there is fed the
models of this entry and must be reproduced exactly), so the a-contrario 'F' and 'H' paths are held through this file too.
The five-point classes are held the same way through one essential_fivepoint call per class; acr_solve5_kernel calls the same
models_of_sample body (tests/test_gpu_acransac.py ties the two).  Run with -s to see the figures.
"""
import numpy as np
import pytest

import twoview_cases as cases

pytestmark = pytest.mark.gpu
ALL = cases.all_classes()
IDS = ["%s-%s" % mc for mc in ALL]


@pytest.fixture(scope="module")
def fx():
    return cases.load_fixture()


@pytest.fixture(scope="module")
def fx_e():
    return cases.load_fixture("E")


def device_slots(ctx, model, name, fx):
    x1, x2, wh, smp = cases.flat_inputs(model, name, fx)
    return ctx.two_view_minimal(model, x1, x2, wh, smp)


@pytest.mark.parametrize("model,name", ALL, ids=IDS)
def test_minimal_kernel_meets_both_rules(gpu_ctx, fx, model, name):
    slots = device_slots(gpu_ctx, model, name, fx)
    assert slots.shape == (cases.N_PER_CLASS, cases.SLOTS[model], 9)
    fig = cases.evaluate(model, name, slots, fx)            # (check_slots inside: every slot all NaN or wholly finite, NaN slots last)
    print("\n%s %s (device): %s" % (model, name, fig))
    assert fig["models"] > 0
    assert fig["backward_ratio"] <= 1.0
    assert fig["missed"] == 0 and fig["spurious"] == 0


@pytest.mark.parametrize("model,name", [("F", "exact"), ("H", "exact")])
def test_one_call_per_sample_gives_the_same_bits(gpu_ctx, fx, model, name):
    x1, x2, wh, smp = cases.flat_inputs(model, name, fx)
    whole = gpu_ctx.two_view_minimal(model, x1, x2, wh, smp)
    for i in range(len(smp)):
        one = gpu_ctx.two_view_minimal(model, x1, x2, wh, smp[i:i + 1])
        assert one.shape == (1,) + whole.shape[1:]
        assert np.array_equal(one[0].view(np.uint64), whole[i].view(np.uint64))


@pytest.mark.parametrize("name", cases.classes("E"))
def test_five_point_kernel_meets_both_rules(gpu_ctx, fx_e, name):
    """The two rules on coloc_amd/csrc/fivept_wave.h: one essential_fivepoint call of the class's 30 samples, judged over the whole class
    by the same evaluate and the same asserts as the host build (tests/test_twoview_reference.py); and the structure: at most ten slots
    per sample, each all NaN or wholly finite, no two returned models matched to one reference solution."""
    x1, x2, K, smp = cases.flat_inputs("E", name, fx_e)
    slots = gpu_ctx.essential_fivepoint(x1, x2, K, K, smp)
    assert slots.shape == (cases.N_PER_CLASS, 10, 9)
    fig = cases.evaluate("E", name, slots, fx_e)
    print("\nE %s (device): %s" % (name, fig))
    assert fig["refs"] == sum(len(row["refs"]) for row in cases.class_table(fx_e, "E", name)[3]) > 0
    assert fig["models"] > 0
    assert fig["backward_ratio"] <= 1.0
    assert fig["missed"] == 0 and fig["spurious"] == 0 and fig["doubled"] == 0

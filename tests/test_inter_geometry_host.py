"""The host path of the inter-camera step (coloc_amd/csrc/inter_geometry.cpp: inter_relative, inter_scale_pose, over the statements of
inter_math.h that inter_front_kernel / inter_scale_kernel share) against tests/golden/inter_geometry_host.npz, bit for bit, on the CPU.

The fixture was written by tools/make_inter_geometry_golden.py from the commit BEFORE the arithmetic moved into inter_math.h, so an
edit of a shared statement that changes a result shows here without a GPU; tests/test_gpu_inter_pose_dev.py then holds the device to
the host.  Values are compared as uint64 bit patterns, counts and indices as integers; the arrays of more than 200 entries through the
SHA-256 of their bytes (inter_geometry_host.fixture_form), which keeps the fixture small."""
import os

import numpy as np
import pytest

import inter_geometry_host as H
import inter_scenes as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inter_geometry_host.npz")


@pytest.fixture(scope="module")
def results():
    got = H.run_cases()
    return got, H.fixture_form(got), dict(np.load(GOLDEN))


def _same(got, want, key):
    g, w = np.asarray(got[key]), np.asarray(want[key])
    assert g.shape == w.shape, (key, g.shape, w.shape)
    if g.dtype.kind == "f":
        g, w = np.ascontiguousarray(g, np.float64).view(np.uint64), np.ascontiguousarray(w, np.float64).view(np.uint64)
    assert np.array_equal(g, w), (key, int((g != w).sum()), "entries differ")


def test_the_cases_are_the_fixtures(results):
    _, got, want = results
    assert sorted(got) == sorted(want)
    for name in S.FRONT_CASES:
        _same(got, want, "front/%s/inliers" % name)
    for name in S.SCALE_CASES:
        _same(got, want, "scale/%s/common" % name)


@pytest.mark.parametrize("name", sorted(S.FRONT_CASES))
def test_inter_relative_bits(results, name):
    _, got, want = results
    assert int(got["front/%s/stage" % name]) == S.FRONT_CASES[name][3]
    for k in ("stage", "n_front", "corr", "Xt", "x2f", "R", "t"):
        _same(got, want, "front/%s/%s" % (name, k))


@pytest.mark.parametrize("name", sorted(S.SCALE_CASES))
def test_inter_scale_pose_bits(results, name):
    _, got, want = results
    assert int(got["scale/%s/stage" % name]) == S.SCALE_CASES[name][2]
    for k in ("stage", "n_common", "scale", "Rt", "Xw"):
        _same(got, want, "scale/%s/%s" % (name, k))


def test_the_cases_take_their_branches(results):
    got, _, _ = results
    for name, (_, _, which, _) in S.FRONT_CASES.items():
        if which == "mixed":
            assert 8 <= int(got["front/%s/n_front" % name]) < len(got["front/%s/inliers" % name])          # the vote rejects something
    for name, (fname, form, stage) in S.SCALE_CASES.items():
        if form in ("shortcut", "chain") and not fname.startswith("n60"):
            assert 8 <= int(got["scale/%s/n_common" % name]) < len(got["scale/%s/common" % name])          # and so does the screen
    assert len(got["scale/odd/common"]) & 1 and not len(got["scale/even/common"]) & 1
    assert int(got["scale/seven/n_common"]) == 7
    # the repeated entry adds one term, which the guard drops: the sum, the count and so the scale are those of the list without it
    assert got["scale/twin/scale"].view(np.uint64) == got["scale/n200b_shortcut/scale"].view(np.uint64)
    assert int(got["scale/twin/n_common"]) == int(got["scale/n200b_shortcut/n_common"]) + 1

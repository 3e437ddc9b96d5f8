"""Keypoint selection (clc_detect_set_selection: CLC_SELECT_FIRST / CLC_SELECT_STRONGEST), the part that needs no GPU: the library
exports the two entry points under ABI version 4, a NULL context is CLC_ERR_BAD_ARG, the header declares calls and constants, and
the host-side statement of the rule -- select_strongest below, what tests/test_gpu_detect_select.py expects of the GPU -- agrees
with numpy's stable argsort on score arrays with heavy ties."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cutoff_of(score, cap):
    """(c, above, tied, kept): c = the largest score with #{score >= c} >= cap; above = #{score > c}; tied = #{score == c};
    kept = cap - above of the tied ones survive.  Only defined for len(score) > cap >= 1."""
    score = np.asarray(score).astype(np.int64)
    assert len(score) > cap >= 1
    hist = np.bincount(score, minlength=256)
    ge = np.cumsum(hist[::-1])[::-1]                       # ge[c] = #{score >= c}
    c = int(np.nonzero(ge >= cap)[0].max())
    above = int(ge[c + 1]) if c + 1 < len(ge) else 0
    return c, above, int(hist[c]), cap - above


def select_strongest(score, cap):
    """Indices (ascending: the list keeps its order) of the keypoints CLC_SELECT_STRONGEST keeps from an uncapped detection with
    these scores: all of them when there are no more than cap; otherwise every score above the cutoff and the first cap - #{above}
    of those at the cutoff."""
    score = np.asarray(score).astype(np.int64)
    if len(score) <= cap:
        return np.arange(len(score))
    c, above, _, kept = cutoff_of(score, cap)
    keep = score > c
    keep[np.nonzero(score == c)[0][:kept]] = True
    assert int(keep.sum()) == cap
    return np.nonzero(keep)[0]


def test_library_exports_the_selection_entry_points():
    from coloc_amd import abi
    lib = abi.load_library()
    assert hasattr(lib, "clc_detect_set_selection") and hasattr(lib, "clc_detect_selection")
    assert "clc_detect_set_selection" in abi.EXPORTS and "clc_detect_selection" in abi.EXPORTS
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4           # new entry points only: the version stays


def test_null_context_is_a_bad_argument():
    from coloc_amd import abi
    lib = abi.load_library()
    assert lib.clc_detect_set_selection(None, 1) == abi.CLC_ERR_BAD_ARG == 1
    assert lib.clc_detect_set_selection(None, 0) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_detect_selection(None) < 0


def test_header_declares_calls_and_constants():
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+clc_detect_set_selection\s*\(\s*clc_ctx\s*\*\s*ctx\s*,\s*int\s+mode\s*\)\s*;", code)
    assert re.search(r"\bint\s+clc_detect_selection\s*\(\s*const\s+clc_ctx\s*\*\s*ctx\s*\)\s*;", code)
    assert re.search(r"\bCLC_SELECT_FIRST\s*=\s*0\b", code) and re.search(r"\bCLC_SELECT_STRONGEST\s*=\s*1\b", code)
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code)
    # the version comment names them, the paragraph above clc_detect states both rules
    assert "clc_detect_set_selection" in hdr[:hdr.index("#define CLC_ABI_VERSION")]
    para = hdr[hdr.index("---- detect:"):hdr.index("int clc_detect(")]
    assert "CLC_SELECT_FIRST" in para and "CLC_SELECT_STRONGEST" in para and "GPUDetector.hpp:135,281" in para


def test_python_constants_mirror_the_header():
    import coloc_amd
    assert coloc_amd.SELECT_FIRST == 0 and coloc_amd.SELECT_STRONGEST == 1
    assert hasattr(coloc_amd.Context, "set_keypoint_selection") and isinstance(coloc_amd.Context.keypoint_selection, property)


def test_rule_agrees_with_the_stable_argsort():
    """The two statements of the rule: cutoff + ties in list order, and D[sort(argsort(-score, kind="stable")[:cap])]."""
    rng = np.random.default_rng(5)
    n_cut_through_ties = 0
    for trial in range(300):
        n = int(rng.integers(1, 3000))
        lo = int(rng.integers(1, 250))
        hi = int(rng.integers(lo + 1, min(lo + 1 + (3, 12, 60)[trial % 3], 256) + 1))     # few distinct values: heavy ties
        score = rng.integers(lo, hi, size=n).astype(np.uint8)
        for cap in {1, 2, max(1, n // 7), max(1, n // 2), max(1, n - 1), n, n + 1, 4 * n}:
            want = np.sort(np.argsort(-score.astype(np.int64), kind="stable")[:cap])
            got = select_strongest(score, cap)
            assert np.array_equal(got, want), (trial, n, cap)
            if n > cap:
                c, above, tied, kept = cutoff_of(score, cap)
                assert 1 <= kept <= tied and above + kept == cap and above < cap
                n_cut_through_ties += kept < tied
    assert n_cut_through_ties > 500
    # extremes: all equal; the cutoff at 255; at 1
    assert np.array_equal(select_strongest(np.full(50, 7, np.uint8), 20), np.arange(20))
    assert np.array_equal(select_strongest(np.array([255, 1, 255, 255], np.uint8), 2), [0, 2])
    assert np.array_equal(select_strongest(np.array([1, 2, 1, 1], np.uint8), 3), [0, 1, 2])

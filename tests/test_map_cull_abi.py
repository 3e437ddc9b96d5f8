"""The entries of the map cull (include/coloc_hip.h: clc_map_observe_dev, clc_map_observe_batch_dev, clc_map_cull_dev,
clc_map_cull_rule_default, clc_map_stats_get, clc_cull_map_points) without a GPU: declared, exported and bound under ABI 4, the three
structures' ctypes mirrors have the C compiler's layout, the default rule is the stated one, and the argument rules that need no device work
return the stated codes."""
import ctypes as C
import os
import re
import subprocess

import map_cull_host as ch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_map_observe_dev", "clc_map_observe_batch_dev", "clc_map_cull_dev", "clc_map_cull_rule_default", "clc_map_stats_get",
               "clc_cull_map_points"]


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
        assert getattr(lib, name).argtypes is not None, name + " not bound"
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code)
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    for meth in ("map_observe_dev", "map_observe_batch_dev", "map_cull_dev", "map_stats", "cull_map_points"):
        assert callable(getattr(abi.Context, meth))
    for src in ("coloc_amd/build.py", "CMakeLists.txt"):                      # both builds compile the step's translation unit
        assert "map_cull.hip" in open(os.path.join(ROOT, src)).read(), src
    assert "cull_math.h" in open(os.path.join(ROOT, "coloc_amd", "build.py")).read()


def _probe(tmp_path, ctype, fields):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "coloc_hip.h"', 'int main(void) {', 'printf("%%zu", sizeof(%s));' % ctype]
    src += ['printf(" %%zu", offsetof(%s, %s));' % (ctype, f) for f in fields]
    src += ['printf("\\n");', 'return 0;', '}']
    c = tmp_path / ("probe_%s.c" % ctype)
    c.write_text("\n".join(src))
    exe = tmp_path / ("probe_%s" % ctype)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]


def test_structures_match_the_c_header(tmp_path):
    from coloc_amd import abi
    view = [f for f, _ in abi.ObserveView._fields_]
    assert view == ["n", "d_count", "d_kps", "d_feat", "feat_stride", "cam", "Rt", "d_track", "d_counts"]
    obs = [f for f, _ in abi.MapObserve._fields_]
    assert obs == ["view", "width", "height", "gate", "margin", "after_stream", "epoch", "map_n", "status"]
    cull = [f for f, _ in abi.MapCull._fields_]
    assert cull == ["min_visible", "num", "den", "max_idle", "d_flagged", "d_track", "track_n", "n_lists", "after_stream", "d_remap", "h_remap",
                    "map_n_before", "n_kept", "n_dropped", "n_flagged", "n_ratio", "n_idle", "status"]
    assert abi.MAX_BATCH == 8 and len(abi.MapCull().d_track) == abi.MAX_BATCH == len(abi.MapCull().track_n)
    for ctype, mirror, fields in (("clc_observe_view", abi.ObserveView, view), ("clc_map_observe", abi.MapObserve, obs),
                                  ("clc_map_cull", abi.MapCull, cull)):
        parts = _probe(tmp_path, ctype, fields)
        assert C.sizeof(mirror) == parts[0], ctype
        assert len(parts) == 1 + len(fields)
        for f, off in zip(fields, parts[1:]):
            assert getattr(mirror, f).offset == off, (ctype, f)


def test_default_rule_is_the_stated_one():
    from coloc_amd import abi
    lib = abi.load_library()
    j = abi.MapCull()
    assert lib.clc_map_cull_rule_default(C.byref(j)) == 0
    got = dict(min_visible=j.min_visible, num=j.num, den=j.den, max_idle=j.max_idle)
    assert got == dict(min_visible=8, num=1, den=4, max_idle=0) == abi.CULL_RULE_DEFAULT == ch.cxx_default_rule()
    assert lib.clc_map_cull_rule_default(None) == abi.CLC_ERR_BAD_ARG


def test_argument_rules_that_need_no_device_work():
    """refused without a device: a null context or job, a view count outside 0 .. CLC_MAX_BATCH.  (The jobs' own rules and the context's
    state need a context: tests/test_gpu_map_cull.py.)"""
    from coloc_amd import abi
    lib = abi.load_library()
    BAD = abi.CLC_ERR_BAD_ARG
    o, c = abi.MapObserve(), abi.MapCull()
    assert lib.clc_map_observe_dev(None, C.byref(o)) == BAD
    assert lib.clc_map_observe_dev(None, None) == BAD
    assert lib.clc_map_observe_batch_dev(None, C.byref(o), 1) == BAD
    assert lib.clc_map_observe_batch_dev(None, None, 0) == BAD
    assert lib.clc_map_cull_dev(None, C.byref(c)) == BAD
    assert lib.clc_map_cull_dev(None, None) == BAD
    assert lib.clc_map_stats_get(None, None, None, None, None, None) == BAD
    assert lib.clc_cull_map_points(None, None, 0) == BAD

"""The entries of the one-to-one filter (include/coloc_hip.h: clc_match_unique_dev, clc_match_unique_batch_dev, clc_match_2nn_unique_dev,
clc_match_map_unique_dev, clc_match_map_binned_unique_dev, clc_match_2nn_unique) without a GPU: declared, exported and bound under ABI 4,
the job struct's ctypes mirror has the C compiler's layout, and the argument rules that need no device work return the stated codes."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_match_unique_dev", "clc_match_unique_batch_dev", "clc_match_2nn_unique_dev", "clc_match_map_unique_dev",
               "clc_match_map_binned_unique_dev", "clc_match_2nn_unique"]


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
    for meth in ("match_unique_dev", "match_unique_batch_dev", "match_2nn_unique_dev", "match_map_unique_dev", "match_map_binned_unique_dev",
                 "match_unique"):
        assert callable(getattr(abi.Context, meth))
    for src in ("coloc_amd/build.py", "CMakeLists.txt"):                      # both builds compile the filter's translation unit
        assert "k2nn_unique.hip" in open(os.path.join(ROOT, src)).read(), src


def test_unique_job_matches_the_c_header(tmp_path):
    from coloc_amd import abi
    fields = [f for f, _ in abi.UniqueJob._fields_]
    assert fields == ["d_match", "d_best", "nq", "nt", "d_owner"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "coloc_hip.h"', 'int main(void) {',
           'printf("%zu", sizeof(clc_unique_job));']
    src += ['printf(" %%zu", offsetof(clc_unique_job, %s));' % f for f in fields]
    src += ['printf("\\n");', 'return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    parts = subprocess.check_output([str(exe)], text=True).split()
    assert C.sizeof(abi.UniqueJob) == int(parts[0])
    assert len(parts) == 1 + len(fields)
    for f, off in zip(fields, parts[1:]):
        assert getattr(abi.UniqueJob, f).offset == int(off), f


def test_argument_rules_that_need_no_device_work():
    """refused before anything is allocated or enqueued, without a device: a null context, a null job, a job count outside
    0 .. CLC_MAX_TRACK_PAIRS.  (The jobs' own rules and the context's state need a context: tests/test_gpu_match_unique.py.)"""
    from coloc_amd import abi
    lib = abi.load_library()
    BAD = abi.CLC_ERR_BAD_ARG
    j = abi.UniqueJob(0x1000, 0x2000, 8, 8, 0x3000)
    assert lib.clc_match_unique_dev(None, C.byref(j), None) == BAD
    assert lib.clc_match_unique_dev(None, None, None) == BAD
    assert lib.clc_match_unique_batch_dev(None, C.byref(j), 1, None) == BAD
    assert lib.clc_match_unique_batch_dev(None, None, 0, None) == BAD
    assert lib.clc_match_unique_batch_dev(None, C.byref(j), -1, None) == BAD
    assert lib.clc_match_unique_batch_dev(None, C.byref(j), abi.MAX_TRACK_PAIRS + 1, None) == BAD
    assert lib.clc_match_2nn_unique_dev(None, 0x1000, 8, 0x2000, 8, 40, 0x3000, None, None) == BAD
    assert lib.clc_match_map_unique_dev(None, 0x1000, 8, 40, 0x3000, None, None) == BAD
    assert lib.clc_match_2nn_unique(None, 0x1000, 8, 0x2000, 8, 40, 0x3000, None) == BAD
    g = abi.MapGuidedJob()
    abi._map_guided_fill(g, d_q=0x1000, nq=8, cam=(500.0, 320.0, 240.0, 0, 0, 0), Rt=[1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, 2], radius=4.0, threshold=40,
                         d_match=0x3000, d_feat=0x4000)
    assert lib.clc_match_map_binned_unique_dev(None, C.byref(g), None, None) == BAD
    assert lib.clc_match_map_binned_unique_dev(None, None, None, None) == BAD

"""The guided match entries (include/coloc_hip.h: clc_match_guided_dev, clc_match_guided_batch_dev) without a GPU: declared, exported
and bound under ABI 4, the job struct's ctypes mirror has the C compiler's layout, and the argument rules that need no device work
return the stated codes."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_match_guided_dev", "clc_match_guided_batch_dev"]


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    assert "typedef struct clc_guided_job" in code
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code)
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    for meth in ("match_guided_dev", "match_guided_batch_dev"):
        assert callable(getattr(abi.Context, meth))


def test_guided_job_matches_the_c_header(tmp_path):
    from coloc_amd import abi
    fields = [f for f, _ in abi.GuidedJob._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "coloc_hip.h"', 'int main(void) {',
           'printf("%zu", sizeof(clc_guided_job));']
    src += ['printf(" %%zu", offsetof(clc_guided_job, %s));' % f for f in fields]
    src += ['printf("\\n");', 'return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    parts = subprocess.check_output([str(exe)], text=True).split()
    assert C.sizeof(abi.GuidedJob) == int(parts[0])
    assert len(parts) == 1 + len(fields)
    for f, off in zip(fields, parts[1:]):
        assert getattr(abi.GuidedJob, f).offset == int(off), f


def test_argument_rules_that_need_no_device_work():
    """refused before anything is enqueued, without a device: a null context, a null job, a job count outside 0 .. CLC_MAX_TRACK_PAIRS.
    (The job's own rules -- both or neither 2-D form of a camera, a misaligned pointer, a non-positive focal, a bad band, a context
    without matcher options -- need a context: tests/test_gpu_guided_match.py::test_edges.)"""
    from coloc_amd import abi
    lib = abi.load_library()
    BAD = abi.CLC_ERR_BAD_ARG
    cam = (500.0, 320.0, 240.0, 0, 0, 0)
    j = abi.GuidedJob()
    abi._guided_fill(j, d_q=0x1000, nq=8, d_t=0x2000, nt=8, cam_a=cam, cam_b=cam, F=[0, 0, 0, 0, 0, -1, 0, 1, 0], band=2.0, threshold=40,
                     d_match=0x3000, d_feat_a=0x4000, d_feat_b=0x5000)
    assert list(j.F) == [0, 0, 0, 0, 0, -1, 0, 1, 0] and j.band == 2.0 and j.threshold == 40
    assert lib.clc_match_guided_dev(None, C.byref(j), None) == BAD
    assert lib.clc_match_guided_dev(None, None, None) == BAD
    assert lib.clc_match_guided_batch_dev(None, C.byref(j), 1, None) == BAD
    assert lib.clc_match_guided_batch_dev(None, None, 0, None) == BAD
    assert lib.clc_match_guided_batch_dev(None, C.byref(j), -1, None) == BAD
    assert lib.clc_match_guided_batch_dev(None, C.byref(j), abi.MAX_TRACK_PAIRS + 1, None) == BAD

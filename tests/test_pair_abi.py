"""The device-side two-view correspondences (include/coloc_hip.h: clc_pair_build_dev, clc_pair_filter_dev, clc_pair_filter_batch_dev)
without a GPU: the entries are declared, exported and bound under ABI 4, the job struct's ctypes mirror has the C compiler's layout, and
the argument rules that need no device work return the stated codes."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_pair_build_dev", "clc_pair_filter_dev", "clc_pair_filter_batch_dev"]


def test_entries_are_declared_exported_and_bound():
    import coloc_amd
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    assert "typedef struct clc_pair_job" in code
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code)
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    for meth in ("pair_build_dev", "pair_filter_dev"):
        assert callable(getattr(abi.Context, meth))
    assert callable(abi.pair_filter_batch_dev) and coloc_amd.pair_filter_batch_dev is abi.pair_filter_batch_dev


def test_pair_job_matches_the_c_header(tmp_path):
    from coloc_amd import abi
    fields = [f for f, _ in abi.PairJob._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "coloc_hip.h"', 'int main(void) {',
           'printf("%zu", sizeof(clc_pair_job));']
    src += ['printf(" %%zu", offsetof(clc_pair_job, %s));' % f for f in fields]
    src += ['printf("\\n");', 'return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    parts = subprocess.check_output([str(exe)], text=True).split()
    assert C.sizeof(abi.PairJob) == int(parts[0])
    assert len(parts) == 1 + len(fields)
    for f, off in zip(fields, parts[1:]):
        assert getattr(abi.PairJob, f).offset == int(off), f


def _job(abi, **over):
    """a job whose pointers are never dereferenced by the checks under test (aligned, non-null, not device memory)"""
    j = abi.PairJob()
    abi._pair_fill(j, None, outputs=False, **dict(dict(d_match=0x1000, nq=8, nt=8, cam_a=(500.0, 320.0, 240.0, 0, 0, 0),
                                                       cam_b=(500.0, 320.0, 240.0, 0, 0, 0), d_feat_a=0x2000, d_feat_b=0x3000,
                                                       img_wh=(640, 480)), **over))
    return j


def test_argument_rules_that_need_no_device_work():
    """refused before anything is enqueued, without a device: a null context or job, an unknown model, a negative job count.  (The
    job's own rules -- both or neither 2-D form of a camera, a misaligned pointer, a non-positive focal -- need a context to tell them
    from these; tests/test_gpu_pair_filter.py::test_edges holds them to CLC_ERR_BAD_ARG.)"""
    from coloc_amd import abi
    lib = abi.load_library()
    BAD = abi.CLC_ERR_BAD_ARG
    job = _job(abi)
    for model in (ord("E"), ord("F"), ord("H"), ord("X")):
        assert lib.clc_pair_filter_dev(None, model, C.byref(job)) == BAD
    assert lib.clc_pair_filter_dev(None, ord("E"), None) == BAD
    assert lib.clc_pair_build_dev(None, C.byref(job), None, None, None, None, None, None) == BAD
    assert lib.clc_pair_filter_batch_dev(None, ord("E"), C.byref(job), 1) == BAD
    assert lib.clc_pair_filter_batch_dev(None, ord("E"), None, 1) == BAD
    null_ctx = (C.c_void_p * 1)(None)
    assert lib.clc_pair_filter_batch_dev(null_ctx, ord("F"), C.byref(job), 1) == BAD
    assert lib.clc_pair_filter_batch_dev(None, ord("H"), None, 0) == abi.CLC_OK
    assert lib.clc_pair_filter_batch_dev(None, ord("X"), None, 0) == BAD            # an unknown model, even with nothing to do
    assert lib.clc_pair_filter_batch_dev(None, ord("E"), None, -1) == BAD

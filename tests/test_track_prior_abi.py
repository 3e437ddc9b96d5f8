"""The pose from the prediction (include/coloc_hip.h: clc_track_prior_dev, clc_track_prior_batch_dev, clc_pnp_refine_prior) without a GPU:
the entries are declared, exported and bound under ABI 4, the job struct's ctypes mirror has the C compiler's layout, and NULL arguments
are refused."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_track_prior_dev", "clc_track_prior_batch_dev", "clc_pnp_refine_prior"]


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    assert "typedef struct clc_track_prior_job" in code
    assert re.search(r"#define\s+CLC_TRACK_PRIOR_OK\s+0\b", code) and re.search(r"#define\s+CLC_TRACK_PRIOR_FEW\s+1\b", code)
    assert (abi.TRACK_PRIOR_OK, abi.TRACK_PRIOR_FEW) == (0, 1)
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    assert "THE RULE" in hdr[hdr.index("a tracked frame's pose from the prediction"):hdr.index("typedef struct clc_track_prior_job")]
    for meth in ("track_prior_dev", "pnp_refine_prior"):
        assert callable(getattr(abi.Context, meth))
    assert callable(abi.track_prior_batch_dev)


def test_null_arguments_are_bad_arguments():
    from coloc_amd import abi
    lib = abi.load_library()
    job = abi.TrackPriorJob()
    assert lib.clc_track_prior_dev(None, C.byref(job)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_prior_dev(None, None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_prior_batch_dev(None, C.byref(job), 1) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_prior_batch_dev(None, None, 1) == abi.CLC_ERR_BAD_ARG
    null_ctx = (C.c_void_p * 1)(None)
    assert lib.clc_track_prior_batch_dev(null_ctx, C.byref(job), 1) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_prior_batch_dev(None, None, 0) == abi.CLC_OK
    assert lib.clc_track_prior_batch_dev(None, None, -1) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_prior_batch_dev(null_ctx, C.byref(job), abi.MAX_BATCH + 1) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_pnp_refine_prior(None, None, None, 0, None, None, 3.0, 16.0, 0, 0, 0, *([None] * 9)) == abi.CLC_ERR_BAD_ARG


def test_track_prior_job_matches_the_c_header(tmp_path):
    from coloc_amd import abi
    fields = [f for f, _ in abi.TrackPriorJob._fields_]
    # the frame is exactly clc_track_job's: the same names at the same offsets
    for f in ("d_match", "nq", "d_count", "d_kps", "d_feat", "feat_stride", "cam", "after_stream"):
        assert getattr(abi.TrackPriorJob, f).offset == getattr(abi.TrackJob, f).offset, f
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "coloc_hip.h"', 'int main(void) {',
           'printf("%zu", sizeof(clc_track_prior_job));']
    for f in fields:
        src.append('printf(" %%zu", offsetof(clc_track_prior_job, %s));' % f)
    src += ['printf("\\n");', 'return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    parts = subprocess.check_output([str(exe)], text=True).split()
    assert C.sizeof(abi.TrackPriorJob) == int(parts[0])
    assert len(parts) == len(fields) + 1
    for f, off in zip(fields, parts[1:]):
        assert getattr(abi.TrackPriorJob, f).offset == int(off), f

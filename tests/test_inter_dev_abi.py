"""The inter-camera step from device memory (include/coloc_hip.h: clc_inter_pose_dev, clc_inter_pose_batch_dev, clc_inter_front_dev)
without a GPU: the entries are declared, exported and bound under ABI 4, the job struct's ctypes mirror has the C compiler's layout, and
the argument rules that need no device work return the stated codes."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_inter_pose_dev", "clc_inter_pose_batch_dev", "clc_inter_front_dev"]


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
    assert "typedef struct clc_inter_dev_job" in code
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code)
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    for meth in ("inter_pose_dev", "inter_front_dev"):
        assert callable(getattr(abi.Context, meth))
    assert callable(abi.inter_pose_batch_dev) and coloc_amd.inter_pose_batch_dev is abi.inter_pose_batch_dev


def _flat(struct, prefix=""):
    """(C member path, ctypes offset) of every leaf field, nested structs included"""
    out = []
    for name, typ in struct._fields_:
        off = getattr(struct, name).offset
        if isinstance(typ, type) and issubclass(typ, C.Structure):
            out += [(prefix + name + "." + n, off + o) for n, o in _flat(typ)]
        else:
            out.append((prefix + name, off))
    return out


def test_inter_dev_job_matches_the_c_header(tmp_path):
    from coloc_amd import abi
    fields = _flat(abi.InterDevJob)
    assert ("pair.cam_b.k3" in dict(fields)) and ("n_map_matches" in dict(fields))
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "coloc_hip.h"', 'int main(void) {',
           'printf("%zu", sizeof(clc_inter_dev_job));']
    src += ['printf(" %%zu", offsetof(clc_inter_dev_job, %s));' % f for f, _ in fields]
    src += ['printf("\\n");', 'return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    parts = subprocess.check_output([str(exe)], text=True).split()
    assert C.sizeof(abi.InterDevJob) == int(parts[0])
    assert len(parts) == 1 + len(fields)
    for (f, off), want in zip(fields, parts[1:]):
        assert off == int(want), f


def test_argument_rules_that_need_no_device_work():
    """refused before anything is enqueued, without a device: a null context or job, a negative job count.  (The job's own rules --
    both or neither source of common features, a misaligned pointer, no map points -- need a context:
    tests/test_gpu_inter_pose_dev.py::test_stages holds them to CLC_ERR_BAD_ARG / CLC_ERR_STATE.)"""
    from coloc_amd import abi
    lib = abi.load_library()
    BAD = abi.CLC_ERR_BAD_ARG
    job = abi.InterDevJob()
    assert lib.clc_inter_pose_dev(None, C.byref(job)) == BAD
    assert lib.clc_inter_pose_dev(None, None) == BAD
    assert lib.clc_inter_pose_batch_dev(None, C.byref(job), 1) == BAD
    assert lib.clc_inter_pose_batch_dev(None, None, 1) == BAD
    null_ctx = (C.c_void_p * 1)(None)
    assert lib.clc_inter_pose_batch_dev(null_ctx, C.byref(job), 1) == BAD
    assert lib.clc_inter_pose_batch_dev(None, None, 0) == abi.CLC_OK
    assert lib.clc_inter_pose_batch_dev(None, None, -1) == BAD
    assert lib.clc_inter_front_dev(None, None, None, 0, None, 0, None, None, None, None, None, None, None, None, None, None) == BAD

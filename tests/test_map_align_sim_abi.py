"""The map replaced under an a-contrario similarity (include/coloc_hip.h: clc_sim3_acransac, clc_sim3_minimal, clc_map_align_sim_dev,
clc_map_update_sim_batch_dev) without a GPU: the entries are declared, exported and bound under ABI 4, the ctypes mirror of
clc_map_align_sim has the C compiler's layout, NULL arguments are refused.  (What a context refuses needs a GPU:
tests/test_gpu_map_align_sim.py.)"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_sim3_acransac", "clc_sim3_minimal", "clc_map_align_sim_dev", "clc_map_update_sim_batch_dev"]


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    assert "typedef struct clc_map_align_sim" in code
    assert re.search(r"CLC_MAP_SIM_OK\s*=\s*0\b", code) and re.search(r"CLC_MAP_SIM_NO_MODEL\s*=\s*1\b", code)
    assert re.search(r"CLC_SIM_APPLY_SCALE\s*=\s*0\b", code) and re.search(r"CLC_SIM_APPLY_FULL\s*=\s*1\b", code)
    assert (abi.MAP_SIM_OK, abi.MAP_SIM_NO_MODEL, abi.SIM_APPLY_SCALE, abi.SIM_APPLY_FULL) == (0, 1, 0, 1)
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code)                       # new entry points only: the version stays
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    assert callable(abi.Context.sim3_acransac) and callable(abi.Context.sim3_minimal)
    assert callable(abi.Context.map_align_sim_dev) and callable(abi.map_update_sim_batch_dev)


def test_the_arithmetic_header_is_listed_in_the_build():
    from coloc_amd import build
    assert "sim3_math.h" in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "sim3_math.h"))


def test_null_arguments_are_bad_arguments():
    from coloc_amd import abi
    lib = abi.load_library()
    a, mj, pj, g, b = abi.MapAlignSim(), abi.MapJob(), abi.PairJob(), abi.MapGrow(), abi.MapBa()
    assert lib.clc_map_align_sim_dev(None, C.byref(a)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_align_sim_dev(None, None) == abi.CLC_ERR_BAD_ARG
    null_ctx = (C.c_void_p * 1)(None)
    upd = lib.clc_map_update_sim_batch_dev
    assert upd(None, C.byref(pj), 1, C.byref(mj), C.byref(a), None, None) == abi.CLC_ERR_BAD_ARG
    assert upd(null_ctx, None, 1, C.byref(mj), C.byref(a), None, None) == abi.CLC_ERR_BAD_ARG
    assert upd(null_ctx, C.byref(pj), 1, None, C.byref(a), None, None) == abi.CLC_ERR_BAD_ARG
    assert upd(null_ctx, C.byref(pj), 1, C.byref(mj), None, None, None) == abi.CLC_ERR_BAD_ARG
    assert upd(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(a), None, None) == abi.CLC_ERR_BAD_ARG          # a NULL context in the list
    assert upd(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(a), C.byref(g), None) == abi.CLC_ERR_BAD_ARG
    assert upd(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(a), None, C.byref(b)) == abi.CLC_ERR_BAD_ARG    # ba needs grow
    assert upd(null_ctx, C.byref(pj), 0, C.byref(mj), C.byref(a), None, None) == abi.CLC_ERR_BAD_ARG          # no pair at all
    # a refused call still says that nothing was transformed
    assert a.status == abi.MAP_SIM_NO_MODEL and a.s == 1.0 and list(a.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(a.t) == [0, 0, 0]
    # the host-pointer entries
    s = C.c_double(5.0)
    none = [None] * 11
    assert lib.clc_sim3_acransac(None, None, None, 10, 256, 1, float("inf"), C.byref(s), *none) == abi.CLC_ERR_BAD_ARG
    assert s.value == 1.0                                                         # identity also from a refused call
    assert lib.clc_sim3_minimal(None, None, None, 10, None, 1, None) == abi.CLC_ERR_BAD_ARG


def test_sim_struct_matches_the_c_header(tmp_path):
    from coloc_amd import abi
    probes = {"clc_map_align_sim": abi.MapAlignSim}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "coloc_hip.h"', 'int main(void) {']
    for name, cls in probes.items():
        src.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            src.append('printf(" %%zu", offsetof(%s, %s));' % (name, f))
        src.append('printf("\\n");')
    src += ['return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    for line in subprocess.check_output([str(exe)], text=True).strip().splitlines():
        parts = line.split()
        cls = probes[parts[0]]
        assert C.sizeof(cls) == int(parts[1]), parts[0]
        assert len(parts) - 2 == len(cls._fields_)
        for (f, _), off in zip(cls._fields_, parts[2:]):
            assert getattr(cls, f).offset == int(off), (parts[0], f)

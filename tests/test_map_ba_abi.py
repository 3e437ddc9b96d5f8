"""The bundle adjustment's entries (include/coloc_hip.h: clc_ba_dev, clc_map_build_grow_ba_dev, clc_map_init_grow_ba_batch_dev,
clc_map_update_grow_ba_batch_dev) without a GPU: declared, exported and bound under ABI 4, the ctypes mirrors of clc_map_ba and clc_ba_job
have the C compiler's layout, NULL arguments and negative counts are refused."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_ba_dev", "clc_map_build_grow_ba_dev", "clc_map_init_grow_ba_batch_dev", "clc_map_update_grow_ba_batch_dev"]


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    assert "typedef struct clc_map_ba" in code and "typedef struct clc_ba_job" in code
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code) and lib.clc_abi_version() == abi.ABI_VERSION == 4
    m = re.search(r"enum\s*\{\s*CLC_BA_OK\s*=\s*(\d+),\s*CLC_BA_MAX_ITERATIONS\s*=\s*(\d+),\s*CLC_BA_STALLED\s*=\s*(\d+)\s*,\s*CLC_BA_BAD_START\s*=\s*(\d+),"
                  r"\s*CLC_BA_EMPTY\s*=\s*(\d+)", code)
    assert [int(v) for v in m.groups()] == [abi.BA_OK, abi.BA_MAX_ITERATIONS, abi.BA_STALLED, abi.BA_BAD_START, abi.BA_EMPTY]
    for meth in ("ba_dev", "map_build_grow_ba_dev"):
        assert callable(getattr(abi.Context, meth))
    assert callable(abi.map_init_grow_ba_batch_dev) and callable(abi.map_update_grow_ba_batch_dev)


def test_the_sources_are_listed_in_both_builds():
    from coloc_amd import build
    assert "map_ba.hip" in build.SOURCES and "ba_math.h" in build.HEADERS
    assert "coloc_amd/csrc/map_ba.hip" in open(os.path.join(ROOT, "CMakeLists.txt")).read()


def test_null_arguments_and_negative_counts_are_bad_arguments():
    from coloc_amd import abi
    lib = abi.load_library()
    mj, pj, g, al, b, bj = abi.MapJob(), abi.PairJob(), abi.MapGrow(), abi.MapAlign(), abi.MapBa(), abi.BaJob()
    assert lib.clc_ba_dev(None, None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_ba_dev(None, C.byref(bj)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_build_grow_ba_dev(None, C.byref(mj), C.byref(g), C.byref(b)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_build_grow_ba_dev(None, None, None, None) == abi.CLC_ERR_BAD_ARG
    null_ctx = (C.c_void_p * 1)(None)
    assert lib.clc_map_init_grow_ba_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(g), None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_init_grow_ba_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), None, C.byref(b)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_init_grow_ba_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(g), C.byref(b)) == abi.CLC_ERR_BAD_ARG      # a NULL context
    assert lib.clc_map_update_grow_ba_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(al), C.byref(g), None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_grow_ba_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), None, C.byref(g), C.byref(b)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_grow_ba_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(al), C.byref(g), C.byref(b)) == abi.CLC_ERR_BAD_ARG
    for field, value in (("max_iterations", -1), ("function_tolerance", -1e-3), ("function_tolerance", float("nan"))):
        bad = abi.MapBa()
        setattr(bad, field, value)
        assert lib.clc_map_init_grow_ba_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(g), C.byref(bad)) == abi.CLC_ERR_BAD_ARG
        assert lib.clc_map_update_grow_ba_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(al), C.byref(g), C.byref(bad)) == abi.CLC_ERR_BAD_ARG


def test_the_structs_match_the_c_header(tmp_path):
    from coloc_amd import abi
    probes = {"clc_map_ba": abi.MapBa, "clc_ba_job": abi.BaJob}
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
        for (f, _), off in zip(cls._fields_, parts[2:]):
            assert getattr(cls, f).offset == int(off), (parts[0], f)

"""The map replaced at the old map's scale (include/coloc_hip.h: clc_map_align_dev, clc_map_update_batch_dev) without a GPU: the entries
are declared, exported and bound under ABI 4, the ctypes mirror of clc_map_align has the C compiler's layout, NULL arguments are refused.
(What a context refuses -- no previous map, capacity, misaligned pointers -- needs a context, so a GPU: tests/test_gpu_map_update.py.)"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_map_align_dev", "clc_map_update_batch_dev"]


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    assert "typedef struct clc_map_align" in code
    assert re.search(r"CLC_MAP_ALIGN_OK\s*=\s*0\b", code) and re.search(r"CLC_MAP_ALIGN_NO_SCALE\s*=\s*1\b", code)
    assert (abi.MAP_ALIGN_OK, abi.MAP_ALIGN_NO_SCALE) == (0, 1)
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code)
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    assert callable(abi.Context.map_align_dev) and callable(abi.map_update_batch_dev)


def test_the_sources_are_listed_in_both_builds():
    from coloc_amd import build
    assert "map_update.hip" in build.SOURCES and "map_build.hip" in build.SOURCES
    assert "coloc_amd/csrc/map_update.hip" in open(os.path.join(ROOT, "CMakeLists.txt")).read()


def test_null_arguments_are_bad_arguments():
    from coloc_amd import abi
    lib = abi.load_library()
    al, mj, pj = abi.MapAlign(), abi.MapJob(), abi.PairJob()
    assert lib.clc_map_align_dev(None, C.byref(al)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_align_dev(None, None) == abi.CLC_ERR_BAD_ARG
    null_ctx = (C.c_void_p * 1)(None)
    assert lib.clc_map_update_batch_dev(None, C.byref(pj), 1, C.byref(mj), C.byref(al)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_batch_dev(null_ctx, None, 1, C.byref(mj), C.byref(al)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_batch_dev(null_ctx, C.byref(pj), 1, None, C.byref(al)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(al)) == abi.CLC_ERR_BAD_ARG      # a NULL context in the list
    assert lib.clc_map_update_batch_dev(null_ctx, C.byref(pj), 0, C.byref(mj), C.byref(al)) == abi.CLC_ERR_BAD_ARG      # no pair at all
    assert lib.clc_map_update_batch_dev(null_ctx, C.byref(pj), abi.MAX_TRACK_PAIRS + 1, C.byref(mj), C.byref(al)) == abi.CLC_ERR_BAD_ARG
    # a refused call still says that nothing was scaled
    assert al.status == abi.MAP_ALIGN_NO_SCALE and al.scale == 1.0


def test_align_struct_matches_the_c_header(tmp_path):
    from coloc_amd import abi
    probes = {"clc_map_align": abi.MapAlign}
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

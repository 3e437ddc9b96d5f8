"""The map grown past the seed pair (include/coloc_hip.h: clc_map_build_grow_dev, clc_map_init_grow_batch_dev,
clc_map_update_grow_batch_dev, clc_map_resect_build_dev) without a GPU: the entries are declared, exported and bound under ABI 4, the
ctypes mirror of clc_map_grow has the C compiler's layout, NULL arguments and a bad camera are refused."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_map_build_grow_dev", "clc_map_init_grow_batch_dev", "clc_map_update_grow_batch_dev", "clc_map_resect_build_dev"]


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    assert "typedef struct clc_map_grow" in code
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code) and lib.clc_abi_version() == abi.ABI_VERSION == 4
    m = re.search(r"enum\s*\{\s*CLC_GROW_OK\s*=\s*(\d+),\s*CLC_GROW_NO_TRACKS\s*=\s*(\d+),\s*CLC_GROW_NO_POSE\s*=\s*(\d+),\s*CLC_GROW_CAPACITY\s*=\s*(\d+)", code)
    assert [int(v) for v in m.groups()] == [abi.GROW_OK, abi.GROW_NO_TRACKS, abi.GROW_NO_POSE, abi.GROW_CAPACITY]
    for meth in ("map_build_grow_dev", "map_resect_build_dev"):
        assert callable(getattr(abi.Context, meth))
    assert callable(abi.map_init_grow_batch_dev) and callable(abi.map_update_grow_batch_dev)


def test_the_sources_are_listed_in_both_builds():
    from coloc_amd import build
    assert "map_grow.hip" in build.SOURCES and "map_math.h" in build.HEADERS
    assert "coloc_amd/csrc/map_grow.hip" in open(os.path.join(ROOT, "CMakeLists.txt")).read()


def test_null_arguments_and_a_bad_camera_are_bad_arguments():
    from coloc_amd import abi
    lib = abi.load_library()
    mj, pj, g, al = abi.MapJob(), abi.PairJob(), abi.MapGrow(), abi.MapAlign()
    assert lib.clc_map_build_grow_dev(None, C.byref(mj), C.byref(g)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_build_grow_dev(None, None, C.byref(g)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_build_grow_dev(None, None, None) == abi.CLC_ERR_BAD_ARG
    null_ctx = (C.c_void_p * 1)(None)
    assert lib.clc_map_init_grow_batch_dev(null_ctx, C.byref(pj), 1, None, C.byref(g)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_init_grow_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_init_grow_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(g)) == abi.CLC_ERR_BAD_ARG      # a NULL context in the list
    assert lib.clc_map_init_grow_batch_dev(None, C.byref(pj), 1, C.byref(mj), C.byref(g)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_grow_batch_dev(null_ctx, C.byref(pj), 1, None, C.byref(al), C.byref(g)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_grow_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), None, C.byref(g)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_grow_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(al), None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_update_grow_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj), C.byref(al), C.byref(g)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_resect_build_dev(None, None, 0, None, None, None, None, None, None) == abi.CLC_ERR_BAD_ARG
    mj.tracks.n_cams = 3
    for camera in (-1, 3, 1 << 20):
        assert lib.clc_map_resect_build_dev(None, C.byref(mj), camera, None, None, None, None, None, None) == abi.CLC_ERR_BAD_ARG


def test_the_struct_matches_the_c_header(tmp_path):
    from coloc_amd import abi
    probes = {"clc_map_grow": abi.MapGrow}
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

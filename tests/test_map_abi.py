"""The map built on the device (include/coloc_hip.h: clc_tracks_build_dev, clc_map_build_dev, clc_map_init_batch_dev) without a GPU: the
entries are declared, exported and bound under ABI 4, the ctypes mirrors of the job structs have the C compiler's layout, NULL arguments are
refused.  (What a context refuses -- pairs with cam_a >= cam_b, misaligned pointers, both or neither 2-D side -- needs a context, so a
GPU: tests/test_gpu_map_build.py.)"""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_tracks_build_dev", "clc_map_build_dev", "clc_map_init_batch_dev"]


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    for t in ("clc_tracks_pair", "clc_tracks_job", "clc_map_camera", "clc_map_job"):
        assert "typedef struct %s" % t in code
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code)
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    assert int(re.search(r"#define\s+CLC_MAX_TRACK_PAIRS\s+(\d+)", code).group(1)) == abi.MAX_TRACK_PAIRS
    assert int(re.search(r"#define\s+CLC_MAX_BATCH\s+(\d+)", code).group(1)) == abi.MAX_BATCH
    for meth in ("tracks_build_dev", "map_build_dev"):
        assert callable(getattr(abi.Context, meth))
    assert callable(abi.map_init_batch_dev) and callable(abi.seed_poses) and callable(abi.tracks_capacity)


def test_the_sources_are_listed_in_both_builds():
    from coloc_amd import build
    assert "map_build.hip" in build.SOURCES and "map_math.h" in build.HEADERS
    assert "coloc_amd/csrc/map_build.hip" in open(os.path.join(ROOT, "CMakeLists.txt")).read()


def test_null_arguments_are_bad_arguments():
    from coloc_amd import abi
    lib = abi.load_library()
    tj, mj, pj = abi.TracksJob(), abi.MapJob(), abi.PairJob()
    assert lib.clc_tracks_build_dev(None, C.byref(tj), None, None, None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_tracks_build_dev(None, None, None, None, None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_build_dev(None, C.byref(mj)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_build_dev(None, None) == abi.CLC_ERR_BAD_ARG
    null_ctx = (C.c_void_p * 1)(None)
    assert lib.clc_map_init_batch_dev(None, C.byref(pj), 1, C.byref(mj)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_init_batch_dev(null_ctx, None, 1, C.byref(mj)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_init_batch_dev(null_ctx, C.byref(pj), 1, None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_map_init_batch_dev(null_ctx, C.byref(pj), 1, C.byref(mj)) == abi.CLC_ERR_BAD_ARG          # a NULL context in the list
    assert lib.clc_map_init_batch_dev(null_ctx, C.byref(pj), 0, C.byref(mj)) == abi.CLC_ERR_BAD_ARG          # no pair at all
    assert lib.clc_map_init_batch_dev(null_ctx, C.byref(pj), abi.MAX_TRACK_PAIRS + 1, C.byref(mj)) == abi.CLC_ERR_BAD_ARG


def test_job_structs_match_the_c_header(tmp_path):
    from coloc_amd import abi
    probes = {"clc_tracks_pair": abi.TracksPair, "clc_tracks_job": abi.TracksJob, "clc_map_camera": abi.MapCamera, "clc_map_job": abi.MapJob}
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


def test_tracks_capacity_is_the_headers_formula():
    from coloc_amd import abi
    assert abi.tracks_capacity([300, 300, 300], [dict(n=100), dict(n=50)]) == 150
    assert abi.tracks_capacity([10, 11], [dict(n=100)]) == 10
    assert abi.tracks_capacity([10, 11], []) == 0

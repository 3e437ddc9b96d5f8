"""The entries of the map extension (include/coloc_hip.h: clc_map_extend_dev, clc_map_extend_batch_dev, clc_fundamental_from_poses,
clc_append_map_points) without a GPU: declared, exported and bound under ABI 4, the two structures' ctypes mirrors have the C compiler's
layout, clc_fundamental_from_poses is the g++ statement bit for bit, and the argument rules that need no device work return the stated
codes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import map_extend_host as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_map_extend_dev", "clc_map_extend_batch_dev", "clc_fundamental_from_poses", "clc_append_map_points"]


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
    for meth in ("extend_map", "extend_map_batch", "fundamental_from_poses", "append_map_points"):
        assert callable(getattr(abi.Context, meth))
    for src in ("coloc_amd/build.py", "CMakeLists.txt"):                      # both builds compile the step's translation unit
        assert "map_extend.hip" in open(os.path.join(ROOT, src)).read(), src
    assert "extend_math.h" in open(os.path.join(ROOT, "coloc_amd", "build.py")).read()


def _probe(tmp_path, ctype, fields):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "coloc_hip.h"', 'int main(void) {', 'printf("%%zu", sizeof(%s));' % ctype]
    src += ['printf(" %%zu", offsetof(%s, %s));' % (ctype, f) for f in fields]
    src += ['printf("\\n");', 'return 0;', '}']
    c = tmp_path / ("probe_%s.c" % ctype)
    c.write_text("\n".join(src))
    exe = tmp_path / ("probe_%s" % ctype)
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]


def test_structures_match_the_c_header(tmp_path):
    from coloc_amd import abi
    view = [f for f, _ in abi.ExtendView._fields_]
    assert view == ["d_desc", "n", "d_count", "d_kps", "d_feat", "feat_stride", "cam", "Rt", "d_track"]
    job = [f for f, _ in abi.MapExtend._fields_]
    assert job == ["a", "b", "band", "threshold", "max_distance", "update_tracks", "after_stream", "d_new_q", "d_new_t", "new_q", "new_t", "X", "F",
                   "map_n_before", "n_guided", "n_added", "n_dropped", "status"]
    for ctype, mirror, fields in (("clc_extend_view", abi.ExtendView, view), ("clc_map_extend", abi.MapExtend, job)):
        parts = _probe(tmp_path, ctype, fields)
        assert C.sizeof(mirror) == parts[0], ctype
        assert len(parts) == 1 + len(fields)
        for f, off in zip(fields, parts[1:]):
            assert getattr(mirror, f).offset == off, (ctype, f)


def test_fundamental_from_poses_is_the_statement_bit_for_bit():
    from coloc_amd import abi
    rng = np.random.RandomState(17)
    cases = [(mh.CAM, mh.pose(0.0, (0, 0, 0)), mh.CAM_K1, mh.pose(0.03, (0.6, 0, 0))), (mh.CAM, mh.pose(0.2, (0, 0, 0)), mh.CAM, mh.pose(0.0, (0, 0, 0)))]
    for _ in range(50):
        Ra, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Rb, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        cases.append(((rng.uniform(300, 900), rng.uniform(200, 500), rng.uniform(150, 400)), np.column_stack([Ra, rng.normal(size=3)]),
                      (rng.uniform(300, 900), rng.uniform(200, 500), rng.uniform(150, 400)), np.column_stack([Rb, rng.normal(size=3)])))
    for cam_a, Rt_a, cam_b, Rt_b in cases:
        got, want = abi.fundamental_from_poses(cam_a, Rt_a, cam_b, Rt_b), mh.fundamental(cam_a, Rt_a, cam_b, Rt_b)
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64))
    assert np.array_equal(abi.Context.fundamental_from_poses(*cases[0]), mh.fundamental(*cases[0]))


def test_argument_rules_that_need_no_device_work():
    """refused without a device: a null context or job, a job count outside 0 .. CLC_MAX_TRACK_PAIRS, null pointers and a non-positive focal
    of clc_fundamental_from_poses.  (The jobs' own rules and the context's state need a context: tests/test_gpu_map_extend.py.)"""
    from coloc_amd import abi
    lib = abi.load_library()
    BAD = abi.CLC_ERR_BAD_ARG
    j = abi.MapExtend()
    assert lib.clc_map_extend_dev(None, C.byref(j)) == BAD
    assert lib.clc_map_extend_dev(None, None) == BAD
    assert lib.clc_map_extend_batch_dev(None, C.byref(j), 1) == BAD
    assert lib.clc_map_extend_batch_dev(None, None, 0) == BAD
    assert lib.clc_append_map_points(None, None, 0) == BAD
    cam, bad_cam = abi.CameraK3(512.0, 320.0, 240.0, 0.0, 0.0, 0.0), abi.CameraK3(0.0, 320.0, 240.0, 0.0, 0.0, 0.0)
    Rt, F = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), (C.c_double * 9)()
    assert lib.clc_fundamental_from_poses(C.byref(cam), Rt, C.byref(cam), Rt, F) == 0
    assert lib.clc_fundamental_from_poses(None, Rt, C.byref(cam), Rt, F) == BAD
    assert lib.clc_fundamental_from_poses(C.byref(cam), None, C.byref(cam), Rt, F) == BAD
    assert lib.clc_fundamental_from_poses(C.byref(cam), Rt, C.byref(cam), Rt, None) == BAD
    assert lib.clc_fundamental_from_poses(C.byref(bad_cam), Rt, C.byref(cam), Rt, F) == BAD
    assert lib.clc_fundamental_from_poses(C.byref(cam), Rt, C.byref(bad_cam), Rt, F) == BAD

"""The device-side 2D-3D tracks (include/coloc_hip.h: clc_set_map_points, clc_track_build_dev, clc_track_localize*_dev) without a GPU: the
entries are declared, exported and bound under ABI 4, the job struct's ctypes mirror has the C compiler's layout, NULL arguments are refused
-- and tests/track_host.py, the yardstick the GPU tests hold the track kernel to, has Pinhole_Intrinsic_Radial_K3::get_ud_pixel's bits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import track_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_set_map_points", "clc_track_build_dev", "clc_track_localize_dev", "clc_track_localize_batch_dev"]


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    assert "typedef struct clc_track_job" in code and "typedef struct clc_camera_k3" in code
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    for meth in ("set_map_points", "track_localize_dev", "track_build_dev"):
        assert callable(getattr(abi.Context, meth))
    assert callable(abi.track_localize_batch_dev)


def test_null_arguments_are_bad_arguments():
    from coloc_amd import abi
    lib = abi.load_library()
    job = abi.TrackJob()
    X = np.zeros(3)
    assert lib.clc_set_map_points(None, abi._p(X), 1) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_localize_dev(None, C.byref(job)) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_localize_dev(None, None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_build_dev(None, C.byref(job), None, None, None, None, None, None) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_localize_batch_dev(None, C.byref(job), 1) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_localize_batch_dev(None, None, 1) == abi.CLC_ERR_BAD_ARG
    null_ctx = (C.c_void_p * 1)(None)
    assert lib.clc_track_localize_batch_dev(null_ctx, C.byref(job), 1) == abi.CLC_ERR_BAD_ARG
    assert lib.clc_track_localize_batch_dev(None, None, 0) == abi.CLC_OK


def test_track_job_matches_the_c_header(tmp_path):
    from coloc_amd import abi
    probes = {"clc_camera_k3": (abi.CameraK3, ["focal", "ppx", "ppy", "k1", "k2", "k3"]),
              "clc_track_job": (abi.TrackJob, [f for f, _ in abi.TrackJob._fields_])}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "coloc_hip.h"', 'int main(void) {']
    for name, (_, fields) in probes.items():
        src.append('printf("%s %%zu", sizeof(%s));' % (name, name))
        for f in fields:
            src.append('printf(" %%zu", offsetof(%s, %s));' % (name, f))
        src.append('printf("\\n");')
    src += ['return 0;', '}']
    c = tmp_path / "probe.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    for line in subprocess.check_output([str(exe)], text=True).strip().splitlines():
        parts = line.split()
        cls, fields = probes[parts[0]]
        assert C.sizeof(cls) == int(parts[1]), parts[0]
        for f, off in zip(fields, parts[2:]):
            assert getattr(cls, f).offset == int(off), (parts[0], f)


def _ud_lib():
    out = os.path.join(ROOT, "tests", "host", "libud_pixel_host.so")
    src = os.path.join(ROOT, "tests", "host", "ud_pixel_lib.cpp")
    hdr = os.path.join(ROOT, "coloc_amd", "host", "coloc_hip_geometry.hpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    return C.CDLL(out)


def _pixel_grid(W, H, ppx, ppy):
    """the principal point, the image corners, a regular grid, float32 feature positions of random keypoints, far outside the image"""
    import synth
    gx, gy = np.meshgrid(np.linspace(0.0, W, 23), np.linspace(0.0, H, 17))
    feat = track_host.feature_positions(synth.random_keypoints(500, W, H, seed=9)).astype(np.float64)
    fixed = np.array([[ppx, ppy], [0.0, 0.0], [W, 0.0], [0.0, H], [W, H], [W - 1.0, H - 1.0], [ppx, 0.0], [0.0, ppy], [ppx + 1e-9, ppy],
                      [ppx, ppy - 1e-300], [-0.5 * W, 1.7 * H]])
    return np.concatenate([fixed, np.stack([gx.ravel(), gy.ravel()], 1), feat])


def test_get_ud_pixel_restatement_has_the_host_members_bits():
    lib = _ud_lib()
    for (W, H, f, ppx, ppy) in [(1280, 720, 1000.0, 640.0, 360.0), (640, 480, 517.3, 318.6, 255.3)]:
        p = np.ascontiguousarray(_pixel_grid(W, H, ppx, ppy))
        for k in track_host.DISTORTIONS:
            cam = np.array([f, ppx, ppy, *k], dtype=np.float64)
            want = np.zeros_like(p)
            lib.ud_pixel_host(cam.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), C.c_int(len(p)), want.ctypes.data_as(C.c_void_p))
            got = track_host.get_ud_pixel(p, cam)
            assert np.isfinite(want).all()
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (W, k, int((got != want).sum()))
            # (sanity: without distortion the pixel comes back to within rounding; with it, it moves)
            if k == (0.0, 0.0, 0.0):
                assert np.abs(want - p).max() < 1e-9
            else:
                assert np.abs(want - p).max() > 1.0


def test_build_tracks_rule():
    """the compaction rule on a hand-made case: ascending queries, -1 / out-of-range / past-the-count rows dropped"""
    match = np.array([2, -1, 5, 0, -7, 1, 4, 3], dtype=np.int32)
    X = np.arange(15, dtype=np.float64).reshape(5, 3)
    feat = np.arange(32, dtype=np.float32).reshape(8, 4)
    cam = (100.0, 8.0, 6.0, 0.0, 0.0, 0.0)
    q, m, Xt, x = track_host.build_tracks(match, X, cam, feat=feat, count=7)
    assert q.tolist() == [0, 3, 5, 6] and m.tolist() == [2, 0, 1, 4]
    assert np.array_equal(Xt, X[[2, 0, 1, 4]]) and x.shape == (4, 2)
    assert np.abs(x - feat[[0, 3, 5, 6], :2]).max() < 1e-12

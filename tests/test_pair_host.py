"""tests/pair_host.py, the yardstick the GPU tests hold the pair kernel to, against the product's host get_ud_pixel
(tests/host/ud_pixel_lib.cpp: Pinhole_Intrinsic_Radial_K3 of coloc_amd/host/coloc_hip_geometry.hpp, the member
HIPRobustMatcher::computeRelativePose calls), bit for bit; and its compaction rule on hand-made cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pair_host
import synth
import track_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1280, 720


def _ud_lib():
    out = os.path.join(ROOT, "tests", "host", "libud_pixel_host.so")
    src = os.path.join(ROOT, "tests", "host", "ud_pixel_lib.cpp")
    hdr = os.path.join(ROOT, "coloc_amd", "host", "coloc_hip_geometry.hpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out])
    return C.CDLL(out)


def _host_ud(lib, p, cam):
    p = np.ascontiguousarray(p, dtype=np.float64)
    cam = np.array(cam, dtype=np.float64)
    out = np.zeros_like(p)
    lib.ud_pixel_host(cam.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), C.c_int(len(p)), out.ctypes.data_as(C.c_void_p))
    return out


def _case(seed, nq, nt):
    rng = np.random.default_rng(seed)
    kpsA, kpsB = synth.random_keypoints(nq, W, H, seed=seed + 1), synth.random_keypoints(nt, W, H, seed=seed + 2)
    featA = np.zeros((nq, 4), dtype=np.float32); featB = np.zeros((nt, 4), dtype=np.float32)
    featA[:, :2] = np.stack([rng.uniform(0, W, nq), rng.uniform(0, H, nq)], 1)
    featB[:, :2] = np.stack([rng.uniform(0, W, nt), rng.uniform(0, H, nt)], 1)
    match = rng.integers(0, nt, nq).astype(np.int32)
    u = rng.random(nq)
    match[u < 0.25] = -1
    match[(u >= 0.25) & (u < 0.33)] = nt + rng.integers(0, 1000, nq)[(u >= 0.25) & (u < 0.33)]      # past camera B's rows: "no match"
    match[(u >= 0.33) & (u < 0.40)] = -2 - rng.integers(0, 1 << 20, nq)[(u >= 0.33) & (u < 0.40)]    # negative other than -1
    # a pair whose two ends sit exactly on the principal points (r2 == 0 on both sides)
    j = nq // 2
    kpsA[j] = (640, 360, 0, 0.0, 0); featA[j, :2] = (640.0, 360.0)
    kpsB[5] = (640, 360, 0, 0.0, 0); featB[5, :2] = (640.0, 360.0)
    match[j] = 5
    return match, kpsA, kpsB, featA, featB


@pytest.mark.parametrize("da", range(3))
def test_build_pairs_has_the_host_members_bits(da):
    lib = _ud_lib()
    nq, nt = 900, 700
    match, kpsA, kpsB, featA, featB = _case(31 + da, nq, nt)
    camA = (1000.0, 640.0, 360.0) + track_host.DISTORTIONS[da]
    camB = (1000.0, 640.0, 360.0) + track_host.DISTORTIONS[(da + 1) % 3]               # a different set per camera
    for forms in ("kk", "kf", "fk", "ff"):
        a = dict(kpsA=kpsA) if forms[0] == "k" else dict(featA=featA)
        b = dict(kpsB=kpsB) if forms[1] == "k" else dict(featB=featB)
        for countA, countB in ((None, None), (nq - 200, nt - 150), (nq + 9, nt + 9)):
            q, t, x1, x2 = pair_host.build_pairs(match, nt, camA, camB, countA=countA, countB=countB, **a, **b)
            # the host loop, written out: ascending q, the out-of-range rule, the two positions through the two cameras
            nqe, nte = min(nq, countA or nq), min(nt, countB or nt)
            wq = [i for i in range(nqe) if 0 <= match[i] < nte]
            wt = [int(match[i]) for i in wq]
            assert q.tolist() == wq and t.tolist() == wt and len(wq) > 300
            pA = track_host.feature_positions(kpsA)[wq] if forms[0] == "k" else featA[wq, :2]
            pB = track_host.feature_positions(kpsB)[wt] if forms[1] == "k" else featB[wt, :2]
            w1, w2 = _host_ud(lib, pA.astype(np.float64), camA), _host_ud(lib, pB.astype(np.float64), camB)
            assert np.isfinite(w1).all() and np.isfinite(w2).all()
            assert np.array_equal(x1.view(np.uint64), w1.view(np.uint64)), (forms, countA)
            assert np.array_equal(x2.view(np.uint64), w2.view(np.uint64)), (forms, countA)
            if countA is None:
                k = wq.index(nq // 2)
                assert x1[k].tolist() == [640.0, 360.0] and x2[k].tolist() == [640.0, 360.0]      # r2 == 0: the pixel itself


def test_build_pairs_rule():
    match = np.array([2, -1, 5, 0, -7, 1, 4, 3], dtype=np.int32)
    featA = np.arange(32, dtype=np.float32).reshape(8, 4)
    featB = 100 + np.arange(10, dtype=np.float32).reshape(5, 2)
    cam = (100.0, 8.0, 6.0, 0.0, 0.0, 0.0)
    q, t, x1, x2 = pair_host.build_pairs(match, 5, cam, cam, featA=featA, featB=featB, countA=7)
    assert q.tolist() == [0, 3, 5, 6] and t.tolist() == [2, 0, 1, 4]
    assert np.abs(x1 - featA[[0, 3, 5, 6], :2]).max() < 1e-12 and np.abs(x2 - featB[[2, 0, 1, 4]]).max() < 1e-11
    q, t, _, _ = pair_host.build_pairs(match, 5, cam, cam, featA=featA, featB=featB, countB=3)
    assert q.tolist() == [0, 3, 5] and t.tolist() == [2, 0, 1]
    q, t, x1, x2 = pair_host.build_pairs(np.full(4, -1, dtype=np.int32), 5, cam, cam, featA=featA, featB=featB)
    assert len(q) == 0 and x1.shape == (0, 2) and x2.shape == (0, 2)
    with pytest.raises(ValueError):
        pair_host.build_pairs(match, 5, cam, cam, featA=featA)

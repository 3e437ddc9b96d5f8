"""The one-to-one filter behind the drop-in policy class: HIPMatcher::matchSceneWithMapBinnedUniqueDev and
HIPMatcher::computeMatchesPairUnique through a compiled driver (tests/host/match_unique_driver.cpp, g++ only, over the C ABI).  What they
leave equals the binding's result on the same data, exactly."""
import os
import subprocess

import numpy as np
import pytest

import bin_host as bh
import unique_host as uh
import test_gpu_map_guided as tg
from test_gpu_match_unique import _pair_with_doubles

pytestmark = pytest.mark.gpu

ROOT = tg.ROOT


def test_policy_members_equal_the_entries(monkeypatch, tmp_path):
    torch = tg._torch()
    from coloc_amd import build
    lib = build.build()
    exe = str(tmp_path / "match_unique_driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "coloc_amd", "host"),
                           os.path.join(ROOT, "tests", "host", "match_unique_driver.cpp"), "-o", exe, "-L", os.path.dirname(lib), "-lcoloc_hip",
                           "-ldl", "-Wl,-rpath," + os.path.dirname(lib)])
    nq0, nm, radius, thr = 300, 513, 4.0, 20
    C = (0.3, -0.2, 0.5)
    Rt = tg._pose(0.05, -0.1, 0.03, C=C)
    Q, M, _, kps, X = tg._general_case(nq0, nm, 606, tg.CAM_K, Rt)
    rng = np.random.RandomState(607)
    twins = np.arange(0, nq0, 3)                                               # a second keypoint ON every third one, a near-copy of its descriptor
    Q = np.concatenate([Q, np.array([uh._flip(rng, Q[i], 3) for i in twins], dtype=np.uint8)])
    nq = len(Q)
    both = np.zeros(nq, dtype=kps.dtype)                                       # (np.concatenate would pack the record's layout)
    both[:nq0], both[nq0:] = kps, kps[twins]
    kps = both
    A, B = _pair_with_doubles(300, 257, 43, 608)
    np.concatenate([tg.CAM_K, Rt[:, :3].reshape(-1), C, [nq, nm, radius, thr], X.reshape(-1)]).astype(np.float64).tofile(tmp_path / "map_binned.bin")
    kps.tofile(tmp_path / "kps.bin")
    np.concatenate([Q.reshape(-1), M.reshape(-1)]).tofile(tmp_path / "desc.bin")
    A.tofile(tmp_path / "pair_a.bin")
    B.tofile(tmp_path / "pair_b.bin")
    res = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    got = np.fromfile(tmp_path / "map_unique_out.bin", dtype=np.int32)
    got_pairs = np.fromfile(tmp_path / "pair_unique_out.bin", dtype=np.int32).reshape(-1, 2)
    ctx = tg._ctx(monkeypatch, "matrix", M=M, X=X)
    try:
        assert ctx.map_binned_plan(tg.CAM_K, radius)["plan"] == bh.BINNED
        plain = tg._Job(Q, nm, Rt, radius, thr, tg.CAM_K, kps=kps)
        ctx.match_map_binned_dev(**plain.kw)
        job = tg._Job(Q, nm, Rt, radius, thr, tg.CAM_K, kps=kps)
        d_owner = torch.full((nm,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.match_map_binned_unique_dev(d_owner=d_owner.data_ptr(), **job.kw)
        ctx.sync()
        want_m, want_o = job.result()["match"], d_owner.cpu().numpy()
        assert len(uh.doubled_rows(plain.result()["match"])) >= 5 and len(uh.doubled_rows(want_m)) == 0
        assert (want_m >= 0).sum() > 20
        assert np.array_equal(got[:nq], want_m) and np.array_equal(got[nq:], want_o)
        m, _ = ctx.match_unique(A, B, 40)
        assert len(uh.doubled_rows(ctx.match_2nn(A, B, 40))) >= 20
        want_pairs = np.column_stack([np.nonzero(m >= 0)[0], m[m >= 0]])
        assert len(want_pairs) > 200 and np.array_equal(got_pairs, want_pairs)
    finally:
        ctx.close()

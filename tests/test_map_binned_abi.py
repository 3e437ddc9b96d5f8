"""The entries of the map match through a cell grid (include/coloc_hip.h: clc_match_map_binned_dev, clc_match_map_binned_batch_dev,
clc_map_bin_build_dev, clc_map_binned_plan) without a GPU: declared, exported and bound under ABI 4, the argument rules that need no
device work return the stated codes, and clc_map_binned_plan is right on both sides of each of the plan's limits.  The plan reads nothing
of a context but its number of map rows, so a compiled driver (tests/host/map_binned_plan_driver.cpp) calls the entry on a
default-constructed context with that number set."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bin_host as bh
import guided_host as gh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["clc_match_map_binned_dev", "clc_match_map_binned_batch_dev", "clc_map_bin_build_dev", "clc_map_binned_plan"]
CAM = gh.CAM_EXACT


def test_entries_are_declared_exported_and_bound():
    from coloc_amd import abi
    hdr = open(os.path.join(ROOT, "include", "coloc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = abi.load_library()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name + " not declared"
        assert hasattr(lib, name), name + " not exported"
        assert name in abi.EXPORTS
    assert re.search(r"#define\s+CLC_ABI_VERSION\s+4\b", code)
    assert lib.clc_abi_version() == abi.ABI_VERSION == 4
    for meth in ("match_map_binned_dev", "match_map_binned_batch_dev", "map_bin_build_dev", "map_binned_plan"):
        assert callable(getattr(abi.Context, meth))
    assert (abi.BIN_PLAN_SWEEP, abi.BIN_PLAN_BINNED) == (bh.SWEEP, bh.BINNED) == (0, 1)
    assert re.search(r"#define\s+CLC_BIN_PLAN_SWEEP\s+0\b", code) and re.search(r"#define\s+CLC_BIN_PLAN_BINNED\s+1\b", code)


def test_argument_rules_that_need_no_device_work():
    """refused before anything is enqueued, without a device: a null context, a null job, a job count outside 0 .. CLC_MAX_BATCH.  (The
    job's own rules and the context's state need a context: tests/test_gpu_map_binned.py::test_errors_and_edges.)"""
    from coloc_amd import abi
    lib = abi.load_library()
    BAD = abi.CLC_ERR_BAD_ARG
    j = abi.MapGuidedJob()
    abi._map_guided_fill(j, d_q=0x1000, nq=8, cam=(500.0, 320.0, 240.0, 0, 0, 0), Rt=[1, 0, 0, 0.5, 0, 1, 0, 0, 0, 0, 1, 2], radius=4.0, threshold=40,
                         d_match=0x3000, d_feat=0x4000)
    assert lib.clc_match_map_binned_dev(None, C.byref(j), None) == BAD
    assert lib.clc_match_map_binned_dev(None, None, None) == BAD
    assert lib.clc_match_map_binned_batch_dev(None, C.byref(j), 1, None) == BAD
    assert lib.clc_match_map_binned_batch_dev(None, None, 0, None) == BAD
    assert lib.clc_match_map_binned_batch_dev(None, C.byref(j), -1, None) == BAD
    assert lib.clc_match_map_binned_batch_dev(None, C.byref(j), abi.MAX_BATCH + 1, None) == BAD
    assert lib.clc_map_bin_build_dev(None, C.byref(j), 0x5000, 0x6000, None) == BAD
    assert lib.clc_map_bin_build_dev(None, None, 0x5000, 0x6000, None) == BAD
    info = (C.c_int32 * 4)()
    cam = abi.CameraK3(500.0, 320.0, 240.0, 0.0, 0.0, 0.0)
    assert lib.clc_map_binned_plan(None, C.byref(cam), C.c_float(4.0), info, None) == BAD


def _plan_driver(tmp_path):
    from coloc_amd import build
    lib = build.build()
    exe = str(tmp_path / "map_binned_plan_driver")
    # (clc_ctx.h brings the HIP runtime's headers: the project's own compiler builds the driver, as it builds the library)
    subprocess.check_call([build.hipcc_path(), "--offload-arch=gfx950", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "coloc_amd", "csrc"), os.path.join(ROOT, "tests", "host", "map_binned_plan_driver.cpp"), "-o", exe,
                           "-L", os.path.dirname(lib), "-lcoloc_hip", "-Wl,-rpath," + os.path.dirname(lib)])
    return exe


def test_the_plan_on_both_sides_of_each_limit(tmp_path):
    f32 = np.float32
    cam = lambda ppx, ppy: (500.0, ppx, ppy, 0, 0, 0)
    below = float(np.nextafter(f32(2.0 ** -10), f32(0)))
    rw8 = 8.0 * (1.0 + 2.0 ** -10)                                             # rw of radius 8, exact
    exact = cam(4.0 * rw8, 3.0)                                                # W = 2 ppx = 8 rw exactly
    assert 8.0 * bh.grid(exact, 8.0)[0] == bh.grid(exact, 8.0)[1]
    cases = [(CAM, 3.0, 1000, bh.BINNED),
             (CAM, 2.0 ** -10, 1000, bh.BINNED), (CAM, below, 1000, bh.SWEEP),                                   # radius >= 2^-10
             (exact, 8.0, 1000, bh.BINNED), (cam(float(np.nextafter(4.0 * rw8, 0.0)), 3.0), 8.0, 1000, bh.SWEEP),    # 8 rw <= W
             (CAM, 79.9, 1000, bh.BINNED), (CAM, 80.0, 1000, bh.SWEEP), (CAM, 2000.0, 1000, bh.SWEEP),
             (CAM, 3.0, 65536, bh.BINNED), (CAM, 3.0, 65537, bh.SWEEP), (CAM, 3.0, 1, bh.BINNED), (CAM, 3.0, 0, bh.SWEEP),   # 0 < map_n <= 65 536
             (CAM, 3.0, -1, bh.SWEEP),                                                                           # (no map set)
             (cam(5e-324, 320.0), 3.0, 1000, bh.BINNED), (cam(0.0, 320.0), 3.0, 1000, bh.SWEEP),                  # ppx, ppy finite and positive
             (cam(320.0, -240.0), 3.0, 1000, bh.SWEEP), (cam(np.inf, 240.0), 3.0, 1000, bh.SWEEP), (cam(320.0, np.nan), 3.0, 1000, bh.SWEEP),
             (CAM, np.nan, 1000, bh.SWEEP), (CAM, np.inf, 1000, bh.SWEEP)]
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for c, radius, nm, _ in cases:
            f.write("%s %s %x %d\n" % (float(c[1]).hex(), float(c[2]).hex(), int(np.array([radius], dtype=f32).view(np.uint32)[0]), nm))
    out = subprocess.run([_plan_driver(tmp_path), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    for (c, radius, nm, want), line in zip(cases, lines):
        rc, plan, cells, lanes, zero, side = line.split()
        assert int(rc) == 0 and int(plan) == want == bh.plan(c, radius, nm) == bh.cxx_plan(c, radius, nm), (c, radius, nm, line)
        assert (int(cells), int(zero)) == (bh.AXIS, 0) and int(lanes) in (4, 8, 16, 32, 64), line
        got, st = float.fromhex(side) if side not in ("nan", "-nan") else float("nan"), bh.grid(c, radius)[2]
        assert got == st or (got != got and st != st), (c, radius, line)

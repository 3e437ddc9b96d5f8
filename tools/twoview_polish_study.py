#!/usr/bin/env python3
"""How many Newton steps on det(a + x b) the seven-point solver needs: the host build of
coloc_amd/csrc/twoview_min.h with CLC_TV_POLISH_STEPS = 0 (the closed-form cubic alone), 1, 2, 3 on N random samples of every 'F'
pool of tests/twoview_cases.py, scored by the backward error of tests/twoview_mp.py (60 digits).  Prints, per class and step count,
the median and the worst backward error in pixels, the number of models above 4096 * 2^-53 * max(w, h), the worst ratio of the
smallest to the largest singular value of a returned model, and how many roots the last step still moved by more than 1e-12 relative.

    python tools/twoview_polish_study.py [N]        # N = 300 by default, a few minutes
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import twoview_cases as cases   # noqa: E402
import twoview_host as tvh      # noqa: E402
import twoview_mp               # noqa: E402


def build(steps, tmp):
    out = os.path.join(tmp, "libtv_steps%d.so" % steps)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DCLC_TV_POLISH_STEPS=%d" % steps, "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "host", "twoview_host_lib.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.tv_host_seven_point.restype = C.c_int
    return lib


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    tvh.lib()
    with tempfile.TemporaryDirectory() as tmp:
        libs = {s: build(s, tmp) for s in (0, 1, 2, 3)}
        for name in cases.pool_names("F"):
            p, wh = cases.pool("F", name), cases.image_size(name)
            rng = np.random.default_rng(77)
            smp = np.stack([rng.choice(cases.POOL, 7, replace=False) for _ in range(n)])
            x1, x2 = p[smp][..., :2], p[smp][..., 2:]
            first = 4096.0 * cases.EPS * max(wh)
            prev = None
            for steps, lib in libs.items():
                tvh._LIB = lib
                slots = tvh.class_slots("F", x1, x2, wh)
                be, sr = [], 0.0
                for i in range(n):
                    for g in cases.check_slots(slots[i]):
                        be.append(twoview_mp.backward_error("F", g, x1[i], x2[i], wh))
                        sr = max(sr, twoview_mp.sigma_ratio(g))
                moved = -1
                if prev is not None and np.array_equal(np.isnan(prev), np.isnan(slots)):
                    with np.errstate(invalid="ignore"):
                        u0 = prev / np.sqrt(np.nansum(prev * prev, axis=2, keepdims=True))
                        u1 = slots / np.sqrt(np.nansum(slots * slots, axis=2, keepdims=True))
                        moved = int((np.nanmax(np.abs(u0 - u1), axis=2) > 1e-12).sum())
                prev = slots
                be = np.array(be)
                print("%-10s steps %d: models %d, backward error median %.2e worst %.2e px, above the first term (%.2e): %d, worst "
                      "sigma3/sigma1 %.1e, models this step moved by more than 1e-12: %d"
                      % (name, steps, len(be), np.median(be), be.max(), first, int((be > first).sum()), sr, moved), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's own KFAST<mt, true> / featureAngle (include/coloc/KFAST.h, FeatureAngle.h), compiled into
oracle/_ref/ by `make -C oracle ref` where the reference tree is present, run on exactly the inputs of the fast9 tests in
tests/test_oracle_clatch.py: tests/golden/fast9_ref.npz.  These are genuine reference outputs (like feeder_ref.npz), each stored with
the sha256 of the input it was computed on.

Run:  python tests/golden/make_golden_fast9.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib  # noqa: E402
import test_oracle_clatch as t  # noqa: E402


def xys(k):
    return np.stack([k["x"], k["y"], k["score"].astype(np.int32)], 1).astype(np.int32)


def main():
    ref = oracle_lib.RefFeeder()
    out = {}
    for (W, H, seed) in t.REF_CASES:
        key = "case_%dx%d_%d" % (W, H, seed)
        img = t.ref_case_image(W, H, seed)
        out[key + "_sha256"] = t.digest(img)
        for mt in (True, False):
            out[key + "_mt%d_xys" % mt] = xys(ref.kfast(img, 40, mt))
        k = ref.kfast(img, 40, True)
        out[key + "_angle"] = np.array([ref.feature_angle(img, int(p["x"]), int(p["y"])) for p in k[:200]], dtype=np.float32)
    for W, _, img in t.quirk_images():
        out["quirk_%d_sha256" % W] = t.digest(img)
        out["quirk_%d_count" % W] = np.array(len(ref.kfast(img, 40, False)))
    for (W, H) in t.EDGE_SIZES:
        img = t.edge_image(W, H)
        out["edge_%dx%d_sha256" % (W, H)] = t.digest(img)
        out["edge_%dx%d_xys" % (W, H)] = xys(ref.kfast(img, 40, False))
    np.savez_compressed(os.path.join(HERE, "fast9_ref.npz"), **out)
    print("written", os.path.join(HERE, "fast9_ref.npz"))


if __name__ == "__main__":
    main()

"""Writes tests/golden/inter_geometry_host.npz: what inter_relative / inter_scale_pose (coloc_amd/csrc/inter_geometry.cpp) return, bit
for bit, on the cases of tests/inter_scenes.py -- computed by the PARENT of the commit that moved their arithmetic into
coloc_amd/csrc/inter_math.h, so that tests/test_inter_geometry_host.py holds the moved statements to the bits they had before the move.

The committed fixture was written from commit e360ba3 ("Run the inter-camera step from device memory: map, scale, pose on GPU"), whose
inter_geometry.cpp still carried the statements itself:
    git worktree add <dir> e360ba3 && python tools/make_inter_geometry_golden.py <dir>
The wrapper tests/host/inter_geometry_lib.cpp of THIS tree is copied into <dir> and built there against <dir>'s inter_geometry.cpp (g++
-O2 -ffp-contract=off, no GPU).  Run it against a later commit only to change the cases, never to make a failing test pass.

Before anything is written, every case is checked to take the branch it is there for (the stages, a vote and a screen that reject
something, both median branches, one dropped term)."""
import os
import shutil
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "tests"))
import inter_geometry_host as H
import inter_scenes as S


def walk(o, name):
    """the kept common features of a scale case and the float d2 of every consecutive pair, the way inter_scale_pose walks them"""
    fname, form, _ = S.SCALE_CASES[name]
    p = S.front_inputs(fname)["pair"]
    com, Xt = o["scale/%s/common" % name], o["front/%s/Xt" % fname].reshape(-1, 3)
    Rs = p["Rt_source"]
    ratio = np.linalg.norm(p["map_X"][com[:, 0]] @ Rs[:, :3].T + Rs[:, 3], axis=1) / np.linalg.norm(Xt[com[:, 1]], axis=1)
    keep = com[np.abs(ratio / np.median(ratio) - 1.0) < 0.2]
    d2 = np.linalg.norm(np.diff(Xt[keep[:, 1]], axis=0), axis=1).astype(np.float32)
    return len(com), keep, d2


def main(parent):
    shutil.copy(os.path.join(R, "tests", "host", "inter_geometry_lib.cpp"), os.path.join(parent, "tests", "host", "inter_geometry_lib.cpp"))
    o = H.run_cases(parent)
    for name, (_, _, which, stage) in S.FRONT_CASES.items():
        got, nf, ni = int(o["front/%s/stage" % name]), int(o["front/%s/n_front" % name]), len(o["front/%s/inliers" % name])
        print("front %-13s stage %d  inliers %4d  n_front %4d" % (name, got, ni, nf))
        assert got == stage, name
        if which == "mixed":
            assert 8 <= nf < ni, (name, "the vote rejects nothing")
    assert len(o["front/few_inliers/inliers"]) == 12 and len(o["front/all_replaced/inliers"]) == 13
    for name, (fname, form, stage) in S.SCALE_CASES.items():
        got, nc = int(o["scale/%s/stage" % name]), int(o["scale/%s/n_common" % name])
        raw, keep, d2 = walk(o, name)
        dropped = int((d2 <= 1e-9).sum())
        print("scale %-15s stage %d  common %4d  kept %4d  dropped terms %d  scale %.6f" % (name, got, raw, nc, dropped, float(o["scale/%s/scale" % name])))
        assert got == stage, name
        if stage == 0:
            assert nc == len(keep) and dropped == (form == "twin"), name
            p = S.front_inputs(fname)["pair"]                  # (the scale is the true baseline, to a few per cent)
            assert abs(float(o["scale/%s/scale" % name]) / np.linalg.norm(p["td"] - p["Rd"] @ p["Rs"].T @ p["ts"]) - 1.0) < 0.05, name
        if form in ("shortcut", "chain") and not fname.startswith("n60"):
            assert 8 <= nc < raw, (name, "the screen rejects nothing")
    assert len(o["scale/odd/common"]) & 1 and not len(o["scale/even/common"]) & 1
    assert int(o["scale/seven/n_common"]) == 7
    assert np.array_equal(np.sort(o["scale/n900a_chain/common"][:, 0]), o["scale/n900a_chain/common"][:, 0]) and (np.diff(o["scale/n900a_shortcut/common"][:, 1]) > 0).all()
    path = os.path.join(R, "tests", "golden", "inter_geometry_host.npz")
    np.savez_compressed(path, **H.fixture_form(o))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))

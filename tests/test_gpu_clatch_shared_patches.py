"""CLATCH with the slot table that seats triplets sharing a patch in one half-wave (coloc_amd/csrc/latch_layout_swap.inc, searched under
the merged-read model of tools/latch_anneal.c): the descriptors stay the oracle's, bit for bit.  One small image, three pyramid levels, 192
keypoints with every level, the special angles and clamped windows among them.  The set is chosen so that each of the 512 descriptor bits
takes both values in the ORACLE's output: a slot that un-permutes into the wrong bit, or evaluates the wrong triplet, then cannot hide
behind a bit that is constant over the set."""
import math

import numpy as np
import pytest

import synth

W, H, LEVELS, N, SEED = 96, 80, 3, 192, 20250


def _inputs():
    rng = np.random.default_rng(SEED)
    img = rng.integers(0, 256, (H, W), dtype=np.uint8)
    ws, hs, _ = synth.pyramid_dims(W, H, levels=LEVELS)
    rows = []
    special = [0.0, math.pi / 2, -math.pi / 2, math.pi, math.pi / 4, -3 * math.pi / 4]
    # 24 keypoints within 8 px of a border or corner (8 per level): the window's clamps act on every side
    for lv in range(LEVELS):
        w, h = ws[lv], hs[lv]
        spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, int(rng.integers(0, 8))), (w // 2, h - 1 - int(rng.integers(0, 8))),
                 (int(rng.integers(0, 8)), h // 2), (w - 1 - int(rng.integers(0, 8)), h // 2)]
        for i, (x, y) in enumerate(spots):
            rows.append((x, y, special[i] if i < len(special) else (rng.random() * 2 - 1) * math.pi, lv))
    # the rest anywhere, levels in turn; the first of them at the special angles
    while len(rows) < N:
        lv = len(rows) % LEVELS
        a = special[len(rows) % len(special)] if len(rows) < 48 else (rng.random() * 2 - 1) * math.pi
        rows.append((int(rng.integers(0, ws[lv])), int(rng.integers(0, hs[lv])), a, lv))
    kps = np.zeros(N, dtype=synth.KP_DTYPE)
    for i, (x, y, a, lv) in enumerate(rows):
        kps[i]["x"], kps[i]["y"], kps[i]["angle"], kps[i]["scale"] = x, y, np.float32(a), lv
    return img, kps, ws, hs


def _check_set(kps, ws, hs):
    assert len(kps) == N and set(kps["scale"].tolist()) == set(range(LEVELS))
    ang = kps["angle"]
    assert (ang == 0).any() and (ang == np.float32(math.pi / 2)).any() and (ang == np.float32(-math.pi / 2)).any()
    w, h = np.array(ws)[kps["scale"]], np.array(hs)[kps["scale"]]
    near = (kps["x"] < 8) | (kps["y"] < 8) | (kps["x"] >= w - 8) | (kps["y"] >= h - 8)
    assert int(near.sum()) >= 16
    assert ((kps["x"] >= 0) & (kps["x"] < w) & (kps["y"] >= 0) & (kps["y"] < h)).all()


def _oracle_descriptors(oracle):
    img, kps, ws, hs = _inputs()
    _check_set(kps, ws, hs)
    want = oracle.clatch(oracle.pyramid(img, levels=LEVELS), kps)
    bits = np.unpackbits(want, axis=1, bitorder="little")
    assert bits.shape == (N, 512)
    ones = bits.sum(axis=0)
    stuck = np.nonzero((ones == 0) | (ones == N))[0]
    assert stuck.size == 0, "descriptor bits constant over the set (choose another seed): %s" % stuck[:10]
    return img, kps, want


def test_every_descriptor_bit_takes_both_values_in_the_oracle(oracle):
    _oracle_descriptors(oracle)


@pytest.mark.gpu
def test_descriptors_equal_the_oracle_bit_for_bit(oracle):
    from coloc_amd import Context
    img, kps, want = _oracle_descriptors(oracle)
    ctx = Context(device=0, width=W, height=H, maxkp=256)
    ctx.pyramid_build(img)
    got = ctx.describe(kps)
    ctx.close()
    diff = np.unpackbits(got ^ want, axis=1, bitorder="little")
    bad = np.nonzero(diff.any(axis=1))[0]
    assert bad.size == 0, "keypoints %s differ; descriptor bits %s" % (bad[:10], np.nonzero(diff.any(axis=0))[0][:16])

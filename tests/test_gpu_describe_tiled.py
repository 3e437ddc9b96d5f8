"""CLATCH gathers its samples from a second, column-strip copy of every pyramid level (clc_internal.h: LevelDesc) that the
pyramid launch writes beside the row-major one.  Descriptors must stay bit-identical to the CPU oracle's CLATCH (src/CLATCH.cu:157-188)
on every route that fills a pyramid, at image sizes that are no multiple of the strip width (16) or the padded height (8), with every
clamp firing, and a context must never describe from a strip copy left by an earlier image."""
import math

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

SIZES = [(101, 67), (37, 29)]
ANGLES = [0.0, math.pi / 4, math.pi / 2, math.pi, -math.pi / 2]


def _image(W, H, kind, seed=5):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)
    # gradient: ramps along x and y so that a transposed or shifted gather changes the sums
    x = np.arange(W)[None, :] * 255 // (W - 1)
    y = np.arange(H)[:, None] * 255 // (H - 1)
    return ((x * 2 + y + seed) // 3).astype(np.uint8)


def _keypoints(W, H, seed=11, n=500):
    """~n keypoints over all eight levels: every position within 3 px of each border and corner on every level (all four clamps fire),
    the rest uniform; angles cycle through 0, pi/4, pi/2, pi, -pi/2 and a random one."""
    rng = np.random.default_rng(seed)
    ws, hs, _ = synth.pyramid_dims(W, H)
    rows = []
    for lv in range(8):
        w, h = int(ws[lv]), int(hs[lv])
        for d in range(4):
            d = min(d, w - 1, h - 1)
            rows += [(d, h // 2, lv), (w - 1 - d, h // 2, lv), (w // 2, d, lv), (w // 2, h - 1 - d, lv),
                     (d, d, lv), (w - 1 - d, d, lv), (d, h - 1 - d, lv), (w - 1 - d, h - 1 - d, lv)]
    while len(rows) < n:
        lv = int(rng.integers(0, 8))
        rows.append((int(rng.integers(0, ws[lv])), int(rng.integers(0, hs[lv])), lv))
    kps = np.zeros(len(rows), dtype=synth.KP_DTYPE)
    for i, (x, y, lv) in enumerate(rows):
        a = ANGLES[i % 6] if i % 6 < 5 else rng.uniform(-math.pi, math.pi)
        kps[i] = (x, y, 0, np.float32(a), lv)
    return kps


_REF = {}


def _ref(oracle, W, H, kind, seed=5):
    """(image, keypoints, oracle descriptors), computed once per case and shared (read-only) by the tests"""
    key = (W, H, kind, seed)
    if key not in _REF:
        img = _image(W, H, kind, seed)
        kps = _keypoints(W, H)
        want = oracle.clatch(oracle.pyramid(img), kps)
        want.setflags(write=False)
        _REF[key] = (img, kps, want)
    return _REF[key]


def _ctx(W, H, maxkp=1024):
    from coloc_amd import Context
    return Context(device=0, width=W, height=H, maxkp=maxkp)


def _device_image(img, pitch):
    import torch
    t = torch.full((img.shape[0], pitch), 0xAB, dtype=torch.uint8, device="cuda:0")
    t[:, :img.shape[1]] = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    return t


def _describe_dev_route(ctx, img, kps, pitch):
    d = _device_image(img, pitch)
    ctx.pyramid_build_dev(d.data_ptr(), img.shape[1], img.shape[0], pitch)
    return ctx.describe(kps)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", ["noise", "gradient"])
def test_odd_sizes_all_levels_borders_angles(oracle, W, H, kind):
    img, kps, want = _ref(oracle, W, H, kind)
    assert len(kps) >= 500 and set(kps["scale"]) == set(range(8))
    ctx = _ctx(W, H)
    ctx.pyramid_build(img)
    got = ctx.describe(kps)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, "descriptors differ for keypoints %s" % [tuple(kps[i]) for i in bad[:5]]
    ctx.close()


@pytest.mark.parametrize("route", ["host", "device"])
def test_second_image_is_not_described_from_a_stale_copy(oracle, route):
    W, H = SIZES[0]
    (img1, kps, want1), (img2, _, want2) = _ref(oracle, W, H, "noise", 5), _ref(oracle, W, H, "noise", 6)
    assert not np.array_equal(want1, want2)
    ctx = _ctx(W, H)
    for img, want in ((img1, want1), (img2, want2), (img1, want1)):
        if route == "host":
            ctx.pyramid_build(img)
            got = ctx.describe(kps)
        else:
            got = _describe_dev_route(ctx, img, kps, W)
        assert np.array_equal(got, want)
    ctx.close()


def test_two_contexts_of_different_sizes(oracle):
    (imga, kpsa, wanta), (imgb, kpsb, wantb) = _ref(oracle, *SIZES[0], "gradient"), _ref(oracle, *SIZES[1], "noise")
    a, b = _ctx(*SIZES[0]), _ctx(*SIZES[1])
    a.pyramid_build(imga)
    b.pyramid_build(imgb)
    assert np.array_equal(b.describe(kpsb), wantb)
    assert np.array_equal(a.describe(kpsa), wanta)
    a.close(); b.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_in_place_level0_route_equals_device_image_route(oracle, W, H):
    """host image uploaded into the arena, then pyramid + describe (level 0 is never copied: its strips come from workgroups of their
    own) against the same pixels as a caller-owned device image"""
    img, kps, want = _ref(oracle, W, H, "noise")
    ctx = _ctx(W, H)
    ctx.pyramid_build(img)
    host = ctx.describe(kps)
    other = _ctx(W, H)
    dev = _describe_dev_route(other, img, kps, W)
    assert np.array_equal(host, dev) and np.array_equal(host, want)
    # and the in-place route behind a device-image frame on the same context
    _describe_dev_route(ctx, _image(W, H, "gradient"), kps, W)
    ctx.pyramid_build(img)
    assert np.array_equal(ctx.describe(kps), want)
    ctx.close(); other.close()


def test_device_image_with_pitch_larger_than_width(oracle):
    W, H = SIZES[0]
    img, kps, want = _ref(oracle, W, H, "gradient")
    ctx = _ctx(W, H)
    assert np.array_equal(_describe_dev_route(ctx, img, kps, 192), want)
    ctx.close()


def test_three_cameras_batched_equal_three_single_calls(oracle):
    import torch
    W, H = SIZES[0]
    pitch = 128
    cases = [_ref(oracle, W, H, "noise", 5), _ref(oracle, W, H, "gradient", 5), _ref(oracle, W, H, "noise", 6)]
    counts = [len(cases[0][1]), 200, 333]
    d_imgs = [_device_image(c[0], pitch) for c in cases]
    d_kps = [torch.from_numpy(c[1][:n].view(np.uint8).reshape(-1, 20).copy()).cuda() for c, n in zip(cases, counts)]
    d_desc = [torch.full((n, 64), 0xAB, dtype=torch.uint8, device="cuda:0") for n in counts]
    torch.cuda.synchronize()
    ctx, single = _ctx(W, H), _ctx(W, H)
    for _ in range(2):          # the second pass runs on slots the first one filled
        ctx.describe_batch_dev([t.data_ptr() for t in d_imgs], W, H, pitch, [t.data_ptr() for t in d_kps], counts, [t.data_ptr() for t in d_desc])
        ctx.sync()
        for c, n in enumerate(counts):
            single.pyramid_build(cases[c][0])
            one = single.describe(cases[c][1][:n])
            got = d_desc[c].cpu().numpy()
            assert np.array_equal(got, one), "camera %d" % c
            assert np.array_equal(got, cases[c][2][:n]), "camera %d against the oracle" % c
        d_imgs = d_imgs[1:] + d_imgs[:1]; d_kps = d_kps[1:] + d_kps[:1]; cases = cases[1:] + cases[:1]; counts = counts[1:] + counts[:1]
        d_desc = [torch.full((n, 64), 0xAB, dtype=torch.uint8, device="cuda:0") for n in counts]
        torch.cuda.synchronize()
    ctx.close(); single.close()

"""CLC_SELECT_STRONGEST (clc_detect_set_selection; coloc_amd/csrc/detect.hip) on the GPU: a frame with more corners than maxkp keeps
the maxkp highest scores, ties by list order, still listed level-major.  Expected = the oracle's UNCAPPED detection put through the
numpy statement of the rule (tests/test_detect_select_abi.py: select_strongest); every comparison is bit for bit.  The caps cut
through groups of tied scores; the tests assert that from the oracle before they look at the GPU."""
import functools
import subprocess

import numpy as np
import pytest

import synth
from test_detect_select_abi import cutoff_of, select_strongest

pytestmark = pytest.mark.gpu


def oracle_detect(oracle, img, thresh=40, levels=8):
    pyr = oracle.pyramid(img, levels=levels)
    out = []
    for lv, im in enumerate(pyr):
        k = oracle.fast9(im, thresh)
        k["scale"] = lv
        for i in range(len(k)):
            k["angle"][i] = oracle.feature_angle(im, int(k["x"][i]), int(k["y"][i]))
        out.append(k)
    return pyr, np.concatenate(out)


def same_kps(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in ("x", "y", "score", "scale")) and \
        np.array_equal(a["angle"].view(np.uint32), b["angle"].view(np.uint32))


def dense_image():
    """the frame of test_gpu_detect.py::test_dense_corners_every_tile"""
    W, H = 640, 480
    rng = np.random.default_rng(77)
    img = rng.integers(90, 110, size=(H, W)).astype(np.uint8)
    m = rng.random((H, W))
    img[m < 0.04] = 255
    img[m > 0.96] = 0
    return img


@functools.lru_cache(maxsize=None)
def _frame(name):
    if name == "dense":
        return dense_image()
    W, H, seed = name
    return synth.rect_image(W, H, seed=seed, noise_sigma=2.0)


_detected = {}


def uncapped(oracle, name, levels=8):
    """(image, pyramid, uncapped oracle detection) of a named frame, computed once per session"""
    key = (name, levels)
    if key not in _detected:
        img = _frame(name)
        _detected[key] = (img,) + oracle_detect(oracle, img, levels=levels)
    return _detected[key]


def strongest_ctx(W, H, cap, **kw):
    from coloc_amd import Context, SELECT_FIRST, SELECT_STRONGEST
    ctx = Context(device=0, width=W, height=H, maxkp=cap, **kw)
    assert ctx.keypoint_selection == SELECT_FIRST                      # the default
    ctx.set_keypoint_selection(SELECT_STRONGEST)
    assert ctx.keypoint_selection == SELECT_STRONGEST
    return ctx


# (frame, found, cap, cutoff, #above, #tied) -- measured on the oracle; cap 1 has no figures of its own
CASES = [((640, 480, 1000), 5006, 500, 177, 499, 4),
         ((640, 480, 1000), 5006, 2000, 109, 1965, 58),
         ((640, 480, 1000), 5006, 5000, 41, 4958, 48),
         ((1280, 720, 1002), 6469, 5000, 62, 4955, 88),
         ("dense", 51469, 1, None, None, None),
         ("dense", 51469, 1000, 153, 692, 480),
         ("dense", 51469, 20000, 93, 19415, 1494)]


@pytest.mark.parametrize("name,found,cap,cutoff,above,tied", CASES)
def test_strongest_are_kept_in_order(oracle, name, found, cap, cutoff, above, tied):
    img, _, want = uncapped(oracle, name)
    assert len(want) == found
    c, n_above, n_tied, kept = cutoff_of(want["score"], cap)
    if cutoff is not None:
        assert (c, n_above, n_tied) == (cutoff, above, tied)
        assert 1 <= kept < n_tied                                      # the cap cuts THROUGH the tied group
    sel = want[select_strongest(want["score"], cap)]
    assert len(sel) == cap
    ctx = strongest_ctx(img.shape[1], img.shape[0], cap)
    ctx.pyramid_build(img)
    for _ in range(2):                                                 # the second call meets what the first left behind
        kps, n_found = ctx.detect()
        assert n_found == found and len(kps) == cap
        assert same_kps(kps, sel)
    ctx.close()


def test_invalid_mode_is_refused_and_changes_nothing():
    from coloc_amd import Context, CLCError, SELECT_STRONGEST
    ctx = strongest_ctx(64, 64, 100)
    for bad in (2, -1, 7):
        with pytest.raises(CLCError) as e:
            ctx.set_keypoint_selection(bad)
        assert e.value.status == 1
    assert ctx.keypoint_selection == SELECT_STRONGEST
    ctx.close()
    m = Context(device=0, detector=False)                              # no detector options: nothing to select
    with pytest.raises(CLCError) as e:
        m.set_keypoint_selection(SELECT_STRONGEST)
    assert e.value.status == 5
    m.close()


@pytest.mark.parametrize("cap", [5006, 5007, 20000])
def test_no_overflow_equals_the_default_rule(oracle, cap):
    from coloc_amd import Context
    img, pyr, want = uncapped(oracle, (640, 480, 1000))
    assert len(want) == 5006 <= cap
    plain = Context(device=0, width=640, height=480, maxkp=cap)
    kps0, desc0, found0 = plain.detect_and_describe(img)
    plain.close()
    ctx = strongest_ctx(640, 480, cap)
    kps1, desc1, found1 = ctx.detect_and_describe(img)
    ctx.close()
    assert found0 == found1 == 5006 and len(kps0) == len(kps1) == 5006
    assert same_kps(kps1, kps0) and same_kps(kps1, want) and np.array_equal(desc1, desc0)


@pytest.mark.parametrize("W,H,seed,cap", [(640, 480, 1000, 300), (214, 161, 5, 150), (214, 161, 5, 449)])
def test_single_level_and_the_walk_replay_level(oracle, W, H, seed, cap):
    """scale_levels = 1; a 214-wide level replays the reference's row walk (KFAST.h:245) in front of the suppression: the scores that
    enter the histogram are those of the keypoints that survive it."""
    img, _, want = uncapped(oracle, (W, H, seed), levels=1)
    assert len(want) > cap
    sel = want[select_strongest(want["score"], cap)]
    ctx = strongest_ctx(W, H, cap, scale_levels=1)
    ctx.pyramid_build(img)
    kps, found = ctx.detect()
    ctx.close()
    assert found == len(want) and same_kps(kps, sel)


def test_walk_replay_level_inside_a_pyramid(oracle):
    """640 x 480: level 6 is 214 wide.  A cap that keeps keypoints of every level, so that level 6's own ranks are exercised."""
    img, _, want = uncapped(oracle, (640, 480, 1000))
    cap = 3000
    idx = select_strongest(want["score"], cap)
    assert set(want["scale"][idx]) == set(range(8))
    ctx = strongest_ctx(640, 480, cap)
    ctx.pyramid_build(img)
    kps, _ = ctx.detect()
    ctx.close()
    assert same_kps(kps, want[idx])


def test_device_chain_describes_the_selected(oracle):
    """clc_detect_dev -> clc_describe_detected_dev: the rows are the selected keypoints' descriptors."""
    import torch
    img, pyr, want = uncapped(oracle, (640, 480, 1000))
    cap = 2000
    sel = want[select_strongest(want["score"], cap)]
    ctx = strongest_ctx(640, 480, cap)
    ctx.pyramid_build(img)
    d_desc = torch.zeros((cap, 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.detect_dev()
    ctx.describe_detected_dev(d_desc.data_ptr())
    ctx.sync()
    assert np.array_equal(d_desc.cpu().numpy(), oracle.clatch(pyr, sel))
    ctx.close()


def test_batch_every_camera_its_own_cutoff(oracle):
    """clc_detect_batch_dev, 4 cameras, different frames: a cutoff per camera; the frames in another order (nothing stale); the same
    context switched back to CLC_SELECT_FIRST gives the default again, and selecting once more the selection."""
    import torch
    from coloc_amd import SELECT_FIRST, SELECT_STRONGEST
    from coloc_amd.abi import KP_DTYPE
    W, H, n, cap = 640, 480, 4, 2000
    imgs = [synth.rect_image(W, H, seed=1200 + c, noise_sigma=2.0 + c) for c in range(n)]
    want = [oracle_detect(oracle, im) for im in imgs]
    cuts = [cutoff_of(w["score"], cap) for _, w in want]
    assert len({c[0] for c in cuts}) == n                                       # four different cutoffs
    assert all(1 <= kept < tied for _, _, tied, kept in cuts)                   # each cuts through its tied group
    ctx = strongest_ctx(W, H, cap)
    d_kps = [torch.zeros((cap, 20), dtype=torch.uint8, device="cuda") for _ in range(n)]
    d_cnt = [torch.zeros((2,), dtype=torch.int32, device="cuda") for _ in range(n)]
    d_desc = [torch.zeros((cap, 64), dtype=torch.uint8, device="cuda") for _ in range(n)]
    runs = [(SELECT_STRONGEST, list(range(n))), (SELECT_STRONGEST, [2, 0, 3, 1]), (SELECT_FIRST, list(range(n))),
            (SELECT_STRONGEST, list(reversed(range(n))))]
    for mode, order in runs:
        ctx.set_keypoint_selection(mode)
        d_imgs = [torch.from_numpy(imgs[c]).cuda() for c in order]
        torch.cuda.synchronize()
        ctx.detect_batch_dev([t.data_ptr() for t in d_imgs], W, H, W, [t.data_ptr() for t in d_kps], [t.data_ptr() for t in d_cnt],
                             [t.data_ptr() for t in d_desc])
        ctx.sync()
        for b, c in enumerate(order):
            pyr, w = want[c]
            exp = w[select_strongest(w["score"], cap)] if mode == SELECT_STRONGEST else w[:cap]
            cnt = d_cnt[b].cpu().numpy()
            assert cnt[0] == cap and cnt[1] == len(w)
            kps = d_kps[b].cpu().numpy().reshape(-1).view(KP_DTYPE)[:cap]
            assert same_kps(kps, exp), (mode, order, b)
            assert np.array_equal(d_desc[b].cpu().numpy(), oracle.clatch(pyr, exp))
    ctx.close()


def test_host_front_end(oracle):
    """clc_detect_and_describe and the one-synchronisation view (+ store): keypoints and descriptors of the selected."""
    img, pyr, want = uncapped(oracle, (640, 480, 1000))
    cap = 2000
    sel = want[select_strongest(want["score"], cap)]
    rows = oracle.clatch(pyr, sel)
    ctx = strongest_ctx(640, 480, cap)
    kps, desc, found = ctx.detect_and_describe(img)
    assert found == len(want) and same_kps(kps, sel) and np.array_equal(desc, rows)
    kps, desc, found, _ = ctx.detect_and_describe_published(img)
    assert found == len(want) and same_kps(kps, sel) and np.array_equal(desc, rows)
    ctx.close()


def test_policy_class_keep_strongest(tmp_path, oracle):
    """HIPDetector<bool>::keepStrongest(true) through the policy host (tests/host/select_driver.cpp): regions hold the selected
    keypoints' features and descriptors, keypointsFound() stays the uncapped count; keepStrongest(false) restores the default."""
    from test_policy_host import build_driver
    W, H, cap = 320, 240, 800
    exe = build_driver(str(tmp_path / "select_driver"), "select_driver.cpp")
    img = synth.rect_image(W, H, n_rect=150, seed=1000, noise_sigma=2.0)
    with open(tmp_path / "img0.pgm", "wb") as f:
        f.write(b"P5\n# synthetic\n%d %d\n255\n" % (W, H))
        f.write(img.tobytes())
    pyr, want = oracle_detect(oracle, img)
    assert len(want) > cap
    _, _, tied, kept = cutoff_of(want["score"], cap)
    assert 1 <= kept <= tied
    sel = want[select_strongest(want["score"], cap)]
    assert not same_kps(sel, want[:cap])
    out = subprocess.run([exe, str(tmp_path), str(W), str(H), str(cap)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    for tag, exp in (("strongest", sel), ("first", want[:cap]), ("again", sel)):
        kps = np.fromfile(tmp_path / ("kps_%s.bin" % tag), dtype=synth.KP_DTYPE)
        assert same_kps(kps, exp), tag
        assert np.array_equal(np.fromfile(tmp_path / ("desc_%s.bin" % tag), dtype=np.uint8).reshape(-1, 64), oracle.clatch(pyr, exp)), tag
        assert np.array_equal(np.fromfile(tmp_path / ("feat_%s.bin" % tag), dtype=np.float32).reshape(-1, 4), oracle.features_from_kps(exp)), tag
        assert int(np.fromfile(tmp_path / ("found_%s.bin" % tag), dtype=np.int32)[0]) == len(want)

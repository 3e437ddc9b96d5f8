"""The detector -> matcher descriptor hand-over, row for row.

A published block (clc_detect_store_descriptors, clc_desc_cache_publish) lets the host-pointer match entries skip its upload.  Under the
default mode a lookup compares the host block with a fold taken AT PUBLISH TIME: that proves the host rows have not changed since, never
that the device rows behind the entry equal them.  So every way of publishing must put the caller's exact rows on the device, and one
that does not must refuse.  The probe below reads a published block's device rows back through the sweep: query i's own row lies at
train i at distance 0, so any device row that differs from its host row changes `best` or the index of that query."""
import ctypes as C
import threading

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

W, H = 320, 240
IMG_A = dict(n_rect=150, seed=41, noise_sigma=2.0)       # ~2350 keypoints at fast_thresh 40
IMG_B = dict(n_rect=150, seed=42, noise_sigma=2.0)       # ~2500
IMG_SPARSE = dict(n_rect=30, seed=45, noise_sigma=2.0)   # ~640


def image(spec):
    return synth.rect_image(W, H, **spec)


_ORACLE = []


def oracle():
    if not _ORACLE:
        import oracle_lib
        _ORACLE.append(oracle_lib.Oracle())
    return _ORACLE[0]


def hits():
    from coloc_amd.abi import desc_cache_stats
    return desc_cache_stats()[0]


def live(handle):
    from coloc_amd.abi import desc_handle_live
    return desc_handle_live(handle)


def _differ(got, want, what):
    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]) | (got[2] != want[2]))[0]
    return ("%s: %d of %d queries differ from the oracle (device rows that are not their host rows), first %s; best got %s want %s"
            % (what, len(bad), len(want[0]), bad[:8].tolist(), got[1][bad[:8]].tolist(), want[1][bad[:8]].tolist()))


def assert_device_rows_are(ctx, block, must_hit):
    """The rows `ctx`'s host-pointer match entries read for numpy `block` are exactly its host rows, through clc_match_2nn (match,
    best and second, as query and as train set), clc_match_map and clc_match_pairs.  must_hit: True = every lookup of `block` was
    answered from the descriptor table, False = none was, None = not checked (another thread changes the table)."""
    o = oracle()
    assert block.dtype == np.uint8 and block.flags["C_CONTIGUOUS"] and block.ndim == 2
    copy = block.copy()                           # another address: always uploaded
    for q, t, what in ((copy, block, "published block as train set"), (block, copy, "published block as query set")):
        h0 = hits()
        got = ctx.match_2nn(q, t, 40, want_dist=True)
        d = hits() - h0
        want = o.k2nn(q, t, 40, want_dist=True)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), _differ(got, want, what)
        if must_hit is not None:
            assert d == (1 if must_hit else 0), "%s: %d hits, expected %s" % (what, d, "one" if must_hit else "none")
    ctx.set_map(copy)
    h0 = hits()
    got = ctx.match_map(block, 60)
    d = hits() - h0
    want = o.k2nn(block, copy, 60)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, "match_map: %d queries differ from the oracle, first %s" % (len(bad), bad[:8].tolist())
    if must_hit is not None:
        assert (d >= 1) if must_hit else (d == 0), "match_map: %d hits" % d
    h0 = hits()
    res = ctx.match_pairs([block, copy], [(0, 1), (1, 0)], 40)
    d = hits() - h0
    for r, w, what in ((res[0], o.k2nn(block, copy, 40), "block -> copy"), (res[1], o.k2nn(copy, block, 40), "copy -> block")):
        bad = np.nonzero(r != w)[0]
        assert len(bad) == 0, "match_pairs %s: %d queries differ from the oracle, first %s" % (what, len(bad), bad[:8].tolist())
    if must_hit is not None:
        assert (d >= 1) if must_hit else (d == 0), "match_pairs: %d hits" % d


def probe(ctx, block, verify, trust=None):
    """assert_device_rows_are under a verifying lookup and (trust not None) a trusting one; the context is left verifying."""
    try:
        ctx.desc_cache_mode("verify")
        assert_device_rows_are(ctx, block, verify)
        if trust is not None:
            ctx.desc_cache_mode("trust")
            assert_device_rows_are(ctx, block, trust)
    finally:
        ctx.desc_cache_mode("verify")


# -- the raw entry points, with their status codes and handles

def view(ctx, img):
    """clc_detect_and_describe_view: (keypoints, a copy of the staged descriptor rows)."""
    from coloc_amd.abi import KP_DTYPE, _p
    img = np.ascontiguousarray(img, dtype=np.uint8)
    pk, pd, n, found = C.c_void_p(), C.c_void_p(), C.c_int(), C.c_int()
    ctx._chk(ctx.lib.clc_detect_and_describe_view(ctx.h, _p(img), W, H, C.byref(pk), C.byref(pd), C.byref(n), C.byref(found)))
    kps = np.zeros(n.value, dtype=KP_DTYPE)
    rows = np.zeros((n.value, 64), dtype=np.uint8)
    if n.value:
        C.memmove(kps.ctypes.data, pk, n.value * KP_DTYPE.itemsize)
        C.memmove(rows.ctypes.data, pd, n.value * 64)
    return kps, rows


def store(ctx, h, n):
    """clc_detect_store_descriptors(ctx, h, n): (status, handle)."""
    from coloc_amd.abi import DescHandle
    handle = DescHandle()
    rc = ctx.lib.clc_detect_store_descriptors(ctx.h, C.c_void_p(h.ctypes.data), int(n), C.byref(handle))
    return rc, handle


def publish(ctx, h, d_src=None):
    """clc_desc_cache_publish(ctx, d_src, h, len(h)): (status, handle)."""
    from coloc_amd.abi import DescHandle
    assert h.dtype == np.uint8 and h.flags["C_CONTIGUOUS"]
    handle = DescHandle()
    rc = ctx.lib.clc_desc_cache_publish(ctx.h, d_src, C.c_void_p(h.ctypes.data), int(h.shape[0]), C.byref(handle))
    return rc, handle


def publish_ok(ctx, h, d_src=None):
    rc, handle = publish(ctx, h, d_src)
    assert rc == 0, ctx.lib.clc_last_error_string(ctx.h)
    assert live(handle)
    return handle


def refused(ctx, rc, handle, code):
    assert rc == code, "status %d, expected %d (%s)" % (rc, code, ctx.lib.clc_last_error_string(ctx.h).decode())
    assert not live(handle) and handle.host is None and handle.count == 0


def described_by_oracle(img, kps):
    o = oracle()
    return o.clatch(o.pyramid(img), kps)


def device_copy(rows):
    """The rows in a device buffer of the caller's (the d_src form), finished before the library's own stream reads them."""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()          # the copy runs on torch's stream, the publish copy on the context's non-blocking one
    return d


@pytest.fixture(scope="module")
def ctxs():
    from coloc_amd import Context
    det = Context(device=0, width=W, height=H, maxkp=4096)                    # detector + matcher (case Q probes with it)
    mat = Context(device=0, width=W, height=H, maxkp=4096, detector=False)
    yield det, mat
    det.close(); mat.close()


@pytest.fixture(autouse=True)
def fresh_table(ctxs):
    from coloc_amd.abi import load_library
    for c in ctxs:
        c.desc_cache_mode("verify")
    load_library().clc_desc_cache_clear()
    yield


# -- A .. D: the publications that were right before, and stay right

def test_view_and_store_publishes_the_frame(ctxs):
    """A: view + store (HIPDetector's path)."""
    det, mat = ctxs
    img = image(IMG_A)
    kps, desc, found, handle = det.detect_and_describe_published(img)
    assert len(desc) > 1000 and live(handle)
    assert np.array_equal(desc, described_by_oracle(img, kps))
    probe(mat, desc, verify=True, trust=True)
    assert live(handle)


def test_partial_store_then_null_publish_of_the_prefix(ctxs):
    """B: store(h, n - 1) copies without publishing; publish(NULL, h[:n - 1]) then publishes the staged prefix."""
    det, mat = ctxs
    _, rows = view(det, image(IMG_A))
    n = len(rows)
    h = np.zeros((n, 64), dtype=np.uint8)
    rc, handle = store(det, h, n - 1)
    assert rc == 0 and not live(handle)
    assert np.array_equal(h[:n - 1], rows[:n - 1])
    probe(mat, h[:n - 1], verify=False, trust=False)
    publish_ok(det, h[:n - 1])
    probe(mat, h[:n - 1], verify=True, trust=True)


def test_stored_frame_published_again_at_a_second_address(ctxs):
    """C: the same staged frame stored at h1 and published from the pinned rows at a copy h2."""
    det, mat = ctxs
    _, rows = view(det, image(IMG_A))
    h1 = np.zeros_like(rows)
    rc, handle1 = store(det, h1, len(rows))
    assert rc == 0 and live(handle1)
    h2 = h1.copy()
    handle2 = publish_ok(det, h2)
    probe(mat, h1, verify=True, trust=True)
    probe(mat, h2, verify=True, trust=True)
    assert live(handle1) and live(handle2)


def test_detect_and_describe_then_null_publish(ctxs):
    """D: detect_and_describe + publish(NULL, desc)."""
    det, mat = ctxs
    img = image(IMG_A)
    kps, desc, _ = det.detect_and_describe(img)
    assert np.array_equal(desc, described_by_oracle(img, kps))
    publish_ok(det, desc)
    probe(mat, desc, verify=True, trust=True)


# -- E .. I: NULL is this context's last described rows, or it fails

@pytest.mark.parametrize("edit", ["row0_and_middle", "middle_only"])
def test_edited_block_is_refused(ctxs, edit):
    """E: after D, the host edits the block and publishes it again with NULL.  The device holds the rows of the frame, not the edited
    ones: CLC_ERR_STATE, nothing published, and the first publication dies at the next lookup."""
    from coloc_amd.abi import CLC_ERR_STATE
    det, mat = ctxs
    _, desc, _ = det.detect_and_describe(image(IMG_A))
    first = publish_ok(det, desc)
    n = len(desc)
    sampled = {(i + 1) * n // 17 for i in range(16)} | {0, n - 1}
    mid = next(r for r in range(n // 3, n) if r not in sampled and r - 1 not in sampled and r + 1 not in sampled)
    if edit == "row0_and_middle":
        desc[0, 3] ^= 0xFF
    desc[mid, 20] ^= 0x04
    rc, handle = publish(det, desc)
    probe(mat, desc, verify=False, trust=False)     # (first: a library that does publish here names the stale rows)
    refused(det, rc, handle, CLC_ERR_STATE)
    assert not live(first)


@pytest.mark.parametrize("maxkp,frame_b", [(400, IMG_B), (4096, IMG_SPARSE)], ids=["same_count", "fewer_rows"])
def test_view_frame_then_device_flow(ctxs, maxkp, frame_b):
    """F: frame A through the view, frame B through pyramid_build + detect + describe_detected_dev(NULL), then publish(NULL, hB):
    B's rows, whether B has as many rows as A (both saturate maxkp) or fewer."""
    from coloc_amd import Context
    _, mat = ctxs
    det = Context(device=0, width=W, height=H, maxkp=maxkp, matcher=False)
    try:
        _, rows_a = view(det, image(IMG_A))
        img_b = image(frame_b)
        det.pyramid_build(img_b)
        kps_b, _ = det.detect()
        det.describe_detected_dev(None)
        h_b = described_by_oracle(img_b, kps_b)
        if maxkp == 400:
            assert len(rows_a) == len(h_b) == 400
        else:
            assert len(h_b) < len(rows_a)
        publish_ok(det, h_b)
        probe(mat, h_b, verify=True, trust=True)
    finally:
        det.close()


def test_view_frame_then_host_describe(ctxs):
    """G: frame A through the view, then clc_describe of other keypoints on another pyramid: NULL publishes the described rows;
    more rows than were described is CLC_ERR_BAD_ARG."""
    from coloc_amd.abi import CLC_ERR_BAD_ARG
    det, mat = ctxs
    _, rows_a = view(det, image(IMG_A))
    img_b = image(IMG_B)
    det.pyramid_build(img_b)
    kps_b = synth.random_keypoints(300, W, H, seed=4242)
    desc_b = det.describe(kps_b)
    assert np.array_equal(desc_b, described_by_oracle(img_b, kps_b)) and len(desc_b) < len(rows_a)
    publish_ok(det, desc_b)
    probe(mat, desc_b, verify=True, trust=True)
    longer = np.vstack([desc_b, synth.random_descriptors(1, seed=4243)])
    rc, handle = publish(det, longer)
    refused(det, rc, handle, CLC_ERR_BAD_ARG)
    probe(mat, longer, verify=False, trust=False)


@pytest.mark.parametrize("call", ["describe_detected_dev", "detect_batch_dev", "describe_batch_dev", "describe_match_pair_dev"])
def test_caller_buffer_describe_leaves_nothing_to_publish(ctxs, call):
    """H: frame A through the view, then a describing call into caller buffers: the context holds no rows of its last describing
    call, so publish(NULL) and store both fail with CLC_ERR_STATE and nothing is published.  A new view publishes again."""
    import torch
    from coloc_amd.abi import CLC_ERR_STATE
    det, mat = ctxs
    img = image(IMG_A)
    _, rows_a = view(det, img)
    n = len(rows_a)
    maxkp = 4096
    img_d = torch.from_numpy(img).cuda()
    img2_d = torch.from_numpy(image(IMG_B)).cuda()
    kps = synth.random_keypoints(300, W, H, seed=77)
    kps_d = torch.from_numpy(kps.view(np.uint8).copy()).cuda()
    desc_d = [torch.empty(maxkp * 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    kps_out = torch.empty(maxkp * 20, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    match = torch.empty(300, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if call == "describe_detected_dev":
        det.describe_detected_dev(desc_d[0].data_ptr())
    elif call == "detect_batch_dev":
        det.detect_batch_dev([img_d.data_ptr()], W, H, W, [kps_out.data_ptr()], [cnt.data_ptr()], [desc_d[0].data_ptr()])
    elif call == "describe_batch_dev":
        det.describe_batch_dev([img_d.data_ptr()], W, H, W, [kps_d.data_ptr()], [300], [desc_d[0].data_ptr()])
    else:
        det.describe_match_pair_dev([img_d.data_ptr(), img2_d.data_ptr()], W, H, W, [kps_d.data_ptr(), kps_d.data_ptr()], [300, 300],
                                    [desc_d[0].data_ptr(), desc_d[1].data_ptr()], 40, match.data_ptr())
    det.sync()
    h_a = rows_a.copy()
    rc, handle = publish(det, h_a)
    refused(det, rc, handle, CLC_ERR_STATE)
    h = np.zeros_like(rows_a)
    rc, handle = store(det, h, n)
    refused(det, rc, handle, CLC_ERR_STATE)
    probe(mat, h_a, verify=False)
    kps2, desc2, _, handle = det.detect_and_describe_published(img)
    assert live(handle) and np.array_equal(desc2, rows_a)
    probe(mat, desc2, verify=True)


def test_device_flow_on_a_fresh_context(ctxs):
    """I: no view ever ran.  detect + describe_detected_dev(NULL): NULL publishes the detected rows; describe_dev into the context's
    own array: its n rows."""
    import torch
    from coloc_amd import Context
    _, mat = ctxs
    det = Context(device=0, width=W, height=H, maxkp=4096, matcher=False)
    try:
        img = image(IMG_A)
        det.pyramid_build(img)
        kps, _ = det.detect()
        det.describe_detected_dev(None)
        h = described_by_oracle(img, kps)
        publish_ok(det, h)
        probe(mat, h, verify=True, trust=True)
        # describe_dev with the context's own descriptor array as the target
        _, _, d_own = det.detect_buffers()
        kps2 = synth.random_keypoints(500, W, H, seed=98)
        kps2_d = torch.from_numpy(kps2.view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        det.describe_dev(kps2_d.data_ptr(), len(kps2), d_own)
        h2 = described_by_oracle(img, kps2)
        publish_ok(det, h2)
        probe(mat, h2, verify=True, trust=True)
    finally:
        det.close()


def test_device_flow_more_rows_than_detected_is_refused(ctxs):
    """I: publish(NULL) of the detected count + 1 rows after describe_detected_dev(NULL) is CLC_ERR_BAD_ARG, nothing published (the
    rows past the count are not described rows; past maxkp they would not even lie in the context's array)."""
    from coloc_amd import Context
    from coloc_amd.abi import CLC_ERR_BAD_ARG
    _, mat = ctxs
    det = Context(device=0, width=W, height=H, maxkp=4096, matcher=False)
    try:
        img = image(IMG_A)
        det.pyramid_build(img)
        kps, _ = det.detect()
        assert 0 < len(kps) < 4096
        det.describe_detected_dev(None)
        longer = np.vstack([described_by_oracle(img, kps), synth.random_descriptors(1, seed=99)])
        rc, handle = publish(det, longer)
        refused(det, rc, handle, CLC_ERR_BAD_ARG)
        probe(mat, longer, verify=False, trust=False)
        publish_ok(det, longer[:-1])                # the described rows themselves still publish
        probe(mat, longer[:-1], verify=True)
    finally:
        det.close()


# -- J .. P: modes, owners, addresses, eviction

def test_view_under_off_then_publish_under_verify(ctxs):
    """J: a frame staged while the context published nothing (mode off) is published from the pinned rows later -- also when an
    earlier frame of as many rows, staged under verify and never stored, had left its rows in a reserved table block."""
    from coloc_amd import Context
    _, mat = ctxs
    det = Context(device=0, width=W, height=H, maxkp=400, matcher=False)
    try:
        _, rows_b = view(det, image(IMG_B))                     # verify: written into a reserved block of the table, not stored
        det.desc_cache_mode("off")
        _, desc, _, handle = det.detect_and_describe_published(image(IMG_A))
        assert not live(handle) and len(desc) == len(rows_b) == 400 and not np.array_equal(desc, rows_b)
        det.desc_cache_mode("verify")
        publish_ok(det, desc)
        probe(mat, desc, verify=True, trust=True)
    finally:
        det.close()


def test_trusting_publisher(ctxs):
    """K: (a) publish(NULL) from a trusting context carries no fold: verifying lookups miss, trusting ones hit; (b) store always folds."""
    det, mat = ctxs
    det.desc_cache_mode("trust")
    _, desc, _ = det.detect_and_describe(image(IMG_A))
    publish_ok(det, desc)
    probe(mat, desc, verify=False, trust=True)
    _, desc_b, _, handle = det.detect_and_describe_published(image(IMG_B))
    assert live(handle)
    probe(mat, desc_b, verify=True, trust=True)


def test_publication_dies_with_its_context(ctxs):
    """L: a block published by another context is read until that context is destroyed."""
    from coloc_amd import Context
    _, mat = ctxs
    det = Context(device=0, width=W, height=H, maxkp=4096, matcher=False)
    try:
        _, desc, _, handle = det.detect_and_describe_published(image(IMG_A))
        probe(mat, desc, verify=True, trust=True)
    finally:
        det.close()
    assert not live(handle)
    probe(mat, desc, verify=False, trust=False)


def test_second_publication_of_an_address_wins(ctxs):
    """M: two contexts publish the same host address: the first publication dies, lookups read the second's rows."""
    det, mat = ctxs
    _, rows = view(det, image(IMG_A))
    n = len(rows)
    block = synth.random_descriptors(n, seed=600)
    d = device_copy(block)
    first = publish_ok(mat, block, d_src=d.data_ptr())
    probe(mat, block, verify=True)
    rc, second = store(det, block, n)
    assert rc == 0 and live(second) and not live(first)
    assert np.array_equal(block, rows)
    probe(mat, block, verify=True, trust=True)


@pytest.mark.parametrize("maxkp,frames", [(400, (IMG_A, IMG_B)), (4096, (IMG_A, IMG_SPARSE))], ids=["same_count", "fewer_rows"])
def test_regions_block_reused_for_the_next_frame(ctxs, maxkp, frames):
    """N: one host block receives frame A and then frame B through view + store (regions[idx] reused): A's publication dies, B's
    stands and its rows are B's -- also when both frames have the same count."""
    from coloc_amd import Context
    _, mat = ctxs
    det = Context(device=0, width=W, height=H, maxkp=maxkp, matcher=False)
    try:
        block = np.zeros((maxkp, 64), dtype=np.uint8)
        _, rows_a = view(det, image(frames[0]))
        rc, handle_a = store(det, block, len(rows_a))
        assert rc == 0 and live(handle_a)
        probe(mat, block[:len(rows_a)], verify=True)
        _, rows_b = view(det, image(frames[1]))
        if maxkp == 400:
            assert len(rows_a) == len(rows_b) == 400
        rc, handle_b = store(det, block, len(rows_b))
        assert rc == 0 and live(handle_b) and not live(handle_a)
        assert np.array_equal(block[:len(rows_b)], rows_b)
        probe(mat, block[:len(rows_b)], verify=True, trust=True)
    finally:
        det.close()


def test_more_blocks_than_entries(ctxs):
    """O: 40 blocks published through d_src into a table of 32 entries: every lookup is exact, and hits exactly when its handle lives."""
    _, mat = ctxs
    blocks, handles = [], []
    for i in range(40):
        b = synth.random_descriptors(100 + 23 * i, seed=700 + i)
        d = device_copy(b)
        handles.append(publish_ok(mat, b, d_src=d.data_ptr()))
        blocks.append(b)
    alive = [live(h) for h in handles]
    k = alive.index(True)
    # the least recently published ones went (a block a front end holds reserved is not taken, so a few fewer than 32 may live)
    assert all(alive[k:]) and 24 <= 40 - k <= 32, alive
    for b, a in zip(blocks, alive):
        assert_device_rows_are(mat, b, a)


def test_table_cleared_between_view_and_store(ctxs):
    """P: clc_desc_cache_clear between view and store: the reserved block survives, store publishes it."""
    from coloc_amd.abi import load_library
    det, mat = ctxs
    _, rows = view(det, image(IMG_A))
    load_library().clc_desc_cache_clear()
    h = np.zeros_like(rows)
    rc, handle = store(det, h, len(rows))
    assert rc == 0 and live(handle)
    probe(mat, h, verify=True, trust=True)


def test_publish_and_probe_from_two_threads(ctxs):
    """Q: one thread publishes 60 fresh blocks through d_src, over and over until the other is done (eviction pressure); the other
    stores frames and probes its blocks 60 times.  ctypes drops the GIL, so the table is used from both at once: every probe exact,
    no error."""
    import torch
    det, mat = ctxs
    errors = []
    done = threading.Event()
    imgs = [image(dict(IMG_SPARSE, seed=45 + i)) for i in range(3)]
    blocks = [synth.random_descriptors(200 + i, seed=800 + i) for i in range(60)]
    d_blocks = [torch.from_numpy(b).cuda() for b in blocks]
    torch.cuda.synchronize()          # the copies run on torch's stream, the publish copies on the context's non-blocking one
    published = [0]

    def publisher():
        try:
            while published[0] < len(blocks) or not done.is_set():
                i = published[0] % len(blocks)
                mat.desc_cache_publish(blocks[i], d_src=d_blocks[i].data_ptr())
                published[0] += 1
        except BaseException as e:                  # noqa: BLE001 (reported by the main thread)
            errors.append(("publisher", repr(e)))

    def prober():
        try:
            desc = None
            for i in range(60):
                if i % 10 == 0:
                    _, desc, _, handle = det.detect_and_describe_published(imgs[(i // 10) % 3])
                assert_device_rows_are(det, desc, None)
        except BaseException as e:                  # noqa: BLE001
            errors.append(("prober", repr(e)))
        finally:
            done.set()

    threads = [threading.Thread(target=publisher), threading.Thread(target=prober)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=240)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"
    assert not errors, errors
    assert published[0] >= len(blocks)

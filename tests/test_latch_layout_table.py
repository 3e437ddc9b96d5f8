"""The generated CLATCH slot table (coloc_amd/csrc/latch_layout_swap.inc over the geometry of latch_layout.inc), recomputed here the way
clatch.hip's make_slot_table does it: every learned triplet is evaluated exactly once, the un-permute records lead back
to descriptor order, the a <-> c exchange flags are consistent, every (round, patch kind) group that the kernel reads with the 8-byte
ds_read_b64 form lies on 8-byte aligned rows in all 64 lanes, and the four window copies still fit twelve waves per CU."""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coloc_amd", "csrc")
MAX_WAVE_BYTES = 12688          # 160 KB of LDS / 12 waves per CU, less the allocation granule


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def _macro_ints(text, name):
    """the integers of `#define name ...` (a macro's lines run on while they end in a backslash); None if there is no such macro"""
    m = re.search(r"^#define\s+%s\b" % name, text, re.M)
    if not m:
        return None
    lines = []
    for line in text[m.end():].split("\n"):
        lines.append(line)
        if not line.rstrip().endswith("\\"):
            break
    return [int(v) for v in re.findall(r"-?\d+", " ".join(lines))]


def _layout():
    geo, tab = _text("latch_layout.inc"), _text("latch_layout_swap.inc")
    g = {k: _macro_ints(geo, "LATCH_" + k) for k in ("ROW0", "COL0", "STRIDE", "NROWS", "WAVE_BYTES", "COPY_BASES")}
    pattern = [tuple(int(v) for v in m) for m in re.findall(r"^\{(\d+),(\d+), (\d+),(\d+), (\d+),(\d+)\}", _text("latch_pattern.inc"), re.M)]
    shift4 = _macro_ints(tab, "LATCH_COPY_SHIFT4") or [0, 0, 0, 0]
    planned = _macro_ints(tab, "LATCH_ROUND_B64") or [0] * 24
    slots = _macro_ints(tab, "LATCH_SLOT_TRIPLET_EX")
    return g, pattern, shift4, np.array(planned).reshape(8, 3), slots


def _addr(g, shift4, row, col):
    p = (row - g["ROW0"][0]) * g["STRIDE"][0] + (col - g["COL0"][0])
    return g["COPY_BASES"][p & 3] + 4 * shift4[p & 3] + (p & ~3)


def _records(g, pattern, shift4, slots):
    """rec[slot] = (a, b, c, exchanged) as the kernel loads them, src[n] = (lane * 4) | (round << 8) for output bit n"""
    rec, src = [], {}
    for slot, v in enumerate(slots):
        n, ex = v & 511, (v >> 10) & 1
        a, b, c = (_addr(g, shift4, pattern[n][2 * k], pattern[n][2 * k + 1]) for k in range(3))
        rec.append((c, b, a, 1) if ex else (a, b, c, 0))
        src[n] = ((slot & 63) << 2) | ((slot >> 6) << 8)
    return rec, src


def test_sizes_parse():
    g, pattern, shift4, planned, slots = _layout()
    assert len(pattern) == 512 and len(slots) == 512 and len(shift4) == 4 and planned.shape == (8, 3)
    assert all(0 <= r <= 56 and 0 <= c <= 56 for t in pattern for r, c in (t[0:2], t[2:4], t[4:6]))
    assert all(v & ~(511 | 1 << 10) == 0 for v in slots), "only the triplet and the exchange bit (no row rotation in the shipped kernel)"


def test_every_triplet_is_placed_exactly_once():
    _, _, _, _, slots = _layout()
    assert sorted(v & 511 for v in slots) == list(range(512))


def test_unpermute_record_points_at_the_slot_that_evaluates_the_triplet():
    g, pattern, shift4, _, slots = _layout()
    _, src = _records(g, pattern, shift4, slots)
    assert sorted(src) == list(range(512))
    for n in range(512):
        lane, rnd = (src[n] & 0xFF) >> 2, src[n] >> 8
        assert 0 <= lane < 64 and 0 <= rnd < 8
        assert slots[rnd * 64 + lane] & 511 == n, "output bit %d" % n


def test_exchange_flag_is_consistent():
    g, pattern, shift4, _, slots = _layout()
    rec, _ = _records(g, pattern, shift4, slots)
    for slot, (a, b, c, ex) in enumerate(rec):
        n = slots[slot] & 511
        pa, pb, pc = (_addr(g, shift4, pattern[n][2 * k], pattern[n][2 * k + 1]) for k in range(3))
        assert b == pb and ((a, c) == (pc, pa) if ex else (a, c) == (pa, pc))
        assert ex == (slots[slot] >> 10) & 1
        assert max(a, b, c) < 0x8000, "bit 15 of the first address carries the exchange flag"


def test_groups_read_with_the_8_byte_form_are_8_byte_aligned_in_every_lane():
    """The groups a table states in LATCH_ROUND_B64 (tools/latch_anneal.c's b64 searches) are the ones a kernel may read with ds_read_b64:
    exactly those must have all 64 addresses = 0 mod 8.  The shipped table states none -- the kernel reads every group as dword pairs
    (profiles/clatch_two_paths.txt) -- and then must not have one by accident either, or the statement in its header would be wrong."""
    g, pattern, shift4, planned, slots = _layout()
    rec, _ = _records(g, pattern, shift4, slots)
    addr = np.array([r[:3] for r in rec]).reshape(8, 64, 3)
    assert (addr % 4 == 0).all()
    derived = (addr % 8 == 0).all(axis=1)                       # a group may use the 8-byte form only if every lane is aligned
    assert np.array_equal(derived, planned != 0), "the table does not deliver the groups its generator states"
    for r in range(8):
        for k in range(3):
            if derived[r, k]:
                assert not (addr[r, :, k] & 4).any()
    # all eight rows of a patch keep the alignment of the first one
    assert g["STRIDE"][0] % 8 == 0 and all((b + 4 * s) % 4 == 0 for b, s in zip(g["COPY_BASES"], shift4))


def test_four_copies_fit_twelve_waves_and_keep_their_gaps():
    g, _, shift4, _, _ = _layout()
    win = g["NROWS"][0] * g["STRIDE"][0]                        # 4 * kWinDwords
    base = [b + 4 * s for b, s in zip(g["COPY_BASES"], shift4)]
    assert g["WAVE_BYTES"][0] <= MAX_WAVE_BYTES
    assert base[0] == 0 and all(s in (0, 1) for s in shift4)
    # clatch.hip's static_assert: the copy phase reads 8 bytes at the window's last dword, and no copy may overlap what it reads or another copy
    assert base[1] >= win + 8 and base[2] >= base[1] + win + 8 and base[3] >= base[2] + win + 8
    assert g["WAVE_BYTES"][0] >= base[3] + win

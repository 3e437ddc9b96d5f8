"""The CLATCH slot table under the merged-read model, recomputed from the three .inc files alone (no call into tools/latch_anneal.c).

The LDS serves the lanes of a half-wave that read the SAME address with one access, so two triplets that share a patch -- the 1 536 patch
uses of the learned pattern sit at only 1 113 positions -- cost nothing extra when they sit in one half-wave of one round and read that
patch as the same kind (a-or-c after the slot's exchange flag, or anchor).  The conflict degree of a half-wave read is then the largest
number of DISTINCT addresses on one of the 32 banks; the plain model counts lanes.  The table states both sums and its co-location count;
a 200 M-move search under the merged model reaches a merged sum of 63 (the table searched under the plain model: 71), so a shipped table
above 64 means that search was not run."""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coloc_amd", "csrc")
BANKS = 32


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def _macro(text, name):
    m = re.search(r"^#define\s+%s\b" % name, text, re.M)
    assert m, "no macro %s" % name
    lines = []
    for line in text[m.end():].split("\n"):
        lines.append(line)
        if not line.rstrip().endswith("\\"):
            break
    return [int(v) for v in re.findall(r"-?\d+", " ".join(lines))]


def _reads():
    """pos[round, lane, kind] = (row, col) of the patch the slot reads as kind 0 / 1 / 2 (the exchange flag swaps a and c), addr[...] its LDS address"""
    geo, tab = _text("latch_layout.inc"), _text("latch_layout_swap.inc")
    row0, col0, stride = (_macro(geo, "LATCH_" + k)[0] for k in ("ROW0", "COL0", "STRIDE"))
    bases = _macro(geo, "LATCH_COPY_BASES")
    pattern = [tuple(int(v) for v in m) for m in re.findall(r"^\{(\d+),(\d+), (\d+),(\d+), (\d+),(\d+)\}", _text("latch_pattern.inc"), re.M)]
    slots = _macro(tab, "LATCH_SLOT_TRIPLET_EX")
    assert len(pattern) == 512 and len(slots) == 512 and len(bases) == 4
    pos = np.zeros((8, 64, 3, 2), np.int64)
    addr = np.zeros((8, 64, 3), np.int64)
    for slot, v in enumerate(slots):
        n, ex = v & 511, (v >> 10) & 1
        for k in range(3):
            kk = 2 - k if (ex and k != 1) else k
            r, c = pattern[n][2 * kk], pattern[n][2 * kk + 1]
            p = (r - row0) * stride + (c - col0)
            pos[slot >> 6, slot & 63, k] = (r, c)
            addr[slot >> 6, slot & 63, k] = bases[p & 3] + (p & ~3)
    return tab, pattern, pos, addr


def _groups(addr):
    for r in range(8):
        for h in range(2):
            for k in range(3):
                yield r, h, k, addr[r, 32 * h:32 * h + 32, k]


def _sums(addr):
    plain = merged = coloc = 0
    for _, _, _, a in _groups(addr):
        bank = (a // 4) % BANKS
        plain += max(np.bincount(bank, minlength=BANKS))
        merged += max(len(set(a[bank == b].tolist())) for b in range(BANKS))
        coloc += len(a) - len(set(a.tolist()))              # lanes whose address a lower lane of the group already reads
    return int(plain), int(merged), int(coloc)


def test_the_pattern_repeats_patch_positions():
    _, pattern, _, _ = _reads()
    uses = [t[2 * k:2 * k + 2] for t in pattern for k in range(3)]
    assert len(uses) == 1536 and len(set(uses)) == 1113


def test_stated_sums_are_the_recomputed_ones():
    tab, _, _, addr = _reads()
    plain, merged, coloc = _sums(addr)
    assert _macro(tab, "LATCH_DEGREE_PLAIN") == [plain]
    assert _macro(tab, "LATCH_DEGREE_MERGED") == [merged]
    assert _macro(tab, "LATCH_COLOCATIONS") == [coloc]
    assert 48 <= merged <= plain


def test_merged_sum_is_what_a_merged_search_reaches():
    _, _, _, addr = _reads()
    assert _sums(addr)[1] <= 64


def test_co_located_lanes_read_equal_addresses():
    """pairs are found by PATCH POSITION (after the exchange flag); each must be one LDS address -- and no two different patches may share one"""
    _, _, pos, addr = _reads()
    pairs = 0
    for r in range(8):
        for h in range(2):
            for k in range(3):
                lanes = range(32 * h, 32 * h + 32)
                for i in lanes:
                    for j in range(32 * h, i):
                        same = tuple(pos[r, i, k]) == tuple(pos[r, j, k])
                        assert same == (addr[r, i, k] == addr[r, j, k]), (r, i, j, k)
                        pairs += same
    plain, merged, coloc = _sums(addr)
    assert pairs >= coloc and (coloc > 0) == (pairs > 0)
    assert merged == plain or coloc > 0                     # only co-locations can make the merged sum smaller

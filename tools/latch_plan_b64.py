#!/usr/bin/env python3
"""Plan the 8-byte-aligned (round, patch kind) groups of clatch_kernel's slot table: the starting point of tools/latch_anneal.c's
constrained search (its tenth argument).

A group = the 64 lanes of one unrolled round reading one patch kind (a, b or c).  It may use the full-rate ds_read_b64 form only if all 64
patch addresses are multiples of 8.  In the four-copy layout a patch at window byte p lies at COPY_BASE[p & 3] + (p & ~3), so it is
8-byte aligned iff bit 2 of p is clear -- or set, if that copy's base is moved by 4 bytes (the shift mask).  With the a <-> c role exchange
a triplet may offer its c patch where a round wants an aligned a.

For every shift mask this tool finds the round types (which kinds a round keeps aligned) that maximise the number of aligned groups
and still admit an assignment of all 512 triplets (a flow over the eight alignment classes), and writes for the best mask

    <shift mask>
    8 lines "fa fb fc"          the planned groups of round r
    512 values                  slot r*64+l -> triplet | (exchanged << 10)

usage: tools/latch_plan_b64.py out.plan [mask]
"""
import itertools
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW0 = COL0 = 5
STRIDE = 56
TYPES = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)]     # c-only / b+c are a-only / a+b with every triplet exchanged


def pattern():
    rows = []
    for line in open(os.path.join(ROOT, "coloc_amd", "csrc", "latch_pattern.inc")):
        m = re.match(r"\{(\d+),(\d+), (\d+),(\d+), (\d+),(\d+)\}", line)
        if m:
            rows.append(tuple(int(v) for v in m.groups()))
    assert len(rows) == 512
    return rows


def aligned(row, col, mask):
    p = (row - ROW0) * STRIDE + (col - COL0)
    return (((p >> 2) & 1) ^ ((mask >> (p & 3)) & 1)) == 0


def fits(cls, typ):
    """0: not at all, 1: as it is, 2: only with a and c exchanged"""
    if all(c or not t for c, t in zip(cls, typ)):
        return 1
    ex = (cls[2], cls[1], cls[0])
    return 2 if all(c or not t for c, t in zip(ex, typ)) else 0


def flow(count, types):
    """classes -> rounds, 64 per round (Edmonds-Karp on source -> class -> round -> sink); returns take[class, round] or None"""
    classes = sorted(count)
    nr = len(types)
    S, T = "s", "t"
    cap = {}
    def edge(u, v, c):
        cap[u, v] = c; cap.setdefault((v, u), 0)
    for c in classes:
        edge(S, c, count[c])
        for r, t in enumerate(types):
            if fits(c, t):
                edge(c, r, 64)
    for r in range(nr):
        edge(r, T, 64)
    adj = {}
    for u, v in cap:
        adj.setdefault(u, []).append(v)
    total = 0
    while True:
        prev = {S: None}
        queue = [S]
        for u in queue:
            for v in adj[u]:
                if v not in prev and cap[u, v] > 0:
                    prev[v] = u; queue.append(v)
        if T not in prev:
            break
        path = []; v = T
        while prev[v] is not None:
            path.append((prev[v], v)); v = prev[v]
        push = min(cap[e] for e in path)
        for u, v in path:
            cap[u, v] -= push; cap[v, u] += push
        total += push
    if total != 64 * nr:
        return None
    return {(c, r): (cap[r, c] if (c, r) in cap else 0) for c in classes for r in range(nr)}


def plan(pat, mask):
    cls_of = [tuple(int(aligned(t[2 * k], t[2 * k + 1], mask)) for k in range(3)) for t in pat]
    count = {}
    for c in cls_of:
        count[c] = count.get(c, 0) + 1
    for c in itertools.product((0, 1), repeat=3):
        count.setdefault(c, 0)
    combos = sorted(itertools.combinations_with_replacement(TYPES, 8), key=lambda ts: -sum(sum(t) for t in ts))
    for types in combos:                       # ends at the all-unaligned plan at the latest
        take = flow(count, types)
        if take:
            return cls_of, count, (sum(sum(t) for t in types), types, take)


def main():
    out = sys.argv[1]
    pat = pattern()
    masks = [int(sys.argv[2])] if len(sys.argv) > 2 else range(0, 16, 2)      # copy 0 sits at byte 0 of the region: it does not move
    found = None
    for mask in masks:
        cls_of, count, best = plan(pat, mask)
        print("shift mask %2d: classes (a, b, c aligned) %s -> %d aligned groups" % (mask, [count[c] for c in sorted(count)], best[0]))
        if not found or best[0] > found[2][0]:
            found = (mask, cls_of, best)
    mask, cls_of, (groups, types, take) = found
    pool = {}
    for n, c in enumerate(cls_of):
        pool.setdefault(c, []).append(n)
    slots = []
    for r, t in enumerate(types):
        row = []
        for c in sorted(pool):
            for _ in range(take[c, r]):
                n = pool[c].pop()
                row.append(n | ((fits(c, t) == 2) << 10))
        assert len(row) == 64
        slots.append(row)
    with open(out, "w") as f:
        f.write("%d\n" % mask)
        for t in types:
            f.write("%d %d %d\n" % t)
        for row in slots:
            f.write(" ".join(str(v) for v in row) + "\n")
    print("wrote %s: shift mask %d, %d of 24 groups aligned, round types %s" % (out, mask, groups, list(types)))


if __name__ == "__main__":
    main()

"""What msd_set_sorted has to produce (a helper module like merge_expect.py, not a test).

The expectation is defined HERE, with numpy: both inputs are unsigned views of their bit patterns plus a key type
(``sort_rows_expect``'s U32 .. F64); the concatenation ``[A; B]`` becomes order-preserving unsigned codes with
``sort_rows_expect.np_encode``; ``np.unique(return_index=True)`` of the codes gives the distinct values ascending and, per
value, the index of its FIRST occurrence in the concatenation (in A where A holds it), and ``np.isin`` says which side holds
a value.  Equality is equality of codes, that is of bits: for floats -0.0 and +0.0 differ and NaNs with equal bits are one
value -- NOT numpy's or torch's float equality.

:func:`tiles` is a numpy model of the kernels (csrc/msd_setops.hpp): the cut of the merged sequence into tiles along the
merge path -- ``search_expect.splits(..., right=True)`` is the split model -- and per tile the decision which elements are
kept, from the tile and a halo of three elements alone.

Plain module, no fixture: ``import set_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

import search_expect as S
import sort_rows_expect as E

KEY_TYPES = S.KEY_TYPES
INTERSECTION, UNION, DIFFERENCE, SYMMETRIC_DIFFERENCE = range(4)      # MSD_SET_* of include/msd_setops_hip.h
OPS = (INTERSECTION, UNION, DIFFERENCE, SYMMETRIC_DIFFERENCE)
OP_NAMES = {INTERSECTION: "intersection", UNION: "union", DIFFERENCE: "difference", SYMMETRIC_DIFFERENCE: "symmetric_difference"}


def bound(op, n, m):
    """the most results the operation can have"""
    return min(n, m) if op == INTERSECTION else n if op == DIFFERENCE else n + m


def _kept(in_a, in_b, op):
    return {INTERSECTION: in_a & in_b, UNION: in_a | in_b, DIFFERENCE: in_a & ~in_b, SYMMETRIC_DIFFERENCE: in_a ^ in_b}[op]


def expected(a_bits, b_bits, key_type, op):
    """``(keys, origin)``: the bit patterns of the result, ascending by code, and per result the index (uint64) in the
    concatenation [A; B] of the first occurrence of its value"""
    a_bits, b_bits = np.asarray(a_bits), np.asarray(b_bits)
    ca, cb = E.np_encode(a_bits, key_type), E.np_encode(b_bits, key_type)
    for name, c in (("A", ca), ("B", cb)):
        assert (c[1:] >= c[:-1]).all(), "%s is not ascending in the order of its type" % name
    cat = np.concatenate([a_bits, b_bits])
    values, first = np.unique(np.concatenate([ca, cb]), return_index=True)
    keep = _kept(np.isin(values, ca), np.isin(values, cb), op)
    return cat[first[keep]], first[keep].astype(np.uint64)


class _Window:
    """one side of a tile: reads are allowed inside [lo, hi) and at the halo indices"""

    def __init__(self, x, lo, hi, halo):
        self.x, self.lo, self.hi, self.halo = x, lo, hi, set(halo)

    def exists(self, i):
        return 0 <= i < len(self.x)

    def __getitem__(self, i):
        assert self.lo <= i < self.hi or i in self.halo, "index %d is neither in the tile [%d, %d) nor in its halo %s" % (i, self.lo, self.hi, sorted(self.halo))
        assert self.exists(i)
        return self.x[i]


def tiles(a_codes, b_codes, tile, op):
    """The model: ``(codes, origin)`` as the kernels compute them.  The splits are those of the merge (B after every A that
    is not larger).  In tile i, with a[a0, a1) and b[b0, b1) and the halo a[a0 - 1], b[b0 - 1], b[b1]:
    an A element is a candidate iff its predecessor in A differs, and matched iff b[b0 + |{b in tile : b < a}|] equals it;
    a B element is a candidate iff its predecessor in B differs, and matched iff a[a0 + |{a in tile : a <= b}| - 1] equals
    it.  Kept: matched A candidates (intersection), unmatched A candidates (difference), all A and the unmatched B candidates
    (union), unmatched candidates of both (symmetric difference), in the order of their merged ranks.  Asserts that every
    index read lies in the tile or is one of the three halo elements."""
    a_codes, b_codes = np.asarray(a_codes), np.asarray(b_codes)
    n, m = len(a_codes), len(b_codes)
    sa, sb, _ = S.splits(a_codes, b_codes, tile, True)
    keep_a = {INTERSECTION: (True, False), UNION: (True, True), DIFFERENCE: (False, True), SYMMETRIC_DIFFERENCE: (False, True)}[op]   # (matched, unmatched)
    keep_b = {INTERSECTION: (False, False), UNION: (False, True), DIFFERENCE: (False, False), SYMMETRIC_DIFFERENCE: (False, True)}[op]
    codes, origin = [], []
    for i in range(len(sa) - 1):
        a0, a1, b0, b1 = sa[i], sa[i + 1], sb[i], sb[i + 1]
        A = _Window(a_codes, a0, a1, [a0 - 1])
        B = _Window(b_codes, b0, b1, [b0 - 1, b1])
        ka, kb = a_codes[a0:a1], b_codes[b0:b1]
        ranked = []
        for e in range(a1 - a0):
            x = A[a0 + e]
            head = not (A.exists(a0 + e - 1) and A[a0 + e - 1] == x)
            below = int((kb < x).sum())
            matched = B.exists(b0 + below) and B[b0 + below] == x
            if head and keep_a[0 if matched else 1]:
                ranked.append((e + below, x, a0 + e))
        for j in range(b1 - b0):
            x = B[b0 + j]
            head = not (B.exists(b0 + j - 1) and B[b0 + j - 1] == x)
            not_above = int((ka <= x).sum())
            matched = A.exists(a0 + not_above - 1) and A[a0 + not_above - 1] == x
            if head and keep_b[0 if matched else 1]:
                ranked.append((j + not_above, x, n + b0 + j))
        ranked.sort()
        assert len({r for r, _, _ in ranked}) == len(ranked), "two kept elements with one rank"
        codes += [x for _, x, _ in ranked]
        origin += [s for _, _, s in ranked]
    return np.array(codes, a_codes.dtype), np.array(origin, np.uint64)


# ---- the clamped model: inputs in ANY order (the pieces: search_expect)

KEEP_MASK = {INTERSECTION: 1, UNION: 7, DIFFERENCE: 2, SYMMETRIC_DIFFERENCE: 6}    # set_keep_mask: matched A, unmatched A, unmatched B


class ClampedTile:
    """set_tile: the extent and the halo of tile i (A, B: Checked arrays)"""

    def __init__(self, i, A, B, splits, tile, stats=None):
        n, m = len(A), len(B)
        x = S.Extent(i, n, m, splits, tile, stats)
        self.a0, self.b0, self.na, self.nb = x.a0, x.b0, x.na, x.nb
        self.has_a_before = self.a0 > 0 and self.a0 <= n
        self.has_b_before = self.b0 > 0 and self.b0 <= m
        self.has_b_behind = self.b0 + self.nb < m
        self.a_before = A[self.a0 - 1] if self.has_a_before else 0
        self.b_before = B[self.b0 - 1] if self.has_b_before else 0
        self.b_behind = B[self.b0 + self.nb] if self.has_b_behind else 0


def decide(codes, self0, count, other0, length, has_before, before, has_edge, edge, keep_matched, keep_unmatched, bside, store):
    """set_decide: the number of kept elements; store(e, x, base, keep) for every element"""
    kept = [0]

    def f(e, x, base):
        prev = codes[self0 + (e - 1 if e else 0)]
        head = prev != x if e else not (has_before and before == x)
        in_tile = base > 0 if bside else base < length
        y = codes[other0 + (base - 1 if bside else base) if in_tile else 0]
        matched = y == x if in_tile else (has_edge and edge == x)
        keep = head and (keep_matched if matched else keep_unmatched)
        kept[0] += 1 if keep else 0
        store(e, x, base, keep)
    S.merge_for_counts(codes, self0, count, other0, length, bside, f)
    return kept[0]


def decide_a(codes, t, keep_matched, keep_unmatched, store):
    """set_decide_a"""
    return decide(codes, 0, t.na, t.na, t.nb, t.has_a_before, t.a_before, t.has_b_behind, t.b_behind, keep_matched, keep_unmatched, False, store)


def decide_tile(codes, t, keep, outk, src):
    """set_decide_tile (outk is None: the count kernel's, which writes nothing)"""
    last = t.na + t.nb - 1
    self0 = [0]

    def store(e, x, base, kept):
        if outk is not None:
            r = e + base if e + base < last else last
            src[r] = self0[0] + e if kept else S.NONE16
            if kept:
                outk[r] = x
    kept = decide_a(codes, t, keep & 1 != 0, keep & 2 != 0, store)
    self0[0] = t.na
    kept += decide(codes, t.na, t.nb, 0, t.na, t.has_b_before, t.b_before, t.has_a_before, t.a_before, False, keep & 4 != 0, True, store)
    return kept


def count_clamped(A, B, splits, tile, keep):
    """set_count_kernel for every tile: the tile counts (no race, no junk: every cell that is read was staged)"""
    n, m = len(A), len(B)
    tile_counts = []
    for i in range(len(splits) - 1):
        t = ClampedTile(i, A, B, splits, tile)
        if t.na + t.nb == 0:
            tile_counts.append(0)
            continue
        codes = S.Lds(tile, None, False, "codes")
        S.stage(A, t.a0, t.na, codes, 0)
        S.stage(B, t.b0, t.nb, codes, t.na)
        codes.barrier()
        tile_counts.append(decide_tile(codes, t, keep, None, None))
        assert codes.junk_reads == 0 and tile_counts[-1] <= t.na + t.nb
    return tile_counts


def tiles_clamped(a_codes, b_codes, tile, op, cap=None, junk=S.NONE16, first=False, stats=None, counted=None):
    """The clamped model of msd_set_sorted (the split, set_count_kernel, the scan, set_write_kernel with keys and origin) for
    inputs in ANY order.  ``cap`` None: no cap.  ``junk``, ``first``: see merge_expect.tiles_clamped.  ``counted``: the
    ``tile_counts`` an earlier run on these inputs returned (they depend on nothing else).  Returns
    ``(Clamped(count, out, origin), junk_reads, collisions)``: count is what *d_num_out receives, out holds codes."""
    a_codes, b_codes = np.asarray(a_codes), np.asarray(b_codes)
    n, m = len(a_codes), len(b_codes)
    A, B = S.Checked(a_codes, "a"), S.Checked(b_codes, "b")
    sa, _ = S.split_points(A.x, B.x, tile, True)
    splits = S.Checked(sa, "splits")
    keep = KEEP_MASK[op]
    tile_counts = count_clamped(A, B, splits, tile, keep) if counted is None else counted
    count = sum(tile_counts)
    windows = S.out_windows(tile_counts, count, count if cap is None else cap)
    out, origin = S.Stores("d_out"), S.Stores("d_out_origin")
    junk_reads = collisions = 0
    for i, (base, lim) in enumerate(windows):
        if base >= lim:
            continue
        t = ClampedTile(i, A, B, splits, tile, stats)
        ranks = t.na + t.nb
        if ranks == 0:
            continue
        cnt = min(lim - base, ranks)
        last = ranks - 1
        j = last if junk == "last" else junk
        codes, outk, src = S.Lds(tile, j, first, "codes"), S.Lds(tile, j, first, "outk"), S.Lds(tile, j, first, "src")
        S.stage(A, t.a0, t.na, codes, 0)
        S.stage(B, t.b0, t.nb, codes, t.na)
        codes.barrier()
        decide_tile(codes, t, keep, outk, src)
        collisions += src.collisions
        if stats is not None:
            stats.hit("collision", src.collisions)
        for lds in (codes, outk, src):
            lds.barrier()

        def place(r, to, e):
            codes[to] = outk[r]
            src[to] = e
        marks = S.ballot_compact(src, ranks, cnt, tile, place)
        if stats is not None and min(marks, cnt) < cnt:
            stats.hit("unplaced")                                       # positions nothing was compacted to are stored
        codes.barrier()
        src.barrier()
        for p in range(cnt):
            assert base + p < lim
            out[base + p] = codes[p]
            e = src[p] if src[p] < last else last
            from_a = e < t.na
            at = t.a0 + e if from_a else t.b0 + (e - t.na)
            assert at < (n if from_a else m)
            origin[base + p] = at if from_a else n + at
        junk_reads += codes.junk_reads + outk.junk_reads + src.junk_reads
    return S.Clamped(count=count, tile_counts=tile_counts, out=out, origin=origin), junk_reads, collisions


def decide_np(codes, self0, count, other0, length, has_before, before, has_edge, edge, keep_matched, keep_unmatched, bside):
    """decide, vectorised over the `count` elements: ``(keep, base)``"""
    if count == 0:
        return np.zeros(0, bool), np.zeros(0, np.int64)
    e = np.arange(count)
    x = codes[self0 + e]
    base = S.lds_count_np(codes, other0, length, x, bside)
    prev = codes[self0 + np.maximum(e - 1, 0)]
    head = np.where(e > 0, prev != x, not (has_before and before == x[0]))
    in_tile = base > 0 if bside else base < length
    y = codes[np.where(in_tile, other0 + (base - 1 if bside else base), 0)]
    matched = np.where(in_tile, y == x, bool(has_edge) & (x == edge))
    return head & np.where(matched, keep_matched, keep_unmatched), base


def count_np(a_codes, b_codes, tile, op):
    """count_clamped, vectorised, at any tile: what *d_num_out (INTERSECTION: *d_num_groups) receives for inputs in any order"""
    A, B = np.asarray(a_codes), np.asarray(b_codes)          # (the index checks are count_clamped's)
    a_codes, b_codes = A, B
    sa, _ = S.split_points(A, B, tile, True)
    splits = S.Checked(sa, "splits")
    keep, tile_counts = KEEP_MASK[op], []
    for i in range(len(sa) - 1):
        t = ClampedTile(i, A, B, splits, tile)
        kept = 0
        if t.na + t.nb:
            codes = S.stage_np(a_codes, b_codes, t)
            kept += int(decide_np(codes, 0, t.na, t.na, t.nb, t.has_a_before, t.a_before, t.has_b_behind, t.b_behind, keep & 1 != 0, keep & 2 != 0, False)[0].sum())
            kept += int(decide_np(codes, t.na, t.nb, 0, t.na, t.has_b_before, t.b_before, t.has_a_before, t.a_before, False, keep & 4 != 0, True)[0].sum())
        tile_counts.append(kept)
    return tile_counts

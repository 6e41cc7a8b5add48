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

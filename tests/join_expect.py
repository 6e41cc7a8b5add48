"""What msd_join_groups and msd_join_pairs have to produce (a helper module like set_expect.py, not a test).

The expectation is defined HERE, with numpy: both inputs are unsigned views of their bit patterns plus a key type
(``sort_rows_expect``'s U32 .. F64) and become order-preserving unsigned codes with ``sort_rows_expect.np_encode``.
``np.unique(return_index=True, return_counts=True)`` of each side gives its distinct values with the first index and the
length of every run, ``np.intersect1d`` the values both sides hold.  Equality is equality of codes, that is of bits: for
floats -0.0 and +0.0 differ and NaNs with equal bits are one value.

:func:`pairs` gives the index pairs of a range of ranks without building the whole product; :func:`tiles` is a numpy model
of the write kernel (csrc/msd_join.hpp): per tile of the merge path the groups whose A head lies in the tile, from the tile
and a halo of four elements, with at most one search behind the tile per side.

Plain module, no fixture: ``import join_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

import search_expect as S
import sort_rows_expect as E

KEY_TYPES = S.KEY_TYPES


def groups(a_bits, b_bits, key_type):
    """``(keys, a_first, a_count, b_first, b_count)``: per value that both sides hold, ascending by code, its bit pattern
    and (uint64) the first index and the run length in A and in B"""
    a_bits, b_bits = np.asarray(a_bits), np.asarray(b_bits)
    ca, cb = E.np_encode(a_bits, key_type), E.np_encode(b_bits, key_type)
    for name, c in (("A", ca), ("B", cb)):
        assert (c[1:] >= c[:-1]).all(), "%s is not ascending in the order of its type" % name
    va, fa, na = np.unique(ca, return_index=True, return_counts=True)
    vb, fb, nb = np.unique(cb, return_index=True, return_counts=True)
    _, ia, ib = np.intersect1d(va, vb, assume_unique=True, return_indices=True)
    u = lambda x: x.astype(np.uint64)
    return a_bits[fa[ia]], u(fa[ia]), u(na[ia]), u(fb[ib]), u(nb[ib])


def total(g):
    """the number of pairs of the groups (a Python int: it may exceed 64 bits nowhere, n and m being below 2^32)"""
    return int(sum(int(p) * int(q) for p, q in zip(g[2].tolist(), g[4].tolist())))


def pairs(g, lo, hi):
    """``(ia, ib)`` (uint64) of the pairs with ranks [lo, min(hi, total)): the groups in order, within a group of p x q
    pairs rank t is (a_first + t // q, b_first + t % q)"""
    _, a_first, a_count, b_first, b_count = g
    ends = np.cumsum(a_count * b_count, dtype=np.uint64)
    tot = int(ends[-1]) if ends.size else 0
    r = np.arange(lo, max(lo, min(hi, tot)), dtype=np.uint64)
    at = np.searchsorted(ends, r, side="right")                     # the group of rank r: the first whose end lies beyond r
    t = r - (ends[at] - (a_count * b_count)[at])
    return a_first[at] + t // b_count[at], b_first[at] + t % b_count[at]


class _Window:
    """one side of a tile: reads are allowed inside [lo, hi) and at the halo indices; a search behind the tile is counted"""

    def __init__(self, x, lo, hi, halo):
        self.x, self.lo, self.hi, self.halo, self.searches = x, lo, hi, set(halo), 0

    def exists(self, i):
        return 0 <= i < len(self.x)

    def __getitem__(self, i):
        assert self.lo <= i < self.hi or i in self.halo, "index %d is neither in the tile [%d, %d) nor in its halo %s" % (i, self.lo, self.hi, sorted(self.halo))
        assert self.exists(i)
        return self.x[i]

    def upper_behind(self, v):
        """the end of the run of v that leaves the tile: the one global search"""
        self.searches += 1
        return self.hi + int(np.searchsorted(self.x[self.hi:], v, side="right"))


def tiles(a_codes, b_codes, tile):
    """The model: ``(codes, a_first, a_count, b_first, b_count)`` as the kernels compute them.  The splits are those of the
    merge (B after every A that is not larger).  In tile i, with a[a0, a1) and b[b0, b1) and the halo a[a0 - 1], a[a1],
    b[b0 - 1], b[b1]: an A element is kept iff its predecessor in A differs and b[b0 + lb] equals it, lb = |{b in tile : b <
    a}|.  Its runs end at a0 + |{a in tile : a <= v}| and b0 + |{b in tile : b <= v}| where those lie inside the tile;
    otherwise at the tile's end, unless the halo element behind the tile equals v: then one search behind the tile finds the
    end.  Asserts that every index read lies in the tile or the halo and that a tile searches at most once per side."""
    a_codes, b_codes = np.asarray(a_codes), np.asarray(b_codes)
    sa, sb, _ = S.splits(a_codes, b_codes, tile, True)
    out = [[], [], [], [], []]
    for i in range(len(sa) - 1):
        a0, a1, b0, b1 = sa[i], sa[i + 1], sb[i], sb[i + 1]
        A = _Window(a_codes, a0, a1, [a0 - 1, a1])
        B = _Window(b_codes, b0, b1, [b0 - 1, b1])
        ka, kb = a_codes[a0:a1], b_codes[b0:b1]
        for e in range(a1 - a0):
            v = A[a0 + e]
            head = not (A.exists(a0 + e - 1) and A[a0 + e - 1] == v)
            lb = int((kb < v).sum())
            if not (head and B.exists(b0 + lb) and B[b0 + lb] == v):
                continue
            ua, ub = int((ka <= v).sum()), int((kb <= v).sum())
            a_end, b_end = a0 + ua, b0 + ub
            if ua == a1 - a0 and A.exists(a1) and A[a1] == v:
                a_end = A.upper_behind(v)
            if ub == b1 - b0 and B.exists(b1) and B[b1] == v:
                b_end = B.upper_behind(v)
            for col, x in zip(out, (v, a0 + e, a_end - (a0 + e), b0 + lb, b_end - (b0 + lb))):
                col.append(x)
        assert A.searches <= 1 and B.searches <= 1, "tile %d searches behind itself %d and %d times" % (i, A.searches, B.searches)
    return (np.array(out[0], a_codes.dtype),) + tuple(np.array(c, np.uint64) for c in out[1:])

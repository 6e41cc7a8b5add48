"""What msd_merge_sorted has to produce (a helper module like search_expect.py, not a test).

The expectation is defined HERE, with numpy: both inputs are unsigned views of their bit patterns plus a key type
(``sort_rows_expect``'s U32 .. F64); the concatenation ``[A; B]`` becomes order-preserving unsigned codes with
``sort_rows_expect.np_encode``, and ``np.argsort(kind="stable")`` of the codes is the origin: the merged keys are the
concatenation's bit patterns in that order.  Stable means: among equal codes A before B, and within a side in input order.
For floats the order is IEEE-754 totalOrder on the bits, NOT numpy's or torch's float order.

:func:`tiles` is a numpy model of the two kernels (csrc/msd_merge2.hpp): the cut of the merged sequence into tiles along the
merge path -- ``search_expect.splits(..., right=True)`` is the split model -- and per tile the rank of every element.

Plain module, no fixture: ``import merge_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

import search_expect as S
import sort_rows_expect as E

KEY_TYPES = S.KEY_TYPES


def expected(a_bits, b_bits, key_type):
    """``(merged_bits, origin)``: the n + m bit patterns in the stable order of their codes, and per position the index
    (uint64) in the concatenation [A; B] of the element that lands there"""
    a_bits, b_bits = np.asarray(a_bits), np.asarray(b_bits)
    for name, x in (("A", a_bits), ("B", b_bits)):
        c = E.np_encode(x, key_type)
        assert (c[1:] >= c[:-1]).all(), "%s is not ascending in the order of its type" % name
    cat = np.concatenate([a_bits, b_bits])
    origin = np.argsort(E.np_encode(cat, key_type), kind="stable")
    return cat[origin], origin.astype(np.uint64)


def tiles(a_codes, b_codes, tile):
    """The model: ``(merged_codes, origin)`` as the two kernels compute them.  The splits are those of the search's merge
    path under the RIGHT rule (B after every A that is not larger); in tile i local A element e goes to
    e + |{b in tile : b < a_e}| and local B element j to j + |{a in tile : a <= b_j}|, and position p of the tile's slice
    takes the element ranked there.  Asserts that every position is written exactly once."""
    a_codes, b_codes = np.asarray(a_codes), np.asarray(b_codes)
    n, m = len(a_codes), len(b_codes)
    sa, sb, _ = S.splits(a_codes, b_codes, tile, True)
    merged = np.zeros(n + m, a_codes.dtype)
    origin = np.full(n + m, -1, np.int64)
    for i in range(len(sa) - 1):
        d0 = min(i * tile, n + m)
        ka, kb = a_codes[sa[i]:sa[i + 1]], b_codes[sb[i]:sb[i + 1]]
        assert len(ka) + len(kb) == min((i + 1) * tile, n + m) - d0
        ranked = [(e + int((kb < x).sum()), x, sa[i] + e) for e, x in enumerate(ka)]
        ranked += [(j + int((ka <= x).sum()), x, n + sb[i] + j) for j, x in enumerate(kb)]
        for r, x, src in ranked:
            assert 0 <= r < len(ka) + len(kb), "a rank outside the tile"
            assert origin[d0 + r] == -1, "a position written twice"
            merged[d0 + r], origin[d0 + r] = x, src
    assert (origin >= 0).all(), "a position no tile wrote"
    return merged, origin.astype(np.uint64)

"""What msd_search_sorted has to produce (a helper module like reduce_expect.py, not a test).

The expectation is defined HERE, with numpy: keys and needles are unsigned views of their bit patterns plus a key type
(``sort_rows_expect``'s U32 .. F64); both become order-preserving unsigned codes with ``sort_rows_expect.np_encode``, and
``np.searchsorted`` on the codes gives, per needle, the number of keys whose code is ``<`` (left) or ``<=`` (right) the
needle's.  For floats that is IEEE-754 totalOrder on the bits, NOT numpy's or torch's float order.

:func:`splits` is a numpy model of the merge path's decomposition (csrc/msd_search.hpp): the cut of the merged sequence of
keys and needles into tiles, and per tile the search of its needles in its keys.

Plain module, no fixture: ``import search_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

import sort_rows_expect as E

LEFT, RIGHT = 0, 1
KEY_TYPES = [E.U32, E.I32, E.F32, E.U64, E.I64, E.F64]


def expected(sorted_bits, needle_bits, key_type, right):
    """uint64 array, one per needle: the number of keys (unsigned bit patterns of ``key_type``, ascending by code) whose
    code is < (``right``: <=) the needle's code"""
    keys = E.np_encode(sorted_bits, key_type)
    assert (keys[1:] >= keys[:-1]).all(), "the keys are not ascending in the order of their type"
    return np.searchsorted(keys, E.np_encode(needle_bits, key_type), side="right" if right else "left").astype(np.uint64)


def sort_by_code(bits, key_type):
    """the bit patterns in the order of their type"""
    return E.np_decode(np.sort(E.np_encode(bits, key_type)), key_type)


def _precedes(x, k, right):
    """does a needle with code x go before a key with code k in the merged sequence?  Left: before every key that is not
    smaller.  Right: after every key that is not larger."""
    return x < k if right else x <= k


def splits(a_codes, b_codes, tile, right):
    """The model: keys ``a_codes`` and needles ``b_codes`` (both ascending codes) merged into one sequence and cut every
    ``tile`` elements.  Returns ``(a, b, result)``: per diagonal i = 0 .. ceil((n + m) / tile) the keys a[i] and the needles
    b[i] among the first min(i * tile, n + m) elements (found by the binary search of the split kernel), and per needle
    a[i] + the number of the tile's keys that count for it (the tile kernel), -1 where no tile wrote."""
    n, m = len(a_codes), len(b_codes)
    tiles = -(-(n + m) // tile)
    a, b = [], []
    for i in range(tiles + 1):
        d = min(i * tile, n + m)
        lo, hi = max(0, d - n), min(d, m)
        while lo < hi:
            mid = (lo + hi) // 2
            assert 0 <= mid < m and 0 <= d - mid - 1 < n
            if _precedes(b_codes[mid], a_codes[d - mid - 1], right):
                lo = mid + 1
            else:
                hi = mid
        a.append(d - lo)
        b.append(lo)
    result = np.full(m, -1, np.int64)
    for i in range(tiles):
        ka, kb = a_codes[a[i]:a[i + 1]], b_codes[b[i]:b[i + 1]]
        for j, x in enumerate(kb):
            assert result[b[i] + j] == -1, "a needle written twice"
            result[b[i] + j] = a[i] + int(((ka <= x) if right else (ka < x)).sum())
    return a, b, result

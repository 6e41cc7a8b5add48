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


def split_points(a_codes, b_codes, tile, right):
    """The split kernel, line for line: ``(a, b)``, per diagonal i = 0 .. ceil((n + m) / tile) the keys a[i] and the needles
    b[i] = d_i - a[i] among the first d_i = min(i * tile, n + m) elements of the merged sequence, by the binary search of
    search_split_kernel.  Nothing here needs ascending inputs: every probe is asserted to lie inside its array, and every
    result inside [d_i - min(d_i, m), min(d_i, n)]."""
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
        assert d - min(d, m) <= d - lo <= min(d, n)
        a.append(d - lo)
        b.append(lo)
    return a, b


def splits(a_codes, b_codes, tile, right):
    """The model: keys ``a_codes`` and needles ``b_codes`` (both ascending codes) merged into one sequence and cut every
    ``tile`` elements.  Returns ``(a, b, result)``: per diagonal i = 0 .. ceil((n + m) / tile) the keys a[i] and the needles
    b[i] among the first min(i * tile, n + m) elements (found by the binary search of the split kernel), and per needle
    a[i] + the number of the tile's keys that count for it (the tile kernel), -1 where no tile wrote."""
    m = len(b_codes)
    a, b = split_points(a_codes, b_codes, tile, right)
    tiles = len(a) - 1
    result = np.full(m, -1, np.int64)
    for i in range(tiles):
        ka, kb = a_codes[a[i]:a[i + 1]], b_codes[b[i]:b[i + 1]]
        for j, x in enumerate(kb):
            assert result[b[i] + j] == -1, "a needle written twice"
            result[b[i] + j] = a[i] + int(((ka <= x) if right else (ka < x)).sum())
    return a, b, result


# ---- the CLAMPED models: what the tile kernels do when the inputs are NOT ascending
#
# The pieces below follow the kernels' text statement by statement (csrc/msd_search.hpp, msd_merge2.hpp): they compute what
# the kernels compute, clamps included, with every read of an input, a split, a position or an LDS cell index-checked and
# every store recorded.  merge_expect.tiles_clamped, set_expect.tiles_clamped, join_expect.tiles_clamped and
# join_expect.expand_clamped are built from them.

MASK64 = (1 << 64) - 1
NONE16 = 0xFFFF                              # kSetNone
JUNKS = (0, "last", 0xFFFE, NONE16)          # what an LDS cell nothing wrote in this launch may hold ("last": the tile's last rank)


class Checked:
    """an array in global memory: every read is index-checked"""

    def __init__(self, x, name):
        self.x, self.name = x.tolist() if hasattr(x, "tolist") else list(x), name

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        assert 0 <= i < len(self.x), "%s[%d] is read: outside [0, %d)" % (self.name, i, len(self.x))
        return self.x[i]


class Stores:
    """an output array: every store is recorded, ``at[index]`` = the values stored there, in order"""

    def __init__(self, name):
        self.name, self.at = name, {}

    def __setitem__(self, i, v):
        assert i >= 0, "%s[%d] is stored" % (self.name, i)
        self.at.setdefault(i, []).append(v)

    def indices(self):
        return set(self.at)


class Lds:
    """An LDS array of ``size`` cells.  A cell nothing wrote in this launch reads as ``junk`` (and ``junk_reads`` counts
    it).  Two stores to one cell between two barriers are a race on the GPU: ``first`` says which one stays -- for every cell of
    the array alike -- and ``collisions`` counts them."""

    def __init__(self, size, junk, first, name):
        self.size, self.junk, self.first, self.name = size, junk, first, name
        self.cells, self.phase, self.collisions, self.junk_reads = {}, set(), 0, 0

    def barrier(self):
        self.phase = set()

    def __getitem__(self, i):
        assert 0 <= i < self.size, "%s[%d] is read: outside [0, %d)" % (self.name, i, self.size)
        if i in self.cells:
            return self.cells[i]
        self.junk_reads += 1
        return self.junk

    def __setitem__(self, i, v):
        assert 0 <= i < self.size, "%s[%d] is stored: outside [0, %d)" % (self.name, i, self.size)
        if i in self.phase:
            self.collisions += 1
            if self.first:
                return
        self.phase.add(i)
        self.cells[i] = v


class Clamped:
    """what a clamped model returns: the Stores of every output, and whatever the call counts"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Stats(dict):
    """counters of the clamps that were hit"""

    def hit(self, what, by=1):
        if by:
            self[what] = self.get(what, 0) + by


def variants(run):
    """``run(junk, first)`` for the junk values and the race orders that can differ: every junk in JUNKS only if a junk cell
    was read, both orders only if two stores met in one cell (``run`` returns ``(result, junk_reads, collisions)``).
    The two orders are GLOBAL -- every cell of every LDS array keeps its first store, or every cell its last -- not one choice
    per colliding cell: on the GPU src and outk of one place may have different winners.  No index depends on that: whichever
    wins is a key or a local index inside the tile.  Yields ``(junk, first, result)``."""
    r, junk_reads, collisions = run(JUNKS[0], False)
    yield JUNKS[0], False, r
    for first in ((False, True) if collisions else (False,)):
        for junk in (JUNKS if junk_reads else JUNKS[:1]):
            if (junk, first) != (JUNKS[0], False):
                yield junk, first, run(junk, first)[0]


class Extent:
    """merge_tile_extent: tile i as the splits (a Checked array) cut it, with the clamps"""

    def __init__(self, i, n, m, splits, tile, stats=None):
        total = n + m
        self.d0, self.d1 = min(i * tile, total), min((i + 1) * tile, total)
        a1 = splits[i + 1]
        b1 = self.d1 - a1
        self.a0 = splits[i]
        self.b0 = self.d0 - self.a0
        assert 0 <= a1 <= n and 0 <= b1 <= m and 0 <= self.a0 <= n and 0 <= self.b0 <= m     # (what the split kernel guarantees)
        self.na = min(a1 - self.a0, tile) if a1 > self.a0 else 0
        self.nb = min(b1 - self.b0, tile - self.na) if b1 > self.b0 else 0
        if stats is not None:
            if a1 < self.a0:
                stats.hit("a_descends")
            if b1 < self.b0:
                stats.hit("b_descends")
            if a1 - self.a0 > tile:
                stats.hit("na_over_tile")
            if b1 - self.b0 > tile - self.na:
                stats.hit("nb_clipped")
        assert self.a0 + self.na <= n and self.b0 + self.nb <= m and self.na + self.nb <= tile


def stage(src, first, count, lds, dst):
    """search_stage: ``count`` elements of the Checked array ``src`` from ``first`` to the LDS at ``dst``"""
    for e in range(count):
        lds[dst + e] = src[first + e]


def counts(k, x, right):
    """search_counts"""
    return k < x or (right and k == x)


def lds_count(lds, at, length, x, right):
    """lds_count: the branch-free search over lds[at, at + length)"""
    base = 0
    if length:
        l = length
        while l > 1:
            half = l >> 1
            base += half if counts(lds[at + base + half - 1], x, right) else 0
            l -= half
        base += 1 if counts(lds[at + base], x, right) else 0
    return base


def merge_for_counts(codes, self0, count, other0, length, right, f):
    """merge_for_counts: f(e, x, base) for every element e < count"""
    for e in range(count):
        x = codes[self0 + e]
        f(e, x, lds_count(codes, other0, length, x, right))


def ballot_compact(mark, count, cnt, size, place):
    """ballot_compact: place(r, to, mark[r]) for every r < count whose mark is not kSetNone and whose rank `to` among those
    is below cnt.  All of mark is read before place is called (INPLACE: behind the barrier)."""
    assert count <= size
    s = [mark[r] for r in range(count)]
    mark.barrier()
    to = 0
    for r in range(count):
        if s[r] != NONE16:
            if to < cnt:
                place(r, to, s[r])
            to += 1
    return to


def out_windows(tile_counts, total, cap):
    """tile_out_window for every tile: [base, lim) from the scanned counts"""
    bases = [0]
    for c in tile_counts:
        bases.append(bases[-1] + c)
    assert bases[-1] == total
    return [(bases[i], min(bases[i + 1], cap)) for i in range(len(tile_counts))]


def tiles_clamped(a_codes, b_codes, tile, right, positions=None, stats=None):
    """The clamped model of the merge path of the search (search_split_kernel, search_tile_kernel) for keys and needles in
    ANY order: returns the Stores of d_out -- per index the values some tile stores there.  Every LDS cell that is read was
    staged (asserted): the result depends on no junk and on no race."""
    n, m = len(a_codes), len(b_codes)
    A, B = Checked(a_codes, "keys"), Checked(b_codes, "needles")
    P = None if positions is None else Checked(positions, "positions")
    sa, _ = split_points(a_codes.tolist() if hasattr(a_codes, "tolist") else a_codes, B.x, tile, right)
    splits = Checked(sa, "splits")
    out = Stores("d_out")
    for i in range(len(sa) - 1):
        t = Extent(i, n, m, splits, tile, stats)
        if t.nb == 0:
            continue
        lds = Lds(tile, None, False, "lds")
        stage(A, t.a0, t.na, lds, 0)
        stage(B, t.b0, t.nb, lds, t.na)
        lds.barrier()
        for j in range(t.nb):
            x = lds[t.na + j]
            base = lds_count(lds, 0, t.na, x, right)
            at = t.b0 + j
            to = P[at] if P is not None else at
            if stats is not None and to in out.at:
                stats.hit("covered_twice")
            out[to] = t.a0 + base
        assert lds.junk_reads == 0
    return out


# ---- the same at the kernels' real tile, vectorised: what the GPU tests of unsorted inputs compare with (the CPU tests
# compare these with the statement-by-statement models above on small tiles)

def lds_count_np(codes, at, length, x, right):
    """lds_count for every code of the vector x at once over codes[at, at + length): the same probes in the same order"""
    base = np.zeros(x.size, np.int64)
    if length:
        l = length
        while l > 1:
            half = l >> 1
            k = codes[at + base + half - 1]
            base += np.where((k < x) | (right & (k == x)), half, 0)
            l -= half
        k = codes[at + base]
        base += (k < x) | (right & (k == x))
    return base


def extents(a_codes, b_codes, tile, right, stats=None):
    """the Extent of every tile of the merge path over inputs in any order"""
    n, m = len(a_codes), len(b_codes)
    sa, _ = split_points(a_codes, b_codes, tile, right)
    splits = Checked(sa, "splits")
    return [Extent(i, n, m, splits, tile, stats) for i in range(len(sa) - 1)]


def stage_np(a_codes, b_codes, t):
    """the staged tile: a[a0, a0 + na) with b[b0, b0 + nb) behind it"""
    return np.concatenate([a_codes[t.a0:t.a0 + t.na], b_codes[t.b0:t.b0 + t.nb]])


def stored_clamped(a_codes, b_codes, tile, right, positions=None):
    """tiles_clamped, vectorised: ``(index, value)``, two int64 arrays with one entry per store to d_out, in the tiles' order"""
    a_codes, b_codes = np.asarray(a_codes), np.asarray(b_codes)
    index, value = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for t in extents(a_codes, b_codes, tile, right):
        if t.nb == 0:
            continue
        lds = stage_np(a_codes, b_codes, t)
        at = t.b0 + np.arange(t.nb)
        index.append(at if positions is None else np.asarray(positions, np.int64)[at])
        value.append(t.a0 + lds_count_np(lds, 0, t.na, lds[t.na:], right))
    return np.concatenate(index), np.concatenate(value)

"""What msd_compact has to produce, and the masks and keys its tests feed it (a helper module like runs_expect.py, not a test).

The expectation is defined HERE, with numpy on unsigned views of the bit patterns: ``keep`` is (mask byte != 0) AND
(lo code <= code <= hi code) with the codes of ``sort_rows_expect.np_encode``, XOR invert; the expected keys, values and
indices are boolean indexing with it, and with ``rest`` the kept elements followed by the rejected ones.  Floats are
therefore compared in IEEE-754 totalOrder on their bits.

Plain module, no fixture: ``import compact_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

import sort_rows_expect as E

RANGE, INVERT, REST = 1, 2, 4          # MSD_COMPACT_* of include/msd_compact_hip.h
UT = {4: np.uint32, 8: np.uint64}
MASK_BYTES = np.array([1, 2, 0x80, 0xFF], np.uint8)   # what a non-zero mask byte is drawn from


def keep(n, keys=None, kt=0, mask=None, lo=None, hi=None, invert=False):
    """the boolean keep vector of n elements: ``keys`` are bit patterns (unsigned) of key type ``kt``, ``lo`` / ``hi`` bit
    patterns too (both given, or neither: no range test)"""
    k = np.ones(n, bool)
    if mask is not None:
        k &= np.asarray(mask).view(np.uint8) != 0
    if lo is not None:
        ut = keys.dtype.type
        codes = E.np_encode(keys, kt)
        lc, hc = E.np_encode(np.array([lo, hi], dtype=ut), kt)
        k &= (codes >= lc) & (codes <= hc)
    return ~k if invert else k


def expected(k, keys=None, vals=None, rest=False, cap=None):
    """``(m, keys, values, indices)`` as the call stores them for the keep vector ``k``: min(m, cap) elements each, or all n
    with ``rest``; an input that is not given gives ``None``"""
    idx = np.flatnonzero(k).astype(np.int64)
    m = idx.size
    if rest:
        idx = np.r_[idx, np.flatnonzero(~k).astype(np.int64)]
    elif cap is not None:
        idx = idx[:cap]
    return m, (keys[idx] if keys is not None else None), (vals[idx] if vals is not None else None), idx


def naive(n, keys=None, kt=0, mask=None, lo=None, hi=None, invert=False, vals=None, rest=False, cap=None):
    """the same, one element at a time in plain Python"""
    def code(b, W):
        top = 1 << (W - 1)
        if kt % 3 == 0:
            return b
        if kt % 3 == 1:
            return (b + top) % (1 << W)
        return (~b) % (1 << W) if b & top else b | top
    kept, rejected = [], []
    for i in range(n):
        p = True
        if mask is not None:
            p = int(mask[i]) != 0
        if lo is not None:
            W = 8 * keys.itemsize
            p = p and code(int(lo), W) <= code(int(keys[i]), W) <= code(int(hi), W)
        (kept if p != invert else rejected).append(i)
    m = len(kept)
    idx = kept + rejected if rest else kept[:len(kept) if cap is None else cap]
    idx = np.array(idx, np.int64)
    return m, (keys[idx] if keys is not None else None), (vals[idx] if vals is not None else None), idx


# ---- keep patterns

PATTERNS = ["all", "none", "alternating", "every64", "every65", "first", "last", "tile_last", "tile_first", "block", "rand1", "rand50", "rand99"]
BIG_PATTERNS = ["all", "none", "rand50", "rand1"]


def pattern(name, n, tile, seed=1):
    """the named keep vector of n elements for a tile of ``tile`` elements (the array taken as 16-byte aligned: tile t is
    elements [t * tile, (t + 1) * tile))"""
    k = np.zeros(n, bool)
    i = np.arange(n)
    if name == "all":
        k[:] = True
    elif name == "none":
        pass
    elif name == "alternating":
        k[::2] = True
    elif name == "every64":
        k[::64] = True
    elif name == "every65":
        k[::65] = True
    elif name == "first":
        k[:1] = True
    elif name == "last":
        k[n - 1:] = True
    elif name == "tile_last":          # exactly the last element of each tile
        k[i % tile == tile - 1] = True
    elif name == "tile_first":         # exactly the first element of each tile
        k[i % tile == 0] = True
    elif name == "block":              # one kept block of exactly one tile that starts in the middle of a tile
        k[tile // 2 + 3:tile // 2 + 3 + tile] = True
    elif name.startswith("rand"):
        k = np.random.default_rng(seed).random(n) < int(name[4:]) / 100.0
    else:
        raise ValueError(name)
    return k


def mask_of(k, seed=2):
    """mask bytes that keep exactly ``k``: the non-zero ones drawn from MASK_BYTES"""
    rng = np.random.default_rng(seed)
    return np.where(k, MASK_BYTES[rng.integers(0, len(MASK_BYTES), k.size)], 0).astype(np.uint8)


def keys_for_range(k, es, seed=3):
    """``(keys, lo, hi)``: unsigned keys (key type U32 / U64) of which exactly those of ``k`` lie in [lo, hi]; the others lie on
    both sides of the range, the bounds themselves occur"""
    ut = UT[es]
    rng = np.random.default_rng(seed)
    lo, hi = 1000, 1000 + (1 << (8 * es - 2))
    inside = rng.integers(lo, hi + 1, k.size, dtype=np.uint64)
    inside[rng.random(k.size) < 0.05] = lo
    inside[rng.random(k.size) < 0.05] = hi
    below = rng.integers(0, lo, k.size, dtype=np.uint64)
    above = rng.integers(hi + 1, (1 << (8 * es)) - 1, k.size, dtype=np.uint64, endpoint=True)
    outside = np.where(rng.random(k.size) < 0.5, below, above)
    outside[rng.random(k.size) < 0.05] = lo - 1
    outside[rng.random(k.size) < 0.05] = hi + 1
    return np.where(k, inside, outside).astype(ut), lo, hi


def values_for(n, vb, seed=4):
    """a value column of vb-byte elements: a function of the index that differs between neighbours"""
    with np.errstate(over="ignore"):
        return ((np.arange(n, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(64 - 8 * vb)).astype(UT[vb])


def float_specials(ft):
    """name -> bit pattern: the planted float keys"""
    ut = np.uint32 if ft == np.float32 else np.uint64
    W = 8 * np.dtype(ut).itemsize
    sign = 1 << (W - 1)
    qnan = 0x7FC00000 if W == 32 else 0x7FF8 << 48
    inf = 0x7F800000 if W == 32 else 0x7FF << 52
    return {"-nan": qnan | sign | 5, "-inf": inf | sign, "-den": sign | 1, "-0": sign, "+0": 0, "+den": 1, "+inf": inf, "+nan": qnan | 5,
            "+nanmax": sign - 1, "-nanmax": (1 << W) - 1}

"""What msd_run_encode has to produce, and the arrays its tests feed it (a helper module like sort_rows_expect.py, not a test).

The expectation is defined HERE, with numpy on unsigned views of the bit patterns: ``heads = r_[True, a[1:] != a[:-1]]``,
``starts = flatnonzero(heads)``, ``values = a[starts]``, ``inverse = cumsum(heads) - 1``, the inverse applied through the
positions where they are given.  Equality is therefore bitwise: -0.0 and +0.0 differ, NaNs with equal bits are one value.

Plain module, no fixture: ``import runs_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

UT = {4: np.uint32, 8: np.uint64}
IT = {4: np.int32, 8: np.int64}


def expected(a, positions=None):
    """``(m, values, starts, inverse)`` of the unsigned array ``a``: ``starts`` has m + 1 entries, the last one ``a.size``
    (for an empty array: the single entry 0); ``inverse[positions[i]]`` = the run of element i where positions are given."""
    n = a.size
    if n == 0:
        return 0, a[:0].copy(), np.zeros(1, np.int64), np.zeros(0, np.int64)
    heads = np.r_[True, a[1:] != a[:-1]]
    starts = np.flatnonzero(heads).astype(np.int64)
    values = a[starts]
    inverse = np.cumsum(heads, dtype=np.int64) - 1
    if positions is not None:
        through = np.empty(n, np.int64)
        through[positions] = inverse
        inverse = through
    return int(starts.size), values, np.r_[starts, np.int64(n)], inverse


def expected_capped(a, cap, positions=None):
    """what a call with capacity ``cap`` stores: ``(m, values[:k], starts[:k + 1], inverse)`` with k = min(m, cap); the
    last stored start is the array's length if m <= cap, else the start of run ``cap``"""
    m, values, starts, inverse = expected(a, positions)
    k = min(m, cap)
    return m, values[:k], starts[:k + 1], inverse


# ---- inputs

def _odd(es):
    return UT[es](0x9E3779B1) if es == 4 else UT[es](0x9E3779B97F4A7C15)


def distinct(n, es, seed=0):
    """n different values, neighbours far apart: an odd multiple of the index (a bijection of the unsigned type)"""
    with np.errstate(over="ignore"):
        return (np.arange(n, dtype=UT[es]) + UT[es](seed + 1)) * _odd(es)


def from_runs(lengths, es, seed=0, values=None):
    """runs of the given lengths; run j holds ``values[j % len(values)]`` if values are given (neighbours must differ),
    else the j-th of :func:`distinct`"""
    lengths = np.asarray(lengths, dtype=np.int64)
    per_run = distinct(lengths.size, es, seed) if values is None else np.asarray(values, dtype=UT[es])[np.arange(lengths.size) % len(values)]
    return np.repeat(per_run, lengths)


def geometric(n, es, mean, seed):
    """n elements in runs of geometric length with the given mean (the last run cut to fit)"""
    if n == 0:
        return np.zeros(0, UT[es])
    rng = np.random.default_rng(seed)
    lengths = rng.geometric(1.0 / mean, size=int(n / mean * 1.5) + 16)
    while lengths.sum() < n:
        lengths = np.r_[lengths, rng.geometric(1.0 / mean, size=lengths.size)]
    return from_runs(lengths, es, seed)[:n]


def two_values(n, es, a, b, seed):
    """runs of geometric length (mean 3) that alternate between the bit patterns a and b"""
    if n == 0:
        return np.zeros(0, UT[es])
    rng = np.random.default_rng(seed)
    lengths = rng.geometric(1.0 / 3.0, size=n)
    return from_runs(lengths, es, values=[a, b])[:n]


PATTERNS = ["distinct", "equal", "starts_at_tile", "ends_at_tile", "three_tiles", "alternating", "geo1.5", "geo40", "geo5000"]


def make(pattern, n, es, tile, seed=1):
    """the named run pattern at n elements of es bytes, for a tile of `tile` elements (the array is taken as 16-byte aligned:
    tile t is elements [t * tile, (t + 1) * tile)); patterns that need more elements than n are cut to n"""
    ut = UT[es]
    c = ut(0x00C0FFEE)
    if pattern == "distinct":
        return distinct(n, es, seed)
    if pattern == "equal":
        return np.full(n, c, ut)
    if pattern == "alternating":
        a = np.full(n, c, ut)
        a[1::2] = ut(0x0BADF00D)
        return a
    if pattern.startswith("geo"):
        return geometric(n, es, float(pattern[3:]), seed)
    a = distinct(n, es, seed)
    a[a == c] = c + ut(1)                       # (the planted run's value occurs nowhere else)
    if pattern == "starts_at_tile":             # a run whose first element is a tile's first element
        a[tile:tile + 17] = c
    elif pattern == "ends_at_tile":             # a run whose last element is a tile's last element
        a[max(tile - 9, 0):tile] = c
    elif pattern == "three_tiles":              # a run that is exactly tiles 1, 2 and 3, other values around it
        a[tile:4 * tile] = c
    else:
        raise ValueError(pattern)
    return a


def sizes(tile, scan_tile):
    """name -> n: the sizes the issue lists, T = tile"""
    T = tile
    return {"0": 0, "1": 1, "2": 2, "3": 3, "63": 63, "64": 64, "65": 65, "T-1": T - 1, "T": T, "T+1": T + 1, "2T+1": 2 * T + 1,
            "3T-1": 3 * T - 1, "big": (scan_tile + 1) * T + 5}


SIZE_NAMES = list(sizes(0, 0))

"""What msd_scan_runs has to produce (a helper module like reduce_expect.py, not a test).

The expectation is defined HERE, with numpy: the runs and their starts are those of ``runs_expect.expected`` on the unsigned
view of the keys; the values are unsigned views of their bit patterns plus a value type (``sort_rows_expect``'s U32 .. F64),
taken through the positions where they are given; then per element i of a run that starts at s

* ``"sum"`` of integers: a global wrapping cumsum on uint64 (U32, U64) or int64 (I32, I64) minus its value in front of s;
* ``"sum"`` of floats: the SEQUENTIAL float64 cumsum of the run -- not the library's order: equal only where every partial
  sum is exact, otherwise a reference for a rounding bound;
* ``"min"`` / ``"max"``: the running minimum / maximum of the order-preserving codes, decoded back;
* ``"count"``: i - s + 1 as uint64, whatever the values are;

exclusive: the inclusive result of element i - 1, and :func:`identity` at the first element of a run; with ``scatter`` the
result of element i is stored at ``positions[i]``.  (msd_scan_runs does not offer positions yet; the GPU tests use them to
gather a value column on the host.)

Sequential per run, vectorised: a run of at least ``LONG`` elements takes one ``ufunc.accumulate``, the shorter ones advance
together, one element per step (tests/test_scan_abi.py checks both against a plain loop).

Plain module, no fixture: ``import scan_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

import reduce_expect as X
import runs_expect as R
import sort_rows_expect as E

OPS = {"sum": 0, "min": 1, "max": 2, "count": 3}
EXCLUSIVE, SCATTER = 1, 2
LONG = 48


def out_dtype(vt, op):
    """the numpy dtype that carries d_out: sums and counts are 8 bytes, min and max the unsigned view of the value"""
    return np.uint64 if op == "count" else X.out_dtype(vt, op)


def identity(vt, op):
    """what an exclusive scan stores at the first element of a run, as one element of :func:`out_dtype`"""
    if op in ("sum", "count"):
        return out_dtype(vt, op)(0)
    ut = E.UT[vt]
    code = np.array([np.iinfo(ut).max if op == "min" else 0], ut)
    return E.np_decode(code, vt)[0]


def seg_accumulate(ufunc, w, starts, long=LONG):
    """``ufunc`` accumulated from the left inside every run [starts[j], starts[j + 1]), in the order of a plain loop"""
    out = w.copy()
    first, lens = starts[:-1], np.diff(starts)
    big = lens >= long
    for a, b in zip(first[big].tolist(), (first[big] + lens[big]).tolist()):
        out[a:b] = ufunc.accumulate(w[a:b])
    first, lens = first[~big], lens[~big]
    for j in range(1, long):
        at = first[lens > j] + j
        if at.size == 0:
            break
        out[at] = ufunc(out[at - 1], w[at])
    return out


def inclusive(starts, vbits, vt, op):
    """the inclusive scan of the n values (already in the order of the elements) as an array of :func:`out_dtype`"""
    n = int(starts[-1])
    first, lens = starts[:-1], np.diff(starts)
    if op == "count":
        return (np.arange(n, dtype=np.int64) - np.repeat(first, lens) + 1).astype(np.uint64)
    if op == "sum":
        w = X.widen(vbits, vt)
        with np.errstate(over="ignore", invalid="ignore"):
            if vt in X.FLOAT:
                return seg_accumulate(np.add, w, starts)
            c = np.cumsum(w, dtype=w.dtype)
            return c - np.repeat(c[first] - w[first], lens)
    codes = E.np_encode(vbits, vt)
    return E.np_decode(seg_accumulate(np.minimum if op == "min" else np.maximum, codes, starts), vt)


def expected(keys, vbits, vt, op, exclusive=False, positions=None, scatter=False):
    """the n results of the unsigned array ``keys`` and the values ``vbits`` (unsigned bit patterns of value type ``vt``;
    ignored, and may be None, for ``"count"``), as an array of :func:`out_dtype`"""
    if scatter and positions is None:
        raise ValueError("scatter needs positions")
    m, _, starts, _ = R.expected(keys)
    n = keys.size
    if n == 0:
        return np.zeros(0, out_dtype(vt, op))
    if op != "count" and positions is not None:
        vbits = vbits[positions]
    out = inclusive(starts, vbits, vt, op)
    if exclusive:
        shifted = np.empty_like(out)
        shifted[1:] = out[:-1]
        shifted[starts[:-1]] = identity(vt, op)
        out = shifted
    if scatter:
        through = np.empty_like(out)
        through[positions] = out
        out = through
    return out


def naive(keys, vbits, vt, op, exclusive=False, positions=None, scatter=False):
    """the same by a plain loop over the elements (small arrays only): the definition, read off the header"""
    n = keys.size
    out = np.zeros(n, out_dtype(vt, op))
    ident = identity(vt, op)
    codes = None
    if op == "count":
        w = np.ones(n, np.uint64)
    else:
        g = vbits[positions] if positions is not None else vbits
        w = X.widen(g, vt) if op == "sum" else E.np_encode(g, vt)
    acc = None
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            head = i == 0 or keys[i] != keys[i - 1]
            before = None if head else acc
            if head:
                acc = w[i]
            elif op in ("sum", "count"):
                acc = acc + w[i]
            else:
                acc = min(acc, w[i]) if op == "min" else max(acc, w[i])
            s = before if exclusive else acc
            if s is None:
                r = ident
            elif op in ("min", "max"):
                r = E.np_decode(np.array([s], E.UT[vt]), vt)[0]
            else:
                r = s
            out[positions[i] if scatter else i] = r
    return out

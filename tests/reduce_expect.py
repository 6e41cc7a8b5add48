"""What msd_reduce_runs has to produce (a helper module like runs_expect.py, not a test).

The expectation is defined HERE, with numpy: the runs and their starts are those of ``runs_expect.expected`` on the unsigned
view of the keys; the values are unsigned views of their bit patterns plus a value type (``sort_rows_expect``'s U32 .. F64),
taken through the positions where they are given; then

* ``"sum"`` of integers: ``np.add.reduceat`` on uint64 (U32, U64: zero-extended) or int64 (I32, I64: sign-extended), wrapping
  modulo 2^64;
* ``"sum"`` of floats: ``np.add.reduceat`` on float64 -- numpy's order, NOT the library's: equal only where every partial
  sum is exact, otherwise a reference for a rounding bound;
* ``"min"`` / ``"max"``: ``np.minimum.reduceat`` / ``np.maximum.reduceat`` on the order-preserving codes, decoded back: the
  bit patterns of the extreme element in totalOrder.

Plain module, no fixture: ``import reduce_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

import runs_expect as R
import sort_rows_expect as E

OPS = {"sum": 0, "min": 1, "max": 2}
VAL_TYPES = [E.U32, E.I32, E.F32, E.U64, E.I64, E.F64]
SIGNED = {E.I32: np.int32, E.I64: np.int64}
FLOAT = {E.F32: np.float32, E.F64: np.float64}


def out_dtype(vt, op):
    """the numpy dtype that carries d_out: sums are 8 bytes (uint64 / int64 / float64), min and max the unsigned view of the value"""
    if op != "sum":
        return E.UT[vt]
    return np.float64 if vt in FLOAT else np.int64 if vt in SIGNED else np.uint64


def widen(vbits, vt):
    """the values as the accumulator of a sum sees them: uint64, int64 or float64"""
    if vt in FLOAT:
        return vbits.view(FLOAT[vt]).astype(np.float64)
    if vt in SIGNED:
        return vbits.view(SIGNED[vt]).astype(np.int64)
    return vbits.astype(np.uint64)


def expected(keys, vbits, vt, op, positions=None):
    """``(m, starts, out)``: the number of runs of the unsigned array ``keys``, the m + 1 starts, and per run the reduction
    ``op`` of the values ``vbits`` (unsigned bit patterns of value type ``vt``), as an array of :func:`out_dtype`"""
    m, _, starts, _ = R.expected(keys)
    if positions is not None:
        vbits = vbits[positions]
    at = starts[:-1]
    if m == 0:
        return 0, starts, np.zeros(0, out_dtype(vt, op))
    if op == "sum":
        with np.errstate(over="ignore", invalid="ignore"):
            return m, starts, np.add.reduceat(widen(vbits, vt), at)
    codes = E.np_encode(vbits, vt)
    red = np.minimum.reduceat(codes, at) if op == "min" else np.maximum.reduceat(codes, at)
    return m, starts, E.np_decode(red, vt)

"""The argument rules of the Python wrapper, stated once: the counterpart of csrc/msd_args.hpp for api.py.

Every function here is a pure check on tensors and numbers (torch only describes them and, in :func:`output` and
:func:`count_cell`, supplies memory the caller asks for): it raises :class:`MsdError` or returns what the caller goes on
with, and touches neither the library nor the device.  A method of ``MsdContext`` calls the rules that apply to it, top to
bottom, in the order in which they refuse.  tests/test_api_refusals.py records the outcome of every rule through every
method that uses it.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional


class MsdError(RuntimeError):
    pass


def _torch():
    import torch
    return torch


KEY_U32, KEY_I32, KEY_F32, KEY_U64, KEY_I64, KEY_F64 = range(6)   # MSD_KEY_* of include/msd_radix_hip.h


# ---- key tensors
@functools.lru_cache(maxsize=None)
def _key_types() -> dict:
    """The one table of the dtypes that have a key order."""
    torch = _torch()
    table = {torch.int32: KEY_I32, torch.float32: KEY_F32, torch.int64: KEY_I64, torch.float64: KEY_F64}
    for name, kt in (("uint32", KEY_U32), ("uint64", KEY_U64)):   # (not in every torch)
        if hasattr(torch, name):
            table[getattr(torch, name)] = kt
    return table


def key_type(keys) -> int:
    """The ``MSD_KEY_*`` of a tensor's dtype."""
    kt = _key_types().get(keys.dtype)
    if kt is None:
        raise MsdError(f"no key order for dtype {keys.dtype}: float32, int32, float64, int64, uint32 or uint64")
    return kt


def one_dim(name: str, *tensors, what: str = "tensors") -> None:
    """``name`` takes 1-D ``what`` (``None``: an absent tensor, here and below)."""
    for t in tensors:
        if t is not None and t.dim() != 1:
            raise MsdError(f"{name} takes 1-D {what}")


def contiguous(name: str, *tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_contiguous():
            raise MsdError(f"{name} takes contiguous tensors")


def flat(name: str, *tensors, what: str = "1-D contiguous tensors") -> None:
    """Both at once, where one message names both."""
    for t in tensors:
        if t is not None and (t.dim() != 1 or not t.is_contiguous()):
            raise MsdError(f"{name} takes {what}")


def elem_4_or_8(name: str, t, what: str = "4- or 8-byte elements") -> int:
    """The element size of ``t``, which is 4 or 8."""
    if t.element_size() not in (4, 8):
        raise MsdError(f"{name} takes {what}, not {t.dtype}")
    return t.element_size()


def same_length(what: str, *tensors) -> None:
    """``what`` names the tensors: "keys and vals"."""
    if len({t.numel() for t in tensors if t is not None}) > 1:
        raise MsdError(f"{what} differ in length")


def same_dtype(a, b, names: str = "a and b") -> None:
    if b.dtype != a.dtype:
        raise MsdError(f"{names} differ in dtype: {a.dtype} and {b.dtype}")


def sorted_pair(name: str, a, b, contiguous_too: bool = True) -> int:
    """The rules of two sorted inputs, in their order: a dtype with a key order, the same for both, 1-D and (where the
    method does not look at further tensors first) contiguous.  Returns the key type."""
    kt = key_type(a)
    same_dtype(a, b)
    one_dim(name, a, b)
    if contiguous_too:
        contiguous(name, a, b)
    return kt


def positions(t, n: int, what: str = "elements", name: Optional[str] = None) -> None:
    """Refuses positions (``None``: absent) that are not ``n`` contiguous int64 in one dimension.  The message counts them
    against the ``what`` they index, or -- with ``name``, the argument's -- says how many there must be."""
    if t is not None and (t.dtype != _torch().int64 or t.dim() != 1 or t.numel() != n or not t.is_contiguous()):
        raise MsdError(f"{name} must be a contiguous 1-D int64 tensor of {n} elements" if name else
                       f"positions must be a contiguous 1-D int64 tensor, as many as the {what}")


# ---- numbers
def non_negative(what: str, *numbers) -> None:
    """``what`` names the numbers: "n, m and cap"."""
    if min(numbers) < 0:
        raise MsdError(f"{what} must not be negative")


def cap_or(cap, default: int) -> int:
    """``cap`` as an int; ``None`` is the caller's default.  The one place that says "cap must not be negative"."""
    cap = default if cap is None else int(cap)
    non_negative("cap", cap)
    return cap


def op_code(table: dict, op) -> int:
    """The number of ``op`` in ``REDUCE_OPS``, ``SCAN_OPS`` or ``SET_OPS``."""
    if op not in table:
        raise MsdError(f"op must be one of {sorted(table)}, not {op!r}")
    return table[op]


def result_dtype(op: str, vals, vt: int):
    """What a reduction or a scan gives: int64 for a count, the values' dtype for min and max; a sum is float64 for floats,
    uint64 for unsigned values where torch has it, else int64."""
    torch = _torch()
    if op == "count":
        return torch.int64
    if op != "sum":
        return vals.dtype
    if vt in (KEY_F32, KEY_F64):
        return torch.float64
    if vt in (KEY_U32, KEY_U64) and hasattr(torch, "uint64"):
        return torch.uint64
    return torch.int64


# ---- outputs
def output(t, dtype, shape: tuple, message: Optional[str], device=None, at_least: bool = False):
    """An optional output.  A given tensor is checked where there is a ``message`` to refuse it with (``{dtype}`` and
    ``{shape}`` in it stand for those two): ``dtype``, contiguous, and exactly ``shape`` -- or, ``at_least``, one dimension
    of no fewer than ``shape[0]`` elements -- and comes back as it is.  A missing one is allocated with ``shape`` where a ``device`` is given (the caller has looked at where its tensors
    live by then) and stays ``None`` otherwise -- and where ``dtype`` is ``None``: the call does not produce this output."""
    if t is None:
        return _torch().empty(shape, dtype=dtype, device=device) if device is not None and dtype is not None else None
    fits = (t.dim() == 1 and t.numel() >= shape[0]) if at_least else tuple(t.shape) == tuple(shape)
    if message is not None and not (t.dtype == dtype and fits and t.is_contiguous()):
        raise MsdError(message.format(dtype=dtype, shape=tuple(shape)))
    return t


def count_cell(device):
    """The one-element int64 tensor on the device that a call writes its true count to."""
    torch = _torch()
    return torch.empty(1, dtype=torch.int64, device=device)


# ---- pointers
def ptr(t) -> C.c_void_p:
    """The address of a tensor's first element, null for ``None``.  (``MsdContext._ptr`` also checks where the tensor lives
    and how wide its elements are; this is for tensors that a rule above has looked at, or that the wrapper allocated.)"""
    return C.c_void_p(t.data_ptr() if t is not None else 0)

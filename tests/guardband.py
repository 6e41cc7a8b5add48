"""Guard bands around the buffers a test hands to the library: did a kernel write where it must not?

An :class:`Arena` is ONE tensor ``[front guard | lead | payload | back guard]``.  The payload is what the call under test
gets; everything around it is known memory, filled with a pseudo-random function of the element's index (a constant
could not show a shifted copy of itself, and a constant key input could equal it).  ``check()`` regenerates that pattern
and compares.  The front guard ends on a 4 KiB boundary, so ``lead_bytes`` (a multiple of 16: the library refuses
buffers that are not aligned to 16 bytes) says exactly where the payload starts relative to the 256-byte block grid and
the page grid.  A :class:`Buf` is a window into an Arena's payload that knows what the payload was filled with: the
buffers of the tests that call the C ABI.

Plain module, no fixture: ``import guardband`` (tests/ is on sys.path under pytest's default import mode).  It works on
``device="cpu"`` too, which is how tests/test_guardband.py tests it without a GPU.
"""
import numpy as np
import torch

PAGE = 4096
MIN_GUARD_BYTES = 64 << 10

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NP_INT = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
_NP_UINT = {1: np.uint8, 4: np.uint32, 8: np.uint64}
BUF_PATTERN_FIRST = 12345                         # where a Buf's fill starts in the pattern; the value means nothing


def guard_elems(elem_bytes, *unit_elems):
    """Guard width per side in elements: twice the largest unit (in elements) a workgroup of the path under test handles
    at once, never less than 64 KiB, rounded up to whole pages."""
    b = max([MIN_GUARD_BYTES] + [2 * int(u) * elem_bytes for u in unit_elems])
    return (b + PAGE - 1) // PAGE * PAGE // elem_bytes


def _c(v):
    return v - (1 << 64) if v >= 1 << 63 else v   # a 64-bit constant as torch's int64 takes it


def pattern(first, count, elem_bytes, device="cpu"):
    """Cells first .. first + count - 1 of the guard pattern: a multiply-xorshift of the index (wrapping int64
    arithmetic), cut to the element size.  Neighbouring cells differ, and so do cells any fixed distance apart."""
    x = torch.arange(first, first + count, dtype=torch.int64, device=device) + 1
    x = x * _c(0x9E3779B97F4A7C15)
    x = x ^ ((x >> 29) & 0x7FFFFFFFF)
    x = x * _c(0xBF58476D1CE4E5B9)
    x = x ^ ((x >> 32) & 0xFFFFFFFF)
    if elem_bytes == 8:
        return x
    bits = 8 * elem_bytes
    x = x & ((1 << bits) - 1)
    if elem_bytes > 1:                            # the signed value with these bits: the cast below is then exact
        x = (x ^ (1 << (bits - 1))) - (1 << (bits - 1))
    return x.to(_INT[elem_bytes])


class Arena:
    """``Arena(dtype, n, lead_bytes=0, guard=None, neighbours="random", device="cuda")``

    ``payload``: view of n elements of ``dtype`` whose address is (a 4 KiB boundary) + ``lead_bytes``.
    ``guard``: elements per side (default: :func:`guard_elems` of nothing, 64 KiB); rounded up to whole pages.
    ``neighbours``: "low" / "high" force the one element directly in front of and directly behind the payload to all
    zeros / all ones.  A kernel that wrongly takes n + 1 elements as its input and sorts the extra one back into its own
    place leaves a neighbour that is larger than every key intact; with "low" behind an ascending sort it cannot.
    """

    def __init__(self, dtype, n, lead_bytes=0, guard=None, neighbours="random", device="cuda"):
        es = torch.empty(0, dtype=dtype).element_size()
        if lead_bytes % 16 or lead_bytes < 0:
            raise ValueError("lead_bytes must be a non-negative multiple of 16")
        if neighbours not in ("random", "low", "high"):
            raise ValueError(neighbours)
        g = guard_elems(es) if guard is None else guard_elems(es, (int(guard) + 1) // 2)
        self.dtype, self.es, self.n, self.guard, self.neighbours, self.device = dtype, es, int(n), g, neighbours, device
        self.front = g + lead_bytes // es         # cells in front of the payload: the guard and the lead
        self.back = g
        total = (self.front + self.n + self.back) * es
        self._raw = torch.empty(total + PAGE, dtype=torch.uint8, device=device)
        pad = (-self._raw.data_ptr()) % PAGE
        self._cells = self._raw[pad:pad + total].view(_INT[es])
        self._cells[:self.front] = self._expected("front")
        self._cells[self.front + self.n:] = self._expected("back")
        self.payload = self._cells[self.front:self.front + self.n].view(dtype)
        self.ptr = self._cells.data_ptr() + self.front * es   # (an empty view has no address of its own)
        assert self.ptr % PAGE == lead_bytes % PAGE and self.ptr % 16 == 0 and (not self.n or self.payload.data_ptr() == self.ptr)

    def _expected(self, side):
        if side == "front":
            e = pattern(0, self.front, self.es, self.device)
            at = self.front - 1
        else:
            e = pattern(self.front + self.n, self.back, self.es, self.device)
            at = 0
        if self.neighbours != "random":
            e[at] = 0 if self.neighbours == "low" else (255 if self.es == 1 else -1)
        return e

    def fill(self, a):
        """Copies the numpy array ``a`` (n elements of the payload's element size; any dtype of that size) into the payload."""
        a = np.ascontiguousarray(a)
        if a.size != self.n or a.itemsize != self.es:
            raise ValueError(f"fill: {a.size} x {a.itemsize} bytes into a payload of {self.n} x {self.es}")
        if self.n:
            self._cells[self.front:self.front + self.n] = torch.from_numpy(a.view(_NP_INT[self.es])).to(self.device)
        return self

    def host(self, np_dtype):
        """The payload's bits as a numpy array of ``np_dtype`` (same element size)."""
        return self._cells[self.front:self.front + self.n].cpu().numpy().view(np_dtype)

    def check(self, what=""):
        """Synchronises, then asserts that both guards are bit-identical to what they were filled with.  The message
        names the side, the first and last changed cell relative to the payload's boundary (front: -1 is the cell
        directly in front of the payload; back: +0 is the cell directly behind it) and how many cells changed."""
        if str(self.device).startswith("cuda"):
            torch.cuda.synchronize()
        for side in ("front", "back"):
            got = self._cells[:self.front] if side == "front" else self._cells[self.front + self.n:]
            exp = self._expected(side)
            bad = torch.nonzero(got != exp).flatten()
            if bad.numel() == 0:
                continue
            first, last = int(bad[0]), int(bad[-1])
            rel = (lambda i: i - self.front) if side == "front" else (lambda i: i)
            where = "payload start" if side == "front" else "payload end"
            raise AssertionError(
                f"{what + ': ' if what else ''}{side} guard touched: {bad.numel()} cell(s) of {self.es} bytes changed, "
                f"first at {where} {rel(first):+d}, last at {where} {rel(last):+d} "
                f"(payload of {self.n} elements at 4 KiB + {(self.front - self.guard) * self.es} bytes; "
                f"first changed cell holds {int(got[first]) & ((1 << 8 * self.es) - 1):#x}, "
                f"was {int(exp[first]) & ((1 << 8 * self.es) - 1):#x})")


class Buf:
    """``Buf(es, count, off=0, lead_bytes=0, a=None, device="cuda")``: `count` elements of es (1, 4 or 8) bytes that start
    `off` elements into the payload of an Arena whose payload starts `lead_bytes` behind a page boundary.  The whole payload
    holds a known pattern, or, behind `off`, the array `a`; ``fill`` is that content as unsigned words, ``ptr`` the address
    of element `off`."""

    def __init__(self, es, count, off=0, lead_bytes=0, a=None, device="cuda"):
        self.es, self.count, self.off = es, count, off
        self.arena = Arena(_INT[es], count + off, lead_bytes=lead_bytes, device=device)
        self.fill = pattern(BUF_PATTERN_FIRST, count + off, es).numpy().view(_NP_UINT[es]).copy()
        if a is not None:
            self.fill[off:] = a
        self.arena.fill(self.fill)
        self.ptr = self.arena.ptr + off * es

    def reset(self):
        self.arena.fill(self.fill)

    def host(self):
        """the `count` elements; what lies in front of them in the payload must be what it was"""
        h = self.arena.host(_NP_UINT[self.es])
        assert (h[:self.off] == self.fill[:self.off]).all(), "payload in front of the buffer changed"
        return h[self.off:]

    def untouched_from(self, k):
        return (self.host()[k:] == self.fill[self.off + k:]).all()

    def unchanged(self):
        return self.untouched_from(0)

    def written(self, count):
        """the first `count` elements; the rest of the buffer must be what it was"""
        h = self.host()
        assert (h[count:] == self.fill[self.off + count:]).all(), "an element beyond the first %d changed" % count
        return h[:count]

    def check(self, what):
        self.arena.check(what)

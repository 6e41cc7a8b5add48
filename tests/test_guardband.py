"""The guard-band helper (tests/guardband.py) decides whether tests/test_gpu_bounds.py can fail at all, so it is tested
here, on the CPU, with numpy stand-ins for the operation: an honest in-place sort passes, and every kind of stray write
is detected with the right side and offset in the message."""
import re

import numpy as np
import pytest
import torch

import guardband
from guardband import Arena

LEADS = [0, 16, 48, 240, 272]
DTYPES = [torch.int16, torch.int32, torch.int64, torch.uint8]
MODES = ["random", "low", "high"]
NP_U = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _cells(a):
    """numpy view of the whole arena (CPU tensors share their memory with numpy): the stand-in kernels write through it"""
    return a._cells.numpy().view(NP_U[a.es])


def _filled(dtype, n, **kw):
    a = Arena(dtype, n, device="cpu", **kw)
    rng = np.random.default_rng(n + a.es)
    a.fill(rng.integers(1, 1 << (8 * a.es - 1), n, dtype=np.uint64).astype(NP_U[a.es]))   # (never 0, never all ones)
    return a


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lead", LEADS)
def test_honest_sort_passes(lead, dtype, mode):
    n = 1000
    a = _filled(dtype, n, lead_bytes=lead, neighbours=mode)
    before = a.host(NP_U[a.es]).copy()
    c = _cells(a)
    c[a.front:a.front + n].sort()
    a.check("np.sort in place")
    assert (a.host(NP_U[a.es]) == np.sort(before)).all()
    assert a.payload.numel() == n and a.payload.dtype == dtype


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_payload_alignment(lead, dtype):
    a = Arena(dtype, 77, lead_bytes=lead, device="cpu")
    p = a.payload.data_ptr()
    assert p == a.ptr and p % 16 == 0
    assert p % 4096 == lead                           # the front guard ends on a page
    assert (p % 256 == 0) == (lead % 256 == 0)        # off the 256-byte block grid exactly where intended
    assert a.guard * a.es >= 64 << 10 and a.back == a.guard and a.front == a.guard + lead // a.es


def test_lead_must_be_a_multiple_of_16():
    with pytest.raises(ValueError):
        Arena(torch.int32, 10, lead_bytes=8, device="cpu")


def test_guard_width_rule():
    assert guardband.guard_elems(4) == (64 << 10) // 4
    assert guardband.guard_elems(4, 24576) == 2 * 24576
    assert guardband.guard_elems(8, 17408, 2048) * 8 >= 2 * 17408 * 8
    assert guardband.guard_elems(2, 100) * 2 % 4096 == 0
    a = Arena(torch.int64, 5, guard=40000, device="cpu")
    assert a.guard >= 40000 and a.guard * 8 % 4096 == 0


def test_pattern_is_no_constant_and_no_shifted_copy():
    for es in (1, 2, 4, 8):
        p = guardband.pattern(0, 1 << 16, es).numpy()
        assert (guardband.pattern(100, 50, es).numpy() == p[100:150]).all()     # a function of the index alone
        for d in (1, 2, 4, 8, 64, 1024):                                        # a copy shifted by d cells differs nearly everywhere
            assert (p[d:] == p[:-d]).mean() < (0.02 if es == 1 else 1e-3), (es, d)
        if es > 1:
            assert len(np.unique(p)) > 0.6 * len(p)


def _message(a, what="case"):
    with pytest.raises(AssertionError) as e:
        a.check(what)
    return str(e.value)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_element_behind_the_payload(dtype, mode):
    a = _filled(dtype, 333, lead_bytes=48, neighbours=mode)
    c = _cells(a)
    c[a.front + a.n] = c[a.front + a.n - 1]           # the payload's last element once more (never 0, never all ones)
    m = _message(a)
    assert m.startswith("case: back guard touched: 1 cell(s)") and "first at payload end +0, last at payload end +0" in m, m


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_element_in_front_of_the_payload(dtype, mode):
    a = _filled(dtype, 333, lead_bytes=16, neighbours=mode)
    c = _cells(a)
    c[a.front - 1] = c[a.front]
    m = _message(a)
    assert "front guard touched: 1 cell(s)" in m and "first at payload start -1, last at payload start -1" in m, m


@pytest.mark.parametrize("lead", [0, 272])
def test_far_ends_of_the_guards(lead):
    a = _filled(torch.int32, 100, lead_bytes=lead)
    _cells(a)[0] ^= 1
    m = _message(a)
    assert "front guard touched: 1 cell(s)" in m and f"first at payload start {-a.front:+d}," in m, m
    a = _filled(torch.int32, 100, lead_bytes=lead)
    _cells(a)[-1] ^= 0x80000000
    m = _message(a)
    assert "back guard touched: 1 cell(s)" in m and f"last at payload end {a.back - 1:+d} " in m, m


def test_guard_cell_overwritten_with_its_neighbour_cell():
    """What a constant sentinel could not show: a guard cell that now holds the value of the guard cell next to it."""
    a = _filled(torch.int32, 64)
    c = _cells(a)
    at = a.front + a.n + 10
    c[at] = c[at + 1]
    m = _message(a)
    assert "back guard touched: 1 cell(s)" in m and "first at payload end +10, last at payload end +10" in m, m
    a = _filled(torch.int16, 64)
    c = _cells(a)
    c[a.front - 9:a.front - 5] = c[a.front - 8:a.front - 4].copy()      # four cells shifted by one
    m = _message(a)
    assert "front guard touched: 4 cell(s)" in m and "first at payload start -9, last at payload start -6" in m, m


def test_several_cells_first_and_last_are_reported():
    a = _filled(torch.int64, 10, lead_bytes=240)
    c = _cells(a)
    c[a.front + a.n + 3] ^= 1
    c[a.front + a.n + 700] ^= 1
    c[a.front + a.n + 5000] ^= 1
    m = _message(a, what="")
    assert m.startswith("back guard touched: 3 cell(s) of 8 bytes changed, first at payload end +3, last at payload end +5000"), m
    assert re.search(r"4 KiB \+ 240 bytes", m), m


def _sort_one_more(a):
    """A wrong kernel: takes n + 1 elements as its input and sorts them in place."""
    c = _cells(a)
    c[a.front:a.front + a.n + 1].sort()


def _sort_one_before(a):
    c = _cells(a)
    c[a.front - 1:a.front + a.n].sort()


def test_sorting_one_element_too_many_needs_both_neighbour_modes():
    """The stand-in that sorts n + 1 elements is caught behind the payload under "low" (the 0 moves to the front, a key
    takes its cell).  Under "high" it is NOT: all ones is the largest key and is sorted back into its own cell -- which
    is why tests/test_gpu_bounds.py runs both modes.  In front of the payload it is the other way round."""
    a = _filled(torch.int32, 500, neighbours="low")
    _sort_one_more(a)
    m = _message(a)
    assert "back guard touched: 1 cell(s)" in m and "first at payload end +0" in m, m
    a = _filled(torch.int32, 500, neighbours="high")
    _sort_one_more(a)
    a.check("documented blind spot of 'high' behind an ascending sort")
    a = _filled(torch.int32, 500, neighbours="high")
    _sort_one_before(a)
    m = _message(a)
    assert "front guard touched: 1 cell(s)" in m and "first at payload start -1" in m, m
    a = _filled(torch.int32, 500, neighbours="low")
    _sort_one_before(a)
    a.check("documented blind spot of 'low' in front of an ascending sort")


def test_neighbour_cells_hold_what_the_mode_says():
    for dtype in DTYPES:
        for mode, want in (("low", 0), ("high", -1)):
            a = Arena(dtype, 9, lead_bytes=16, neighbours=mode, device="cpu")
            c = _cells(a)
            ones = (1 << (8 * a.es)) - 1
            assert int(c[a.front - 1]) == (want & ones) and int(c[a.front + a.n]) == (want & ones)
            a.check()


def test_fill_checks_size_and_host_returns_the_bits():
    a = Arena(torch.float32, 4, device="cpu")
    with pytest.raises(ValueError):
        a.fill(np.zeros(5, np.float32))
    with pytest.raises(ValueError):
        a.fill(np.zeros(4, np.float64))
    x = np.array([1.5, -0.0, np.nan, np.inf], np.float32)
    a.fill(x)
    assert (a.host(np.uint32) == x.view(np.uint32)).all() and a.payload.dtype == torch.float32
    a.check()
    e = Arena(torch.int32, 0, lead_bytes=16, device="cpu")       # an empty payload: the guards touch
    e.fill(np.zeros(0, np.uint32))
    e.check()


# ---- Buf: a window into an Arena that knows what it was filled with

BUF_CASES = [(1, 0, 0), (4, 3, 48), (8, 1, 272)]      # (element bytes, off, lead_bytes)


def _buf(es, off, lead, count=7, given=True):
    a = np.arange(101, 101 + count).astype(NP_U[es]) if given else None
    return guardband.Buf(es, count, off, lead, a, device="cpu"), a


@pytest.mark.parametrize("es,off,lead", BUF_CASES)
def test_buf_address_and_contents(es, off, lead):
    b, a = _buf(es, off, lead)
    assert b.ptr % 4096 == lead + off * es and b.ptr == b.arena.ptr + off * es and b.arena.n == 7 + off
    assert (b.host() == a).all() and b.host().dtype == NP_U[es] and (b.written(7) == a).all()
    assert (b.fill[off:] == a).all() and (b.fill[:off] == guardband.pattern(guardband.BUF_PATTERN_FIRST, off, es).numpy().view(NP_U[es])).all()
    assert b.unchanged() and b.untouched_from(0) and b.untouched_from(7)
    b.check("untouched")
    p, _ = _buf(es, off, lead, given=False)               # without an array the pattern goes on behind `off`
    assert (p.host() == guardband.pattern(guardband.BUF_PATTERN_FIRST + off, 7, es).numpy().view(NP_U[es])).all() and p.unchanged()


@pytest.mark.parametrize("es,off,lead", BUF_CASES[1:])
def test_buf_catches_a_changed_cell_in_front_of_off(es, off, lead):
    b, _ = _buf(es, off, lead)
    _cells(b.arena)[b.arena.front + off - 1] ^= 1
    for call in (b.host, b.unchanged, lambda: b.untouched_from(7), lambda: b.written(7)):
        with pytest.raises(AssertionError, match="in front of the buffer"):
            call()
    b.check("the guards are what they were")
    b.reset()
    assert b.unchanged()


@pytest.mark.parametrize("es,off,lead", BUF_CASES)
def test_buf_catches_a_changed_cell_at_or_beyond_count(es, off, lead):
    for at in (3, 6):
        b, a = _buf(es, off, lead)
        _cells(b.arena)[b.arena.front + off + at] ^= 1
        with pytest.raises(AssertionError, match="beyond the first 3 changed"):
            b.written(3)
        assert not b.untouched_from(3) and not b.untouched_from(at) and b.untouched_from(at + 1) and not b.unchanged()
        assert (b.written(at + 1)[:at] == a[:at]).all() and b.written(at + 1)[at] == a[at] ^ 1
        b.check("the guards are what they were")
        b.reset()
        assert b.unchanged() and (b.written(3) == a[:3]).all()


@pytest.mark.parametrize("es,off,lead", BUF_CASES)
def test_buf_catches_a_changed_cell_below_count(es, off, lead):
    b, a = _buf(es, off, lead)
    _cells(b.arena)[b.arena.front + off] ^= 1
    assert not b.unchanged() and b.untouched_from(1) and b.host()[0] == a[0] ^ 1 and (b.written(1) == a[:1] ^ 1).all()
    b.reset()
    assert b.unchanged() and (b.host() == a).all()


@pytest.mark.parametrize("es,off,lead", BUF_CASES)
def test_buf_check_catches_a_changed_guard_cell_on_either_side(es, off, lead):
    for at, side in ((-1, "front"), (7 + off, "back")):
        b, _ = _buf(es, off, lead)
        _cells(b.arena)[b.arena.front + at] ^= 1
        with pytest.raises(AssertionError, match="case: %s guard touched: 1 cell" % side):
            b.check("case")
        assert b.unchanged()                              # (the payload is what it was: only check() looks at the guards)

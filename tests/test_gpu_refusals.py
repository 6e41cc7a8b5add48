"""A refused call touches nothing: the argument checks of the entry points around the fine-grained exchange
(msd_hist2_pack_*, msd_order_low16_counts/scatter_u32, msd_pack_low16_u32) and of the small services (msd_histogram_*,
msd_bucket_bounds_*, msd_gather_runs_*, msd_sample_*, msd_splitters_*), through the C ABI.

Every device buffer is a guardband.Arena with the default 64 KiB guards.  A refusal is checked for its return code
(MSD_EINVAL), for a message in msd_last_error that names the rule that refused it (so the ORDER of the checks is pinned
too), and for payloads and guards that are bit for bit what they were.

Overlap cases.  Source and destination lie in ONE arena, 16-byte aligned as the library demands.  Two aligned buffers can
overlap by exactly one element only where a buffer's length is one element more than a multiple of 16 bytes, so these
cases use 65 elements; where no length gives that (a histogram record is a multiple of 16 bytes long) they overlap by 16
bytes, the least the alignment rule lets exist.  The same layout with 64 elements makes the buffers exactly adjacent, in
front of and behind the source: that is accepted and the result is checked.

An EMPTY source placed inside the destination -- what the library answers today, pinned here:
  * msd_hist2_pack_u32 / _low16 (n = 0, d_keys inside the record buffer): refused, "source and destination overlap"
    (the kernel takes its extents from d_bounds, not from n);
  * msd_pack_low16_u32 (n = 0): MSD_OK before any pointer is looked at, nothing is written;
  * msd_order_low16_scatter_u32: its destination is n * 2 bytes, empty whenever its source is -- there is no such case.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MSD_OK, MSD_EINVAL = 0, -1
_NP = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _arena(a):
    """An Arena holding the numpy array ``a``."""
    import torch
    import guardband
    a = np.ascontiguousarray(a)
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.itemsize]
    return guardband.Arena(dt, a.size).fill(a)


def _bits(arena):
    return arena.host(_NP[arena.es]).copy()


def _refused(ctx, name, args, arenas, word):
    """``name(ctx, *args)`` answers MSD_EINVAL with a message containing ``word`` and leaves every arena as it was."""
    before = [_bits(a) for a in arenas]
    rc = getattr(ctx._L, name)(ctx._h, *args)
    msg = ctx._L.msd_last_error(ctx._h).decode()
    assert rc == MSD_EINVAL, (name, word, rc, msg)
    assert msg and word in msg, (name, word, msg)
    for a, b in zip(arenas, before):
        a.check(f"{name} ({word})")
        assert (_bits(a) == b).all(), (name, word, "payload changed")


def _accepted(ctx, name, args, arenas):
    rc = getattr(ctx._L, name)(ctx._h, *args)
    assert rc == MSD_OK, (name, rc, ctx._L.msd_last_error(ctx._h).decode())
    for a in arenas:
        a.check(name)


def _keys(n, seed):
    """n u32 keys ordered by their upper halves, which are 0 (the first 30) and 1"""
    rng = np.random.default_rng(seed)
    return ((np.arange(n, dtype=np.uint32) >= 30).astype(np.uint32) << np.uint32(16)) | rng.integers(0, 1 << 16, n, dtype=np.uint32)


class _Joint:
    """Source and destination in one arena of bytes: ``at(off)`` = the address ``off`` bytes into the payload."""

    def __init__(self, nbytes, seed):
        self.fill = np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)
        self.arena = _arena(self.fill)

    def at(self, off):
        assert 0 <= off <= self.arena.n
        return self.arena.ptr + off

    def put(self, off, a):
        a = np.ascontiguousarray(a).view(np.uint8)
        self.fill[off:off + a.size] = a
        self.arena.fill(self.fill)

    def view(self, off, nbytes):
        return self.arena.payload[off:off + nbytes]

    def unchanged_except(self, off, nbytes):
        got = _bits(self.arena)
        assert (got[:off] == self.fill[:off]).all() and (got[off + nbytes:] == self.fill[off + nbytes:]).all(), "bytes outside the destination changed"
        return got[off:off + nbytes]


# ------------------------------------------------------------------ msd_pack_low16_u32

def test_pack_low16_refusals(ctx):
    J = _Joint(4096, 1)
    A = 1024                                                          # the source's offset
    k65, k64 = _keys(65, 2), _keys(64, 3)
    J.put(A, k65)
    ar = [J.arena]
    f = "msd_pack_low16_u32"
    _refused(ctx, f, (None, 65, J.at(0)), ar, "null pointer")
    _refused(ctx, f, (J.at(A), 65, None), ar, "null pointer")
    _refused(ctx, f, (J.at(A + 4), 65, J.at(0)), ar, "16-byte aligned")             # the source one element off the grid
    _refused(ctx, f, (J.at(A), 65, J.at(2)), ar, "16-byte aligned")                 # the destination one element off
    _refused(ctx, f, (J.at(A), 65, J.at(A + 2 - 130)), ar, "overlap")               # its last element is the source's first half key
    _refused(ctx, f, (J.at(A), 65, J.at(A + 260 - 4)), ar, "overlap")               # it starts on the source's last key
    _refused(ctx, f, (J.at(A), 65, J.at(A)), ar, "overlap")
    # an empty source inside the destination (and null pointers with it): MSD_OK, nothing happens
    before = _bits(J.arena)
    _accepted(ctx, f, (J.at(A + 16), 0, J.at(A)), ar)
    _accepted(ctx, f, (None, 0, None), ar)
    assert (_bits(J.arena) == before).all()
    # exactly adjacent, in front of the source and behind it: accepted, and right
    J.put(A, k64)
    for D in (A - 128, A + 256):
        J.arena.fill(J.fill)
        _accepted(ctx, f, (J.at(A), 64, J.at(D)), ar)
        assert (J.unchanged_except(D, 128).view(np.uint16) == (k64 & np.uint32(0xFFFF)).astype(np.uint16)).all(), D


# ------------------------------------------------------------------ msd_hist2_pack_u32, msd_hist2_pack_u32_low16

@pytest.mark.parametrize("es", [4, 2])
def test_hist2_pack_refusals(ctx, es):
    import torch
    f = "msd_hist2_pack_u32" if es == 4 else "msd_hist2_pack_u32_low16"
    R = int(ctx._L.msd_hist2_record_bytes())
    assert R == ctx.HIST2_RECORD_BYTES and R % 16 == 0
    nb, REC = 2, 2 * R                                                 # two buckets: two records
    A = REC + 1024                                                     # the keys' offset; room for the records on either side
    J = _Joint(A + 1024 + REC + 1024, 10 + es)
    k65, k64 = _keys(65, 11), _keys(64, 12)
    src = (lambda k: k if es == 4 else (k & np.uint32(0xFFFF)).astype(np.uint16))
    J.put(A, src(k65))
    bounds, flag = _arena(np.array([0, 30, 65], dtype=np.uint64)), _arena(np.array([0x5A5A5A5A], dtype=np.uint32))
    ar = [J.arena, bounds, flag]
    K, B, F, D0 = J.at(A), bounds.ptr, flag.ptr, J.at(0)
    for args in ((None, 65, B, nb, D0, REC, F), (K, 65, None, nb, D0, REC, F), (K, 65, B, nb, None, REC, F), (K, 65, B, nb, D0, REC, None)):
        _refused(ctx, f, args, ar, "null pointer")
    _refused(ctx, f, (K, 65, B, 0, D0, REC, F), ar, "1..65536 buckets")
    _refused(ctx, f, (K, 65, B, 65537, D0, REC, F), ar, "1..65536 buckets")
    _refused(ctx, f, (J.at(A + es), 65, B, nb, D0, REC, F), ar, "16-byte aligned")   # the keys one element off the grid
    _refused(ctx, f, (K, 65, B, nb, J.at(1), REC, F), ar, "16-byte aligned")         # the records one byte off
    _refused(ctx, f, (K, 65, B, nb, D0, REC - 1, F), ar, "do not fit")
    _refused(ctx, f, (K, 65, B, nb, J.at(A + 16 - REC), REC, F), ar, "overlap")      # the records end 16 bytes into the keys
    _refused(ctx, f, (K, 65, B, nb, J.at(A + 65 * es - es), REC, F), ar, "overlap")  # they start on the last key
    _refused(ctx, f, (K, 65, B, nb, K, REC, F), ar, "overlap")
    _refused(ctx, f, (J.at(16), 0, B, nb, D0, REC, F), ar, "overlap")                # an empty source inside the destination
    # exactly adjacent: accepted; the records, merged, are the sorted keys
    J.put(A, src(k64))
    bounds.fill(np.array([0, 30, 64], dtype=np.uint64))
    counts = torch.tensor([[30, 34]], dtype=torch.int64, device="cuda")
    for D in (A - REC, A + 64 * es):
        J.arena.fill(J.fill)
        _accepted(ctx, f, (K, 64, B, nb, J.at(D), REC, F), ar)
        J.unchanged_except(D, REC)
        assert int(flag.host(np.uint32)[0]) == 0
        dst = _arena(np.zeros(64, dtype=np.uint32))
        ctx.merge_buckets(J.view(D, REC), counts, [0], 16, 0, dst.payload, 64)
        dst.check("merge of the records")
        assert (dst.host(np.uint32) == np.sort(k64)).all(), D


# ------------------------------------------------------------------ msd_order_low16_counts_u32, msd_order_low16_scatter_u32

def test_order_low16_refusals(ctx):
    rng = np.random.default_rng(20)
    J = _Joint(4096, 21)
    A = 1024
    k65 = rng.integers(0, 1 << 32, 65, dtype=np.uint64).astype(np.uint32)
    k64 = k65[:64].copy()
    J.put(A, k65)
    counts = _arena(np.zeros(65536, dtype=np.uint64))
    ar = [J.arena, counts]
    fc, fs = "msd_order_low16_counts_u32", "msd_order_low16_scatter_u32"
    K, CN = J.at(A), counts.ptr
    _refused(ctx, fc, (K, 65, None), ar, "null pointer")
    _refused(ctx, fc, (None, 65, CN), ar, "null pointer")
    _refused(ctx, fc, (J.at(A + 4), 65, CN), ar, "16-byte aligned")                 # one element off the grid
    _refused(ctx, fc, (K, 1 << 40, CN), ar, "too many keys")
    _refused(ctx, fs, (K, 65, None), ar, "null pointer")
    _refused(ctx, fs, (None, 65, J.at(0)), ar, "null pointer")
    _refused(ctx, fs, (K, 65, J.at(0)), ar, "not preceded")                          # no counts call at all
    # the counts call does run: it orders the keys in place by their top 8 bits and fills `counts`
    def count(n):
        _accepted(ctx, fc, (K, n, CN), ar)
        J.fill[A:A + 4 * n] = _bits(J.arena)[A:A + 4 * n]
        assert (counts.host(np.uint64) == np.bincount(k65[:n] >> np.uint32(16), minlength=65536)).all()
    count(65)
    _refused(ctx, fs, (K, 64, J.at(0)), ar, "not preceded")                          # another length (the counts stay pending)
    _refused(ctx, fs, (K, 65, J.at(2)), ar, "16-byte aligned")                       # the destination one element off the grid
    _refused(ctx, fs, (K, 65, J.at(0)), ar, "not preceded")                          # (that refusal spent the counts call)
    for D, word in ((A + 2 - 130, "overlap"), (A + 260 - 4, "overlap"), (A, "overlap")):
        count(65)
        _refused(ctx, fs, (K, 65, J.at(D)), ar, word)
    # exactly adjacent: accepted; bucket after bucket the low halves of that bucket's keys
    J.put(A, k64)
    for D in (A - 128, A + 256):
        J.arena.fill(J.fill)
        count(64)
        _accepted(ctx, fs, (K, 64, J.at(D)), ar)
        low = J.unchanged_except(D, 128).view(np.uint16)
        sizes = counts.host(np.uint64).astype(np.int64)
        rebuilt = (np.repeat(np.arange(65536, dtype=np.uint32), sizes) << np.uint32(16)) | low.astype(np.uint32)
        assert (np.sort(rebuilt) == np.sort(k64)).all(), D


# ------------------------------------------------------------------ the small services

@pytest.mark.parametrize("es", [4, 8])
def test_histogram_and_bucket_bounds_refusals(ctx, es):
    sfx = "u32" if es == 4 else "u64"
    keys = _arena(np.sort(np.random.default_rng(30).integers(0, 1 << 31, 64, dtype=np.uint64).astype(_NP[es])))
    out = _arena(np.full(4096 + 1, 0x1234567, dtype=np.uint64))
    ar = [keys, out]
    f = "msd_histogram_" + sfx
    _refused(ctx, f, (keys.ptr, 64, 0, 8, None), ar, "null pointer")
    _refused(ctx, f, (None, 64, 0, 8, out.ptr), ar, "null pointer")
    _refused(ctx, f, (keys.ptr, 64, 0, 0, out.ptr), ar, "radix_bits must be 1..12")
    _refused(ctx, f, (keys.ptr, 64, 0, 13, out.ptr), ar, "radix_bits must be 1..12")
    _refused(ctx, f, (keys.ptr, 64, 8 * es - 7, 8, out.ptr), ar, "radix_bits must be 1..12")   # the digit leaves the key
    _refused(ctx, f, (keys.ptr + es, 63, 0, 8, out.ptr), ar, "16-byte aligned")                # one element off the grid
    f = "msd_bucket_bounds_" + sfx
    _refused(ctx, f, (keys.ptr, 64, 16, 0, 4, None), ar, "null pointer")
    _refused(ctx, f, (None, 64, 16, 0, 4, out.ptr), ar, "null pointer")
    _refused(ctx, f, (keys.ptr, 64, 8 * es, 0, 4, out.ptr), ar, "out of range")
    _refused(ctx, f, (keys.ptr, 64, 16, 0, 0, out.ptr), ar, "out of range")
    _refused(ctx, f, (keys.ptr, 64, 16, 0, (1 << 24) + 1, out.ptr), ar, "out of range")


@pytest.mark.parametrize("es", [4, 8])
def test_gather_sample_splitters_refusals(ctx, es):
    sfx = "u32" if es == 4 else "u64"
    src = _arena(np.sort(np.random.default_rng(40).integers(0, 1 << 31, 64, dtype=np.uint64).astype(_NP[es])))
    dst = _arena(np.full(64, 7, dtype=_NP[es]))
    ar = [src, dst]
    one = lambda v: (C.c_uint64 * 1)(v)
    so, do, ln = one(0), one(0), one(64)
    f = "msd_gather_runs_" + sfx
    for args in ((None, src.ptr, so, do, ln, 1), (dst.ptr, None, so, do, ln, 1), (dst.ptr, src.ptr, None, do, ln, 1),
                 (dst.ptr, src.ptr, so, None, ln, 1), (dst.ptr, src.ptr, so, do, None, 1)):
        _refused(ctx, f, args, ar, "null pointer")
    f = "msd_sample_" + sfx
    _refused(ctx, f, (None, 64, 8, 1, dst.ptr), ar, "null pointer or empty input")
    _refused(ctx, f, (src.ptr, 64, 8, 1, None), ar, "null pointer or empty input")
    _refused(ctx, f, (src.ptr, 0, 8, 1, dst.ptr), ar, "null pointer or empty input")
    f = "msd_splitters_" + sfx
    _refused(ctx, f, (src.ptr, 64, 0, dst.ptr), ar, "parts must be 1..256")
    _refused(ctx, f, (src.ptr, 64, 257, dst.ptr), ar, "parts must be 1..256")
    _refused(ctx, f, (None, 64, 4, dst.ptr), ar, "null pointer or empty sample")
    _refused(ctx, f, (src.ptr, 64, 4, None), ar, "null pointer or empty sample")
    _refused(ctx, f, (src.ptr, 0, 4, dst.ptr), ar, "null pointer or empty sample")

"""Host-side mirror of the reference's interface for the hot path.

The reference is a C library with one public call, ``sort(keys, rids, size,
threads, numa, fudge, description, times)`` (include/msb_64.h:37-39) plus
``mamalloc`` and the test hook ``check`` (src/msb_64.c:2470).  :func:`sort`,
:func:`mamalloc` and :func:`check` below keep those names, argument meaning and
error behaviour on numpy host arrays; :class:`MsdContext` wraps the typed
device-resident entry points of include/msd_radix_hip.h on torch tensors (torch
only supplies device memory and the stream).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _args, _lib
from ._args import MsdError, _torch, ptr   # (the argument rules, their error and the null-or-address of a tensor live in _args.py)


# Every name msd_stat knows (the table of csrc/msd_options.hpp; the C ABI cannot enumerate them, so
# tests/test_option_defaults.py holds the two equal).
STAT_NAMES = ("rounds", "parents", "stripes", "children", "slots", "holes", "chain_steps",
              "small_segments", "count_segments", "big_count_segments", "direct_rounds", "regpart_rounds", "skipped_bits", "bit_skip_restarts", "bit_skip_checked_by_histogram",
              "leaves_behind_round", "rounds_planned_early", "front_count_sorts", "front_count_declined", "excess_blocks", "child_scan_split_rounds", "count16_rejected", "count_slow_segments",
              "merge_rejected", "leaf17_segments", "leaf17_rejected", "leaf17_slow_segments", "leaf17_launches", "workspace_bytes",
              "select_hist_passes", "select_skipped_bits", "select_candidates", "select_below",
              "topk_rows_kernel_rows", "topk_rows_looped_rows",
              "sort_rows_kernel_rows", "sort_rows_segment_rows", "sort_rows_lanes",
              "sort_keys_split", "sort_keys_reversed")   # (these two wait for the stream: include/msd_sort_keys_hip.h)


class MsdContext:
    """One sorting context (device + stream + auxiliary workspace)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._L = _lib.load()
        h = C.c_void_p()
        rc = self._L.msd_create(C.byref(h), device, C.c_void_p(stream or 0))
        if rc != 0 or not h:
            raise MsdError(f"msd_create(device={device}) failed with {rc}: no usable HIP device "
                           "(this library has no CPU fallback)")
        self._h = h
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.msd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    def _ok(self, rc: int) -> None:
        if rc != 0:
            raise MsdError(f"error {rc}: {self._L.msd_last_error(self._h).decode()}")

    def _on_gpu(self, *tensors) -> None:
        """Refuses a tensor that does not live on the context's GPU (``None``: an absent one); the library is not touched."""
        if any(not t.is_cuda or t.device.index != self.device for t in tensors if t is not None):
            raise MsdError("the tensors must live on the context's GPU")

    def _ptr(self, t, dtype_size: int) -> C.c_void_p:
        self._on_gpu(t)
        if not t.is_contiguous() or t.element_size() != dtype_size:
            raise MsdError("tensor must be contiguous with the expected element size")
        return ptr(t)

    _check_positions = staticmethod(_args.positions)

    def _layout(self, stem: str, keys, rids=None):
        """``(export, pointers)`` for the key layout: the export named ``stem`` with ``_u32``, ``_u64`` or -- with ``rids`` --
        ``_pairs_u64`` in place of its ``{}``, and the checked pointers its arguments open with, the keys' and the rids'."""
        if rids is not None:
            layout, ptrs = "_pairs_u64", (self._ptr(keys, 8), self._ptr(rids, 8))
        elif keys.element_size() == 4:
            layout, ptrs = "_u32", (self._ptr(keys, 4),)
        else:
            layout, ptrs = "_u64", (self._ptr(keys, 8),)
        return getattr(self._L, stem.format(layout)), ptrs

    def _value_index_outputs(self, shape, keys, out, out_indices, want_idx: bool, exact: bool = True):
        """``(out, out_indices)``: the values (the keys' dtype) and, with ``want_idx``, the int64 positions, allocated with
        ``shape`` where not given.  ``exact``: contiguous tensors of exactly that shape on the context's GPU; otherwise 1-D
        tensors of at least ``shape[0]`` elements (:meth:`_ptr` looks at the rest).  Both dtypes are looked at before
        either shape, so the checks stand here for the pair and :func:`_args.output` only allocates."""
        torch = _torch()
        out = _args.output(out, keys.dtype, shape, None, keys.device)
        if want_idx:
            out_indices = _args.output(out_indices, torch.int64, shape, None, keys.device)
        outs = (out, out_indices) if want_idx else (out,)
        if out.dtype != keys.dtype or (want_idx and out_indices.dtype != torch.int64):
            raise MsdError("the values have the keys' dtype, the indices are int64")
        if not exact and any(t.numel() < shape[0] for t in outs):
            raise MsdError("output tensor shorter than k")
        if exact and any(tuple(t.shape) != shape or not t.is_contiguous() for t in outs):
            raise MsdError(f"an output must be a contiguous tensor of shape {shape}")
        if exact:
            self._on_gpu(keys, *outs)
        return out, out_indices

    def _sorted_with_positions(self, flat):
        """``(sorted copy, positions)`` of a 1-D tensor: :meth:`sort_rows` for 32-bit, :meth:`sort_typed` with rids for 64-bit keys."""
        if flat.element_size() == 4:
            return self.sort_rows(flat, indices=True)
        torch = _torch()
        s = flat.clone()
        positions = torch.arange(flat.numel(), dtype=torch.int64, device=flat.device)
        self.sort_typed(s, rids=positions)
        return s, positions

    def _limits(self, export: str, words: int, arg, what: Optional[str] = None, indices: bool = False):
        """The ``words`` numbers the ``*_limits`` call ``export`` answers with (one: the number, else a tuple).  ``arg`` is an
        element width that the message calls ``what``, or -- without ``what`` -- a key type or a tensor that has one, asked
        about with or without ``indices``."""
        if what is None and not isinstance(arg, int):
            arg = self._key_type(arg)
        cells = [C.c_uint64() for _ in range(words)]
        asked = (int(arg),) if what else (arg, int(indices))
        if getattr(self._L, export)(*asked, *[C.byref(c) for c in cells]) != 0:
            raise MsdError(f"error -1: {what} must be 4 or 8, not {arg}" if what else f"error -1: unknown key type {arg}")
        return tuple(int(c.value) for c in cells) if words > 1 else int(cells[0].value)

    def use_torch_stream(self) -> None:
        torch = _torch()
        self._ok(self._L.msd_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def reserve(self, n: int, key_bytes: int, val_bytes: int = 0) -> None:
        self._ok(self._L.msd_reserve(self._h, n, key_bytes, val_bytes))

    @property
    def workspace_bytes(self) -> int:
        return int(self._L.msd_workspace_bytes(self._h))

    # ---- the sort
    def sort_u32(self, keys, end_bit: int = 32) -> None:
        self._ok(self._L.msd_sort_u32_bits(self._h, self._ptr(keys, 4), keys.numel(), end_bit))

    def sort_u64(self, keys, end_bit: int = 64) -> None:
        self._ok(self._L.msd_sort_u64_bits(self._h, self._ptr(keys, 8), keys.numel(), end_bit))

    def sort_pairs_u64(self, keys, rids, end_bit: int = 64) -> None:
        if keys.numel() != rids.numel():
            raise MsdError("keys and rids differ in length")
        self._ok(self._L.msd_sort_pairs_u64_bits(self._h, self._ptr(keys, 8), self._ptr(rids, 8), keys.numel(), end_bit))

    # ---- the sort for every key type and both directions (include/msd_sort_keys_hip.h)
    REVERSE_TILE = {4: 4092, 8: 2046}   # elements one workgroup of the reversal kernel takes from each end of a range

    def sort_typed(self, keys, descending: bool = False, rids=None) -> None:
        """Sorts the 1-D contiguous tensor ``keys`` in place in the order of its dtype (float32, int32, float64, int64,
        uint32, uint64), ascending or ``descending``; floats in IEEE-754 totalOrder as :meth:`topk_typed`, every key
        bit-exact.  ``rids`` (int64, same length; 64-bit keys only) move with their keys; tuples with equal keys come out
        in any order."""
        torch = _torch()
        kt = self._key_type(keys)
        es = keys.element_size()
        _args.one_dim("sort_typed", keys, rids)
        order = 1 if descending else 0
        if rids is not None and es != 8:
            raise MsdError("tuples have 64-bit keys: float64, int64 or uint64")
        if rids is not None and (rids.dtype != torch.int64 or rids.numel() != keys.numel()):
            raise MsdError("rids must be int64 and as many as the keys")
        kp = self._ptr(keys, es)   # (a tensor that is not on the context's GPU is refused here, before the library is touched)
        if rids is None:
            self._ok(self._L.msd_sort_keys(self._h, kp, kt, keys.numel(), order))
        else:
            self._ok(self._L.msd_sort_pairs_keys(self._h, kp, kt, self._ptr(rids, 8), keys.numel(), order))

    def reverse(self, t, first: int = 0, count: Optional[int] = None) -> None:
        """Reverses elements ``[first, first + count)`` (``count`` None: to the end) of the 1-D contiguous tensor ``t`` of
        4- or 8-byte elements in place; asynchronous."""
        es = t.element_size()
        if es not in (4, 8) or t.dim() != 1:
            raise MsdError("reverse takes a 1-D tensor of 4- or 8-byte elements")
        count = t.numel() - first if count is None else count
        if first < 0 or count < 0 or first + count > t.numel():
            raise MsdError("reverse: the range lies outside the tensor")
        p = self._ptr(t, es)
        self._ok(self._L.msd_reverse(self._h, p, es, first, count))

    # ---- fine-grained sharding (include/msd_radix_hip.h): top digits before the exchange, open bits after it
    def sort_top(self, keys, begin_bit: int, end_bit: Optional[int] = None, rids=None) -> None:
        """Orders ``keys`` by ``key >> begin_bit`` only (keys that agree above ``begin_bit`` end up adjacent, in any order)."""
        eb = keys.element_size() * 8 if end_bit is None else end_bit
        f, ptrs = self._layout("msd_sort{}_top", keys, rids)
        self._ok(f(self._h, *ptrs, keys.numel(), eb, begin_bit))

    def bucket_bounds(self, keys, shift: int, nbuckets: int, first: int = 0):
        """int64[nbuckets + 1] on the device: bounds[b] = first index whose ``key >> shift`` is >= first + b
        (``keys`` ordered by ``key >> shift``)."""
        torch = _torch()
        out = torch.empty(nbuckets + 1, dtype=torch.int64, device=keys.device)
        f, ptrs = self._layout("msd_bucket_bounds{}", keys)
        self._ok(f(self._h, *ptrs, keys.numel(), shift, first, nbuckets, ptr(out)))
        return out

    def merge_buckets(self, src, counts, src_base, open_bits: int, first_prefix: int, dst, n_expected: int) -> None:
        """Finishes the buckets a rank received: ``counts`` = int64[nsrc, nbuckets] on the device (extent lengths per
        source row and bucket), source x's extents lie back to back in ``src`` from ``src_base[x]`` on; the sorted
        buckets are written back to back into ``dst``."""
        nsrc, nb = int(counts.shape[0]), int(counts.shape[1])
        if len(src_base) != nsrc:
            raise MsdError("merge_buckets: one base offset per source row")
        if src.element_size() == 1:   # histogram records (hist2_pack): source x's at x * nb * HIST2_RECORD_BYTES
            if open_bits != 16:
                raise MsdError("merge_buckets: histogram records need 16 open bits")
            self._ok(self._L.msd_merge_buckets_u32_hist2(self._h, self._ptr(src, 1), src.numel(), self._ptr(counts, 8), nsrc, nb,
                                                         first_prefix, self._ptr(dst, 4), dst.numel(), n_expected))
            return
        if src.element_size() == 2:   # extents of low halves (pack_low16): the upper half of a key is its bucket's number
            if open_bits != 16:
                raise MsdError("merge_buckets: extents of low halves need 16 open bits")
            self._ok(self._L.msd_merge_buckets_u32_low16(self._h, self._ptr(src, 2), src.numel(), self._ptr(counts, 8), self._u64arr(src_base),
                                                         nsrc, nb, first_prefix, self._ptr(dst, 4), dst.numel(), n_expected))
            return
        self._ok(self._L.msd_merge_buckets_u32(self._h, self._ptr(src, 4), src.numel(), self._ptr(counts, 8), self._u64arr(src_base),
                                               nsrc, nb, open_bits, first_prefix, self._ptr(dst, 4), dst.numel(), n_expected))

    HIST2_RECORD_BYTES = 17408

    def hist2_pack(self, keys, bounds, rec):
        """``rec`` (uint8, >= (bounds.numel() - 1) * HIST2_RECORD_BYTES) <- one histogram record per bucket of the u32 ``keys``
        (ordered by their upper halves; ``bounds`` from :meth:`bucket_bounds` with shift 16).  Returns a one-element int32
        tensor on the device: non-zero = some bucket does not fit a record (send the low halves instead)."""
        torch = _torch()
        nb = bounds.numel() - 1
        es = keys.element_size()        # 4: whole keys; 2: the low halves order_low16 has written (half the bytes to read)
        if es not in (2, 4) or rec.element_size() != 1 or rec.numel() < nb * self.HIST2_RECORD_BYTES:
            raise MsdError("hist2_pack: u32 keys or their low halves, a uint8 buffer of one record per bucket")
        flag = torch.zeros(1, dtype=torch.int32, device=keys.device)
        f = self._L.msd_hist2_pack_u32 if es == 4 else self._L.msd_hist2_pack_u32_low16
        self._ok(f(self._h, self._ptr(keys, es), keys.numel(), self._ptr(bounds, 8), nb, self._ptr(rec, 1), rec.numel(), ptr(flag)))
        return flag

    def bounds_from_counts16(self, counts):
        """int64[65537] on the device: the prefix sums of 65536 bucket sizes."""
        torch = _torch()
        out = torch.empty(65537, dtype=torch.int64, device=counts.device)
        self._ok(self._L.msd_bounds_from_counts16(self._h, self._ptr(counts, 8), ptr(out)))
        return out

    def order_low16(self, keys, out):
        """Orders the u32 ``keys`` by their upper halves and writes only their low halves: ``out`` (int16, >= keys.numel())
        holds bucket after bucket (bucket = upper half), in any order inside a bucket; returns the 2^16 bucket sizes (int64,
        on the device).  ``keys`` is left ordered by its top 8 bits."""
        torch = _torch()
        if keys.element_size() != 4 or out.element_size() != 2 or out.numel() < keys.numel():
            raise MsdError("order_low16: u32 keys, an int16 buffer at least as long")
        counts = torch.empty(65536, dtype=torch.int64, device=keys.device)
        self._ok(self._L.msd_order_low16_u32(self._h, self._ptr(keys, 4), keys.numel(), self._ptr(out, 2), ptr(counts)))
        return counts

    def order_low16_counts(self, keys):
        """First half of :meth:`order_low16`: the 2^16 bucket sizes (ready in stream order); :meth:`order_low16_scatter` must
        be this context's next call."""
        torch = _torch()
        counts = torch.empty(65536, dtype=torch.int64, device=keys.device)
        self._ok(self._L.msd_order_low16_counts_u32(self._h, self._ptr(keys, 4), keys.numel(), ptr(counts)))
        return counts

    def order_low16_scatter(self, keys, out) -> None:
        if out.element_size() != 2 or out.numel() < keys.numel():
            raise MsdError("order_low16: an int16 buffer at least as long as the keys")
        self._ok(self._L.msd_order_low16_scatter_u32(self._h, self._ptr(keys, 4), keys.numel(), self._ptr(out, 2)))

    def pack_low16(self, keys, out) -> None:
        """``out`` (int16, >= keys.numel() elements) <- the low 16 bits of the u32 ``keys``, in order."""
        if keys.element_size() != 4 or out.element_size() != 2 or out.numel() < keys.numel():
            raise MsdError("pack_low16: u32 keys, an int16 buffer at least as long")
        self._ok(self._L.msd_pack_low16_u32(self._h, self._ptr(keys, 4), keys.numel(), self._ptr(out, 2)))

    # ---- building blocks
    def histogram(self, keys, shift: int, radix_bits: int):
        torch = _torch()
        out = torch.empty(1 << radix_bits, dtype=torch.int64, device=keys.device)
        f, ptrs = self._layout("msd_histogram{}", keys)
        self._ok(f(self._h, *ptrs, keys.numel(), shift, radix_bits, ptr(out)))
        return out

    def exclusive_scan(self, x):
        torch = _torch()
        out = torch.empty_like(x)
        self._ok(self._L.msd_exclusive_scan_u64(self._h, self._ptr(x, 8), ptr(out), x.numel()))
        return out

    def partition(self, keys, shift: int, radix_bits: int, rids=None):
        """One in-place digit pass; returns the bucket sizes (int64 tensor)."""
        torch = _torch()
        cnt = torch.zeros(1 << radix_bits, dtype=torch.int64, device=keys.device)
        f, ptrs = self._layout("msd_partition{}", keys, rids)
        self._ok(f(self._h, *ptrs, keys.numel(), shift, radix_bits, ptr(cnt)))
        return cnt

    # ---- a rank of the multi-GPU sort after its exchange (reference: local sorting of whole key ranges, src/msb_64.c:2200-2255)
    @staticmethod
    def _u64arr(xs):
        """Host array of uint64 for the C ABI (a numpy array goes through without a per-element conversion)."""
        a = np.ascontiguousarray(xs, dtype=np.uint64)
        p = a.ctypes.data_as(C.POINTER(C.c_uint64))
        p._keep = a   # the array must outlive the call
        return p

    def sort_segments(self, keys, seg_off, end_bit: int, rids=None) -> None:
        """Sorts the independent segments [seg_off[i], seg_off[i+1]) on their low ``end_bit`` bits in one call
        (``seg_off``: nseg + 1 ascending element offsets on the host)."""
        nseg = len(seg_off) - 1
        if nseg <= 0:
            return
        off = self._u64arr(seg_off)
        f, ptrs = self._layout("msd_sort{}_segments", keys, rids)
        self._ok(f(self._h, *ptrs, keys.numel(), off, nseg, end_bit))

    def gather_runs(self, dst, src, src_off, dst_off, lens) -> None:
        """Copies run i (``lens[i]`` elements) from ``src[src_off[i]:]`` to ``dst[dst_off[i]:]``, all runs in one launch."""
        if not (len(src_off) == len(dst_off) == len(lens)):
            raise MsdError("gather_runs: the three lists differ in length")
        if dst.element_size() != src.element_size():
            raise MsdError("gather_runs: element sizes differ")
        dp = self._ptr(dst, dst.element_size())
        f, ptrs = self._layout("msd_gather_runs{}", src)
        self._ok(f(self._h, dp, *ptrs, self._u64arr(src_off), self._u64arr(dst_off), self._u64arr(lens), len(lens)))

    # ---- splitter service (reference: src/msb_64.c:1511-1521, :1304-1322, :188-204)
    def sample(self, keys, m: int, seed: int = 0x5EED0007):
        """m keys drawn from the (unsorted) tensor at pseudo-random positions mulhi(splitmix64(seed + i), n);
        u32 (int32 tensor) or u64 (int64 tensor) keys."""
        torch = _torch()
        out = torch.empty(m, dtype=keys.dtype, device=keys.device)
        f, ptrs = self._layout("msd_sample{}", keys)
        self._ok(f(self._h, *ptrs, keys.numel(), m, seed, ptr(out)))
        return out

    def splitters(self, sorted_sample, parts: int):
        """parts-1 equi-depth delimiters (bit patterns in a tensor of the sample's dtype) with the reference's duplicate rule."""
        torch = _torch()
        out = torch.empty(max(parts - 1, 0), dtype=sorted_sample.dtype, device=sorted_sample.device)
        f, ptrs = self._layout("msd_splitters{}", sorted_sample)
        self._ok(f(self._h, *ptrs, sorted_sample.numel(), parts, ptr(out)))
        return out

    sample_u32 = sample          # (round 2's names)
    splitters_u32 = splitters

    def partition_by_splitters(self, keys, delims, parts: int, rids=None):
        """One in-place pass: range p = keys in (delims[p-1], delims[p]] (rids move with their keys); returns the range
        sizes (int64 tensor)."""
        torch = _torch()
        cnt = torch.zeros(parts, dtype=torch.int64, device=keys.device)
        dp = self._ptr(delims, keys.element_size()) if parts > 1 else ptr(None)
        f, ptrs = self._layout("msd_partition_by_splitters{}", keys, rids)
        self._ok(f(self._h, *ptrs, keys.numel(), dp, parts, ptr(cnt)))
        return cnt

    def check(self, keys, rids=None) -> Tuple[int, int, int]:
        """(violations, sum, xor): device form of the reference's check()."""
        v, s, x = C.c_uint64(), C.c_uint64(), C.c_uint64()
        f, ptrs = self._layout("msd_check{}", keys)
        if keys.element_size() != 4:   # (the 64-bit export takes the rids, or null, behind the keys)
            ptrs += (self._ptr(rids, 8) if rids is not None else ptr(None),)
        self._ok(f(self._h, *ptrs, keys.numel(), C.byref(v), C.byref(s), C.byref(x)))
        return int(v.value), int(s.value), int(x.value)

    # ---- radix select and top-k (read-only on ``keys``)
    def topk(self, keys, k: int, largest: bool = False, rids=None, out=None, out_rids=None):
        """The ``k`` smallest (``largest``: largest) keys in ascending order: a slice of the sorted array.  ``keys`` (int32 /
        int64 tensors holding u32 / u64 keys) and ``rids`` are not modified.  Returns ``out`` (allocated when not given), or
        ``(out, out_rids)`` for tuples."""
        torch = _torch()
        es = keys.element_size()
        which = 1 if largest else 0
        if rids is not None and (es != 8 or rids.numel() != keys.numel()):
            raise MsdError("tuples are (u64 key, u64 rid) arrays of equal length")
        if out is None:
            out = torch.empty(max(int(k), 0), dtype=keys.dtype, device=keys.device)
        if rids is not None and out_rids is None:
            out_rids = torch.empty(max(int(k), 0), dtype=rids.dtype, device=rids.device)
        if out.numel() < k or (rids is not None and out_rids.numel() < k):
            raise MsdError("output tensor shorter than k")
        f, ptrs = self._layout("msd_topk{}", keys, rids)
        outs = (out,) if rids is None else (out, out_rids)
        self._ok(f(self._h, *ptrs, keys.numel(), k, which, *[self._ptr(t, es) for t in outs]))
        return out if rids is None else outs

    def select(self, keys, k: int, largest: bool = False) -> int:
        """The key of rank ``k`` (0-based) from the small end, or from the large end with ``largest``; ``keys`` is not modified."""
        f, ptrs = self._layout("msd_select{}", keys)
        v = (C.c_uint32 if keys.element_size() == 4 else C.c_uint64)()
        self._ok(f(self._h, *ptrs, keys.numel(), k, 1 if largest else 0, C.byref(v)))
        return int(v.value)

    # ---- top-k with indices, signed and float keys: the tensor's dtype says how its bit patterns are ordered
    KEY_U32, KEY_I32, KEY_F32, KEY_U64, KEY_I64, KEY_F64 = (_args.KEY_U32, _args.KEY_I32, _args.KEY_F32, _args.KEY_U64, _args.KEY_I64,
                                                            _args.KEY_F64)   # MSD_KEY_* of include/msd_radix_hip.h
    _key_type = staticmethod(_args.key_type)

    def topk_typed(self, keys, k: int, largest: bool = False, indices: bool = False, out=None, out_indices=None):
        """The ``k`` smallest (``largest``: largest) keys of ``keys`` in the order of its dtype, ascending in both cases: a
        slice of the sorted array, bit-exact.  Floats are ordered by IEEE-754 totalOrder (-NaN < -inf < ... < -0 < +0 < ...
        < +inf < +NaN), which differs from ``torch.topk`` only for NaNs with the sign bit set and in telling -0 from +0.
        With ``indices`` (or ``out_indices``) returns ``(values, positions)``: int64 positions with
        ``keys[positions[j]]`` bit-equal to ``values[j]``, none twice; which of several keys equal to the boundary key
        are taken is unspecified.  ``keys`` is not modified."""
        kt = self._key_type(keys)
        es = keys.element_size()
        want_idx = indices or out_indices is not None
        out, out_indices = self._value_index_outputs((max(int(k), 0),), keys, out, out_indices, want_idx, exact=False)
        self._ok(self._L.msd_topk_keys(self._h, self._ptr(keys, es), kt, keys.numel(), k, 1 if largest else 0, self._ptr(out, es),
                                       self._ptr(out_indices, 8) if want_idx else ptr(None)))
        return (out, out_indices) if want_idx else out

    def select_typed(self, keys, k: int, largest: bool = False):
        """The key of rank ``k`` (0-based) from the small end, or from the large end with ``largest``, in the order of the
        tensor's dtype, as a python float / int (-0.0 stays -0.0 and a NaN keeps its sign; the payload of a float32 NaN is
        only exact through ``msd_select_key`` itself, a python float being a double)."""
        kt = self._key_type(keys)
        es = keys.element_size()
        v = (C.c_uint32 if es == 4 else C.c_uint64)()
        self._ok(self._L.msd_select_key(self._h, self._ptr(keys, es), kt, keys.numel(), k, 1 if largest else 0, C.byref(v)))
        raw = np.array([v.value], dtype=np.uint32 if es == 4 else np.uint64)
        if kt in (self.KEY_F32, self.KEY_F64):
            return float(raw.view(np.float32 if es == 4 else np.float64)[0])
        if kt in (self.KEY_I32, self.KEY_I64):
            return int(raw.view(np.int32 if es == 4 else np.int64)[0])
        return int(v.value)

    # ---- per-row (batched) top-k: torch.topk(x, k, dim=-1)
    @staticmethod
    def _rows_layout(keys) -> Tuple[int, int, int]:
        """``(rows, row_len, row_stride)`` of a tensor whose last dimension holds the rows, or :class:`MsdError`: the last
        dimension must have stride 1 and the leading dimensions must collapse to ONE row stride >= row_len (a contiguous
        tensor, or a 2-D one with ``stride(0) >= size(1)``).  Needs no device; nothing is copied."""
        if keys.dim() < 1:
            raise MsdError("topk_rows needs a tensor with at least one dimension")
        sizes, strides = list(keys.shape), list(keys.stride())
        row_len = int(sizes[-1])
        if row_len > 1 and strides[-1] != 1:
            raise MsdError(f"the last dimension must have stride 1, not {strides[-1]} (no hidden copy is made: pass a contiguous tensor)")
        lead = [(int(n), int(st)) for n, st in zip(sizes[:-1], strides[:-1]) if n != 1]   # (a dimension of size 1 has no stride to speak of)
        rows = 1
        for n, _ in lead:
            rows *= n
        if rows <= 1 or not lead:
            return rows, row_len, row_len
        for (_, outer), (n, inner) in zip(lead[:-1], lead[1:]):
            if outer != n * inner:
                raise MsdError("the leading dimensions do not collapse to one row stride (no hidden copy is made: pass a contiguous tensor)")
        row_stride = lead[-1][1]
        if row_stride < row_len:
            raise MsdError(f"rows overlap: row stride {row_stride} < row length {row_len}")
        return rows, row_len, row_stride

    def topk_rows_limits(self, keys_or_key_type, indices: bool = False) -> Tuple[int, int]:
        """``(max_row_len, max_k)``: the envelope of the one-launch row kernel (``msd_topk_rows_limits``)."""
        return self._limits("msd_topk_rows_limits", 2, keys_or_key_type, indices=indices)

    def topk_rows(self, keys, k: int, largest: bool = False, indices: bool = False, out=None, out_indices=None):
        """Top-k along the LAST dimension: for every row the ``k`` smallest (``largest``: largest) keys in the order of the
        dtype, ascending in both cases and bit-exact, as :meth:`topk_typed` gives them for one array.  Returns values of
        shape ``[..., k]``; with ``indices`` (or ``out_indices``) also int64 positions within the row, of the same shape.
        ``keys`` is not modified and never copied: a layout that is not rows of stride 1 with one row stride is refused.
        Inside :meth:`topk_rows_limits` one kernel launch answers all rows and nothing blocks the host."""
        kt = self._key_type(keys)
        rows, row_len, row_stride = self._rows_layout(keys)
        self._on_gpu(keys)
        k = int(k)
        want_idx = indices or out_indices is not None
        out, out_indices = self._value_index_outputs(tuple(keys.shape[:-1]) + (max(k, 0),), keys, out, out_indices, want_idx)
        self._ok(self._L.msd_topk_rows(self._h, ptr(keys), kt, rows, row_len, row_stride, k, 1 if largest else 0,
                                       ptr(out), ptr(out_indices if want_idx else None)))
        return (out, out_indices) if want_idx else out

    # ---- per-row (batched) sort: torch.sort(x, dim=-1)
    def sort_rows_limits(self, keys_or_key_type, indices: bool = False) -> int:
        """``max_row_len``: the longest row the one-launch row kernel takes (``msd_sort_rows_limits``); longer rows go
        through the segment sort."""
        return self._limits("msd_sort_rows_limits", 1, keys_or_key_type, indices=indices)

    def sort_rows(self, keys, descending: bool = False, indices: bool = False, out=None, out_indices=None):
        """Sorts along the LAST dimension: every row in the order of the dtype (floats in IEEE-754 totalOrder, as
        :meth:`topk_typed`), ascending or ``descending``, bit-exact.  Returns values of the input's shape; with ``indices``
        (or ``out_indices``) also int64 positions within the row, of the same shape: ``keys[..., positions[..., j]]`` is
        bit-equal to ``values[..., j]`` and every row's positions are a permutation; the order among equal keys is
        unspecified.  ``keys`` is never copied: a layout that is not rows of stride 1 with one row stride is refused.
        ``out=keys`` sorts a contiguous tensor in place; otherwise ``keys`` is not modified.  Inside
        :meth:`sort_rows_limits` one kernel launch sorts all rows and nothing blocks the host."""
        kt = self._key_type(keys)
        rows, row_len, row_stride = self._rows_layout(keys)
        want_idx = indices or out_indices is not None
        out, out_indices = self._value_index_outputs(tuple(keys.shape), keys, out, out_indices, want_idx)
        self._ok(self._L.msd_sort_rows(self._h, ptr(keys), kt, rows, row_len, row_stride, 1 if descending else 0,
                                       ptr(out), ptr(out_indices if want_idx else None)))
        return (out, out_indices) if want_idx else out

    # ---- run-length encode and unique (include/msd_runs_hip.h)
    def run_encode_limits(self, elem_bytes: int) -> Tuple[int, int]:
        """``(tile, scan_tile)``: the elements one workgroup takes per tile for that element width, and how many tile
        counts one workgroup of the tile-count scan takes at once (``msd_run_encode_limits``)."""
        return self._limits("msd_run_encode_limits", 2, elem_bytes, "elem_bytes")

    def run_encode(self, t, cap: Optional[int] = None, values: bool = True, starts: bool = True, inverse: bool = False, positions=None):
        """Run-length encodes the 1-D contiguous tensor ``t`` of 4- or 8-byte elements (``torch.unique_consecutive``; on a
        sorted tensor the runs are the groups of equal keys).  A run is a maximal stretch of consecutive elements with
        equal BIT PATTERNS: -0.0 and +0.0 are two values, NaNs with equal sign and payload are one value, NaNs with
        different payloads differ -- unlike ``torch.unique``, which keeps every NaN apart.

        Returns ``(num_runs, values, starts, inverse)``; an output that was not asked for is ``None``.  ``num_runs`` is a
        one-element int64 tensor on the device: the true number of runs m, also when m > ``cap`` (default
        ``t.numel()``).  ``values`` (``cap`` elements, the dtype of ``t``) holds the value of run j and ``starts``
        (``cap + 1`` int64) the index of its first element, for j < min(m, cap); ``starts[min(m, cap)]`` closes the last
        stored run (``t.numel()`` if m <= cap), so counts are ``starts[1:] - starts[:-1]``; the rest of both is not
        written.  ``inverse`` (``t.numel()`` int64) holds the run number of every element; with ``positions`` (int64, a
        permutation of the indices as :meth:`sort_rows` or :meth:`sort_typed` with rids produce it)
        ``inverse[positions[i]]`` is the run of element i.  Nothing waits on the host."""
        torch = _torch()
        _args.flat("run_encode", t, what="a 1-D contiguous tensor")
        es = _args.elem_4_or_8("run_encode", t)
        n = t.numel()
        _args.positions(positions, n)
        if positions is not None and not inverse:
            raise MsdError("positions without inverse")
        cap = _args.cap_or(cap, n)
        self._on_gpu(t, positions)
        num = _args.count_cell(t.device)
        vals = torch.empty(cap, dtype=t.dtype, device=t.device) if values else None
        st = torch.empty(cap + 1, dtype=torch.int64, device=t.device) if starts else None
        inv = torch.empty(n, dtype=torch.int64, device=t.device) if inverse else None
        self._ok(self._L.msd_run_encode(self._h, ptr(t), es, n, cap, ptr(vals), ptr(st), ptr(positions), ptr(inv), ptr(num)))
        return num, vals, st, inv

    def unique(self, keys, return_inverse: bool = False, return_counts: bool = False):
        """``torch.unique(keys, sorted=True, return_inverse=..., return_counts=...)`` for a 1-D tensor of float32, int32,
        float64, int64, uint32 or uint64: the distinct values in the dtype's order, then the inverse (int64:
        ``values[inverse]`` is ``keys``) and the counts (int64) where asked for.  Floats are ordered by IEEE-754
        totalOrder and told apart by their BITS, as everywhere in this library: -0.0 and +0.0 are two values and NaNs
        with equal bits are one, where ``torch.unique`` merges the zeros and keeps every NaN apart.  ``keys`` is not
        modified.  One host wait beyond the sort's own: the number of distinct values sizes the results."""
        self._key_type(keys)   # (a dtype without a key order is refused here)
        _args.flat("unique", keys, what="a 1-D contiguous tensor")
        self._on_gpu(keys)
        if return_inverse:
            s, positions = self._sorted_with_positions(keys)
        else:
            s, positions = keys.clone(), None
            self.sort_typed(s)
        num, vals, st, inv = self.run_encode(s, starts=return_counts, inverse=return_inverse, positions=positions)
        m = int(num.item())
        out = (vals[:m],)
        if return_inverse:
            out += (inv,)
        if return_counts:
            out += (st[1:m + 1] - st[:m],)
        return out if len(out) > 1 else out[0]

    # ---- reduce-by-key over runs and group-by (include/msd_reduce_hip.h)
    REDUCE_OPS = {"sum": 0, "min": 1, "max": 2}   # MSD_REDUCE_* of include/msd_reduce_hip.h

    def reduce_runs_limits(self, key_bytes: int) -> Tuple[int, int]:
        """``(tile, scan_tile)`` of ``msd_reduce_runs_limits``: the geometry of :meth:`run_encode_limits`."""
        return self._limits("msd_reduce_runs_limits", 2, key_bytes, "key_bytes")

    def reduce_runs(self, keys, vals, op: str = "sum", positions=None, cap: Optional[int] = None):
        """One number per run of ``keys``: the ``"sum"``, ``"min"`` or ``"max"`` of the values of its elements.  The runs
        are those of :meth:`run_encode` on the same tensor (maximal stretches of equal BIT patterns; 4- or 8-byte
        elements), so run j here is run j there.  The value of element i is ``vals[i]``, or ``vals[positions[i]]`` with
        ``positions`` (int64, as :meth:`sort_rows` or :meth:`sort_typed` with rids produce them): the group-by case,
        where the keys were sorted and the value column stayed where it was.  ``vals`` is float32, int32, float64,
        int64, uint32 or uint64, whatever the keys are.  All tensors are 1-D and contiguous.

        Returns ``(num_runs, out)``.  ``num_runs`` is a one-element int64 tensor on the device: the true number of runs
        m, also when m > ``cap`` (default ``keys.numel()``).  ``out`` has ``cap`` elements, of which the first
        min(m, cap) are written.  A sum is int64 for integer values (uint64 for unsigned ones where torch has that
        dtype), exact modulo 2^64, and float64 for float values: summed in double, without atomics and in an order
        that the sizes and addresses alone fix, so the same call gives the same bits every time -- but not the bits of
        a sequential sum.  ``min`` / ``max`` have the values' dtype and are bit-exact, floats in IEEE-754 totalOrder
        as everywhere in this library: -0.0 is below +0.0, a NaN is the maximum of its run (the minimum, if its sign
        bit is set), unlike ``torch.amax`` / ``torch.amin``, which propagate any NaN.  Nothing waits on the host."""
        torch = _torch()
        code = _args.op_code(self.REDUCE_OPS, op)
        _args.flat("reduce_runs", keys, vals)
        ks = _args.elem_4_or_8("reduce_runs", keys, "4- or 8-byte keys")
        vt = self._key_type(vals)   # (a value dtype without an order is refused here)
        n = keys.numel()
        _args.same_length("keys and vals", keys, vals)
        _args.positions(positions, n)
        cap = _args.cap_or(cap, n)
        self._on_gpu(keys, vals, positions)
        num = _args.count_cell(keys.device)
        out = torch.empty(cap, dtype=_args.result_dtype(op, vals, vt), device=keys.device)
        self._ok(self._L.msd_reduce_runs(self._h, ptr(keys), ks, n, ptr(vals), vt, ptr(positions), code, cap, ptr(out), ptr(num)))
        return num, out

    def group_reduce(self, keys, vals, op: str = "sum"):
        """Group-by: ``(distinct_keys, aggregates)`` for UNSORTED 1-D ``keys`` of float32, int32, float64, int64, uint32
        or uint64 -- the distinct keys in the dtype's order (floats in totalOrder and told apart by their bits, as
        :meth:`unique`) and per distinct key the ``"sum"``, ``"min"`` or ``"max"`` of the ``vals`` of its elements, with
        the dtypes and the rules of :meth:`reduce_runs`.  The keys are sorted with positions, the value column is read
        through them where it lies.  ``keys`` and ``vals`` are not modified.  One host wait beyond the sort's own: the
        number of distinct keys sizes the results."""
        _args.op_code(self.REDUCE_OPS, op)
        self._key_type(keys)
        self._key_type(vals)
        _args.flat("group_reduce", keys, vals)
        _args.same_length("keys and vals", keys, vals)
        self._on_gpu(keys, vals)
        s, positions = self._sorted_with_positions(keys)
        _, distinct, _, _ = self.run_encode(s, starts=False)
        num, out = self.reduce_runs(s, vals, op=op, positions=positions)
        m = int(num.item())
        return distinct[:m], out[:m]

    # ---- scan-by-key over runs: window functions on sorted keys (include/msd_scan_hip.h)
    SCAN_OPS = {"sum": 0, "min": 1, "max": 2, "count": 3}   # MSD_SCAN_* of include/msd_scan_hip.h

    def scan_runs_limits(self, key_bytes: int) -> Tuple[int, int]:
        """``(tile, scan_tile)`` of ``msd_scan_runs_limits``: the geometry of :meth:`run_encode_limits`."""
        return self._limits("msd_scan_runs_limits", 2, key_bytes, "key_bytes")

    def scan_runs(self, keys, vals, op: str = "sum", exclusive: bool = False, positions=None, scatter: bool = False):
        """One number per ELEMENT of ``keys``: the running ``"sum"``, ``"min"``, ``"max"`` or ``"count"`` inside its run --
        ``OVER (PARTITION BY key ORDER BY the order of the elements)``.  The runs are those of :meth:`run_encode` and
        :meth:`reduce_runs` (maximal stretches of equal BIT patterns; 4- or 8-byte elements).  The value of element i is
        ``vals[i]``: the value column lies in the order of the keys (sorted along with them, or gathered with the
        positions a sort left: ``vals[positions]``).  ``positions`` and ``scatter`` are reserved for reading the values
        through positions and storing the results through them; they are NOT OFFERED YET and refused.  ``vals`` is float32, int32, float64, int64, uint32 or uint64, whatever the keys are, and may
        be ``None`` for ``"count"`` only, which counts 1 per element.  All tensors are 1-D and contiguous.

        Returns a tensor of ``keys.numel()`` elements: element i holds the op over its run's elements up to and
        including i, with ``exclusive`` up to the one in front of i and the op's identity at the first element of a
        run (0; for ``min`` the largest value of the dtype, for ``max`` the smallest: for floats the +NaN / -NaN with
        all payload bits set).  ``"count"``
        gives int64: the 1-based row number inside the run, 0-based with ``exclusive``.  A sum is int64 for integer
        values (uint64 for unsigned ones where torch has that dtype), exact modulo 2^64, and float64 for float values:
        every output is the sum of exactly its own prefix, summed in double without atomics and never formed by
        subtraction, in an order that the sizes and addresses alone fix, so the same call gives the same bits every
        time -- reproducible, but not the bits of a sequential sum or of ``torch.cumsum``.  ``min`` / ``max`` have the
        values' dtype and are bit-exact, floats in IEEE-754 totalOrder as everywhere in this library: -0.0 is below
        +0.0 and a NaN is an ordinary largest value (the smallest, if its sign bit is set), unlike ``torch.cummax`` /
        ``torch.cummin``, which propagate any NaN.  Nothing waits on the host.

        There is no convenience on UNSORTED keys: the library's sort is unstable, so the order of the elements inside a
        group -- and with it every running value but the last -- would be unspecified.  For a defined order sort a
        64-bit composite ``(key code << 32) | order column`` with positions, scan on the keys taken from its upper
        half and the values gathered through the positions; ``"count"`` alone may accept the arbitrary order."""
        torch = _torch()
        code = _args.op_code(self.SCAN_OPS, op)
        if vals is None and op != "count":
            raise MsdError(f"vals may be None for op 'count' only, not for {op!r}")
        _args.flat("scan_runs", keys, vals)
        ks = _args.elem_4_or_8("scan_runs", keys, "4- or 8-byte keys")
        vt = self._key_type(vals) if vals is not None else 0   # (a value dtype without an order is refused here)
        n = keys.numel()
        _args.same_length("keys and vals", keys, vals)
        _args.positions(positions, n)
        if scatter and positions is None:
            raise MsdError("scatter without positions")
        if positions is not None:
            raise MsdError("positions (and with them scatter) are not offered yet: gather the values, vals[positions], and scatter the result")
        self._on_gpu(keys, vals)
        out = torch.empty(n, dtype=_args.result_dtype(op, vals, vt), device=keys.device)
        self._ok(self._L.msd_scan_runs(self._h, ptr(keys), ks, n, ptr(vals if op != "count" else None), vt, ptr(None), code,
                                       1 if exclusive else 0, ptr(out)))   # (a count reads no values)
        return out

    # ---- stream compaction and stable partition: the filter (include/msd_compact_hip.h)
    COMPACT_RANGE, COMPACT_INVERT, COMPACT_REST = 1, 2, 4   # MSD_COMPACT_* of include/msd_compact_hip.h

    def compact_limits(self, key_bytes: int) -> Tuple[int, int]:
        """``(tile, scan_tile)`` of ``msd_compact_limits``: the geometry of :meth:`run_encode_limits`."""
        return self._limits("msd_compact_limits", 2, key_bytes, "key_bytes")

    def _bound_bits(self, keys, kt: int, bound, lowest: bool) -> int:
        """The bit pattern of a range bound in the keys' dtype; ``None`` is the key with the lowest / highest code."""
        width = 8 * keys.element_size()
        if bound is None:
            bits = C.c_uint64()
            self._L.msd_key_decode(kt, 0 if lowest else (1 << width) - 1, C.byref(bits))
            return int(bits.value)
        nt = {self.KEY_U32: np.uint32, self.KEY_I32: np.int32, self.KEY_F32: np.float32, self.KEY_U64: np.uint64, self.KEY_I64: np.int64,
              self.KEY_F64: np.float64}[kt]
        is_float = kt in (self.KEY_F32, self.KEY_F64)
        try:
            if not is_float and (int(bound) != bound or not np.iinfo(nt).min <= int(bound) <= np.iinfo(nt).max):
                raise ValueError("not an integer of that range")
            with np.errstate(over="ignore"):
                a = np.array([float(bound) if is_float else int(bound)], dtype=nt)
        except (OverflowError, ValueError, TypeError) as e:
            raise MsdError(f"the bound {bound!r} is not a value of {keys.dtype}: {e}")
        return int(a.view(np.uint32 if width == 32 else np.uint64)[0])

    def compact(self, keys=None, mask=None, lo=None, hi=None, invert: bool = False, rest: bool = False, values=None, indices: bool = False,
                cap: Optional[int] = None, out=None, out_values=None, out_indices=None):
        """The filter: the elements that a predicate keeps, in their original order (the call is stable) -- ``x[mask]``,
        ``torch.masked_select``, ``torch.nonzero``, a ``WHERE lo <= key AND key <= hi``.  Element i is kept if
        ``mask[i] != 0`` (where a ``mask`` is given: any one-byte dtype, ``torch.bool`` included) AND ``lo <= keys[i] <= hi``
        (where ``lo`` or ``hi`` is given: Python numbers, converted to the keys' dtype, both inclusive, ``None`` the lowest
        / highest key of the dtype); ``invert`` keeps exactly the others.  With neither a mask nor a bound everything is
        kept.  ``keys`` is float32, int32, float64, int64, uint32 or uint64 and may be ``None`` for the mask-only form;
        ``values`` is a column of 4- or 8-byte elements of any dtype, as long as the keys or the mask.  All tensors are
        1-D and contiguous, and they are not modified.

        The range is tested in the key order of this library: floats in IEEE-754 totalOrder on their bits.  -0.0 is below
        +0.0, so ``lo=0.0`` drops the -0.0s that ``keys >= 0`` keeps in torch; a NaN is an ordinary key above +inf (below
        -inf with the sign bit set), so ``hi=None`` keeps the +NaNs and ``hi=float("inf")`` does not, where every torch
        comparison with a NaN is false.  ``lo > hi`` keeps nothing.

        Returns ``(out_keys, out_values, out_indices, count)``; an output that was not asked for is ``None``: the kept keys
        (whenever ``keys`` is given; bit-exact), the kept values (with ``values``) and the int64 positions of the kept
        elements (with ``indices`` or ``out_indices``).  ``count`` is a one-element int64 tensor on the device: the true
        number m of kept elements, also when m > ``cap`` (default: the number of elements).  The outputs are allocated at
        ``cap`` elements, or are ``out`` / ``out_values`` / ``out_indices`` of at least that many; their first
        min(m, cap) elements are written and nothing else.  With ``rest`` (a stable partitioning into kept and rejected)
        the outputs hold all elements: the kept ones, then the rejected ones in their original order, ``count`` being the
        split point and ``out_indices`` a permutation that :meth:`run_encode` and :meth:`reduce_runs` take as
        ``positions``; ``cap`` must then be at least the number of elements.  Nothing waits on the host."""
        torch = _torch()
        if keys is None and mask is None:
            raise MsdError("compact needs keys or a mask")
        first = keys if keys is not None else mask
        _args.flat("compact", keys, mask, values)
        n = first.numel()
        _args.same_length("keys, mask and values", keys, mask, values)
        kt = self._key_type(keys) if keys is not None else 0   # (a dtype without a key order is refused here)
        if mask is not None and mask.element_size() != 1:
            raise MsdError(f"the mask has a one-byte dtype (torch.bool, uint8, int8), not {mask.dtype}")
        if values is not None:
            _args.elem_4_or_8("compact", values, "values of 4- or 8-byte elements")
        want_range = lo is not None or hi is not None
        if want_range and keys is None:
            raise MsdError("lo / hi without keys")
        if (out is not None and keys is None) or (out_values is not None and values is None):
            raise MsdError("out without keys, or out_values without values")
        cap = _args.cap_or(cap, n)
        if rest and cap < n:
            raise MsdError("rest needs cap >= the number of elements")
        want_idx = bool(indices) or out_indices is not None
        # (the outputs: name, the tensor given, its dtype -- None: not asked for --, and what refuses a given one)
        like = "must be a contiguous 1-D tensor of the input's dtype with at least cap elements"
        outs = [("out", out, keys.dtype if keys is not None else None, like),
                ("out_values", out_values, values.dtype if values is not None else None, like),
                ("out_indices", out_indices, torch.int64 if want_idx else None, "must be a contiguous 1-D int64 tensor with at least cap elements")]
        for name, t, dt, must in outs:
            _args.output(t, dt, (cap,), name + " " + must, at_least=True)
        self._on_gpu(keys, mask, values, out, out_values, out_indices)
        lo_bits = self._bound_bits(keys, kt, lo, True) if want_range else 0
        hi_bits = self._bound_bits(keys, kt, hi, False) if want_range else 0
        out, out_values, out_indices = [_args.output(t, dt, (cap,), None, first.device) for _, t, dt, _ in outs]
        count = _args.count_cell(first.device)
        flags = (self.COMPACT_RANGE if want_range and n else 0) | (self.COMPACT_INVERT if invert else 0) | (self.COMPACT_REST if rest else 0)
        mask8 = mask.view(torch.uint8) if mask is not None else None
        # (nothing to filter: only the count is written, and an empty tensor has no address to hand over)
        kp, mp, vp, okp, ovp, oip = [ptr(t if n else None) for t in (keys, mask8, values, out, out_values, out_indices)]
        self._ok(self._L.msd_compact(self._h, kp, kt, n, mp, lo_bits, hi_bits, flags, vp, values.element_size() if values is not None else 0, cap,
                                     okp, ovp, oip, ptr(count)))
        return out, out_values, out_indices, count

    def masked_select(self, t, mask):
        """``torch.masked_select(t, mask)`` for contiguous tensors of one shape: the elements of ``t`` (float32, int32,
        float64, int64, uint32 or uint64; bit-exact) where ``mask`` (a one-byte dtype) is non-zero, 1-D, in their order.
        :meth:`compact` and ONE host wait: the count sizes the result."""
        if tuple(t.shape) != tuple(mask.shape) or not t.is_contiguous() or not mask.is_contiguous():
            raise MsdError("masked_select takes contiguous tensors of one shape")
        out, _, _, count = self.compact(t.reshape(-1), mask=mask.reshape(-1))
        return out[:int(count.item())]

    def nonzero(self, mask):
        """``torch.nonzero(mask).flatten()`` for a 1-D contiguous ``mask`` of a one-byte dtype: the int64 positions of its
        non-zero bytes, ascending.  :meth:`compact` in its mask-only form and ONE host wait: the count sizes the result."""
        _, _, idx, count = self.compact(mask=mask, indices=True)
        return idx[:int(count.item())]

    def filter_range(self, keys, lo, hi, values=None):
        """The keys with ``lo <= key <= hi`` in their order -- and, with ``values``, ``(keys, values)``: the rows of the
        value column beside them.  The range is tested as in :meth:`compact` (floats in totalOrder: -0.0 is below +0.0, a
        NaN is an ordinary key), so it equals ``keys[(keys >= lo) & (keys <= hi)]`` on data without NaNs and negative
        zeros.  :meth:`compact` and ONE host wait: the count sizes the result."""
        if lo is None and hi is None:
            raise MsdError("filter_range takes a bound")
        out, out_values, _, count = self.compact(keys, lo=lo, hi=hi, values=values)
        m = int(count.item())
        return out[:m] if values is None else (out[:m], out_values[:m])

    # ---- sorted search (include/msd_search_hip.h)
    def search_sorted_limits(self, key_bytes: int) -> Tuple[int, int]:
        """``(tile, direct_tile)`` of ``msd_search_sorted_limits``: the elements (keys plus needles together) one
        workgroup of the merge path takes for that key width, and the needles one workgroup of the direct path takes."""
        return self._limits("msd_search_sorted_limits", 2, key_bytes, "key_bytes")

    def searchsorted(self, sorted_keys, needles, right: bool = False, needles_sorted: bool = False, sort_needles: bool = False,
                     positions=None, out=None):
        """``torch.searchsorted(sorted_keys, needles, right=right)`` in the key order of this library: for every needle
        the number of keys that are smaller (``right``: not larger), an int64 tensor of the needles' shape.
        ``sorted_keys`` is 1-D and contiguous, of float32, int32, float64, int64, uint32 or uint64, and ascending as
        :meth:`sort_typed` leaves it (trusted); ``needles`` is contiguous, of any shape and the same dtype.

        Where the results differ from ``torch.searchsorted``: floats are ordered by IEEE-754 totalOrder on their bits,
        as everywhere in this library.  -0.0 lies below +0.0, so the left bound of +0.0 points behind the -0.0s; a NaN
        is an ordinary key, a +NaN above +inf, a -NaN (sign bit set) below -inf, among NaNs by payload.  A tensor sorted
        by ``torch.sort`` is in this order only if it holds no -NaN and no zeros of both signs.

        ``needles_sorted=True`` promises needles that are ascending in the same order (flat): the library may then
        merge the two arrays, reading each once, instead of one binary search per needle (``set_option("search_mode",
        ...)``).  ``positions`` (int64, 1-D, a permutation of the needles' flat indices) stores the result of needle j
        at flat index ``positions[j]``.  ``sort_needles=True`` does both for unsorted needles: it sorts a copy of them
        with positions (:meth:`sort_rows` for 32-bit keys, :meth:`sort_typed` with rids for 64-bit keys) and searches
        through those, without one random load into ``sorted_keys``.  Measured on 2^30 sorted keys (DESIGN.md section
        10.7) that is 2 to 4 times faster than the default from 2^24 needles on (89.9 against 332 ms at 2^30 needles) and
        slower at 2^20 needles and fewer (0.51 against 0.45 ms), so the default stays ``False``.  ``out`` (int64, contiguous, the
        needles' shape) receives the result.  ``sorted_keys`` and ``needles`` are not modified.  Nothing waits on the
        host."""
        torch = _torch()
        kt = self._key_type(sorted_keys)
        _args.same_dtype(sorted_keys, needles, "sorted_keys and needles")
        _args.one_dim("searchsorted", sorted_keys, what="sorted_keys")
        _args.contiguous("searchsorted", sorted_keys, needles)
        m = needles.numel()
        _args.positions(positions, m, "needles")
        if positions is not None and sort_needles:
            raise MsdError("positions together with sort_needles: the sort makes positions of its own")
        shape = tuple(needles.shape)
        _args.output(out, torch.int64, shape, "out must be a contiguous int64 tensor of shape {shape}")
        self._on_gpu(sorted_keys, needles, positions, out)
        out = _args.output(out, torch.int64, shape, None, needles.device)
        if m == 0:
            return out
        if sort_needles:
            needles, positions = self._sorted_with_positions(needles.reshape(-1))
            needles_sorted = True
        self._ok(self._L.msd_search_sorted(self._h, ptr(sorted_keys), kt, sorted_keys.numel(), ptr(needles), m,
                                           1 if needles_sorted else 0, 1 if right else 0, ptr(positions), ptr(out)))
        return out

    def bucketize(self, values, boundaries, right: bool = False):
        """``torch.bucketize(values, boundaries, right=right)``: :meth:`searchsorted` ``(boundaries, values, right=right)``,
        with its order -- where results differ from torch: -0.0 lies below +0.0 and a NaN is an ordinary key (+NaN above
        +inf, -NaN below -inf).  ``boundaries`` is 1-D, contiguous and ascending as :meth:`sort_typed` leaves it."""
        return self.searchsorted(boundaries, values, right=right)

    # ---- merge of two sorted arrays (include/msd_merge_hip.h)
    def merge_sorted_limits(self, key_bytes: int) -> int:
        """``tile`` of ``msd_merge_sorted_limits``: the elements (of both inputs together) one workgroup takes for that
        key width."""
        return self._limits("msd_merge_sorted_limits", 1, key_bytes, "key_bytes")

    def merge_sorted(self, a, b, values_a=None, values_b=None, origin: bool = False, out=None, out_values=None, out_origin=None):
        """The merge of two sorted tensors: ``a`` and ``b`` are 1-D, contiguous, of the same dtype (float32, int32,
        float64, int64, uint32 or uint64) and each ascending as :meth:`sort_typed` leaves it (trusted); the result holds
        the ``a.numel() + b.numel()`` keys in ascending order -- what sorting ``torch.cat([a, b])`` gives, but each input
        is read once and nothing is sorted again.

        The merge is stable: among equal keys all of A's come before all of B's, and within one side equal keys keep
        their order.  The keys are bit-exact.  Floats are ordered by IEEE-754 totalOrder on their bits, as everywhere in
        this library: -0.0 lies below +0.0 and the two stay apart, a NaN is an ordinary key (+NaN above +inf, -NaN below
        -inf) and keeps its payload.

        ``values_a`` and ``values_b`` (both or neither; 1-D, contiguous, 8-byte elements of one dtype -- int64, uint64 or
        float64 --, as long as their keys) travel with their keys.  ``origin=True`` (or ``out_origin``) also gives, per position of the result, the
        index in ``torch.cat([a, b])`` of the element that landed there (int64): the stable argsort of the
        concatenation, which :meth:`reduce_runs` takes as ``positions``.  Returns ``merged``, or the tuple
        ``(merged[, values][, origin])`` in that order.  ``out``, ``out_values`` and ``out_origin`` (contiguous, shape
        ``(n + m,)``, the dtype of the keys, of the values, int64) receive the results and must not overlap an input:
        the merge is not in place.  The inputs are not modified.  Nothing waits on the host."""
        torch = _torch()
        kt = _args.sorted_pair("merge_sorted", a, b, contiguous_too=False)   # (all four inputs below)
        if (values_a is None) != (values_b is None):
            raise MsdError("values_a and values_b are given both or neither")
        if values_a is not None:
            _args.one_dim("merge_sorted", values_a, values_b)
            if values_a.dtype != values_b.dtype or values_a.dtype not in [torch.int64, torch.float64] + ([torch.uint64] if hasattr(torch, "uint64") else []):
                raise MsdError(f"the values must have 8-byte elements of one dtype (int64, uint64 or float64), not {values_a.dtype} and {values_b.dtype}")
            if values_a.numel() != a.numel() or values_b.numel() != b.numel():
                raise MsdError("the values must be as long as their keys")
        elif out_values is not None:
            raise MsdError("out_values without values_a and values_b")
        _args.contiguous("merge_sorted", a, b, values_a, values_b)
        n, m = a.numel(), b.numel()
        want_origin = origin or out_origin is not None
        # (the outputs: name, the tensor given, its dtype -- None: not asked for)
        wanted = [("out", out, a.dtype), ("out_values", out_values, values_a.dtype if values_a is not None else None),
                  ("out_origin", out_origin, torch.int64 if want_origin else None)]
        for name, t, dt in wanted:
            _args.output(t, dt, (n + m,), name + " must be a contiguous {dtype} tensor of shape {shape}")
        self._on_gpu(a, b, values_a, values_b, out, out_values, out_origin)
        res = [_args.output(t, dt, (n + m,), None, a.device) for _, t, dt in wanted]
        self._ok(self._L.msd_merge_sorted(self._h, ptr(a), n, ptr(b), m, kt, ptr(values_a), ptr(values_b),
                                          *[ptr(t) for t in res]))
        res = [t for t in res if t is not None]
        return res[0] if len(res) == 1 else tuple(res)

    # ---- set operations on two sorted arrays (include/msd_setops_hip.h)
    SET_OPS = {"intersection": 0, "union": 1, "difference": 2, "symmetric_difference": 3}   # MSD_SET_* of include/msd_setops_hip.h

    def set_sorted_limits(self, key_bytes: int) -> Tuple[int, int]:
        """``(tile, scan_tile)`` of ``msd_set_sorted_limits``: the elements (of both inputs together) one workgroup takes
        for that key width, and how many tile counts one workgroup of the tile-count scan takes at once."""
        return self._limits("msd_set_sorted_limits", 2, key_bytes, "key_bytes")

    @staticmethod
    def _set_bound(op: str, n: int, m: int) -> int:
        """the most results ``op`` can have on inputs of n and m elements"""
        return min(n, m) if op == "intersection" else n if op == "difference" else n + m

    def set_sorted(self, a, b, op: str, origin: bool = False, cap: Optional[int] = None, out=None, out_origin=None):
        """A set operation on two sorted tensors: ``a`` and ``b`` are 1-D, contiguous, of the same dtype (float32, int32,
        float64, int64, uint32 or uint64) and each ascending as :meth:`sort_typed` leaves it (trusted; duplicates are
        allowed).  ``op`` is ``"intersection"`` (the values in both), ``"union"`` (in either), ``"difference"`` (in
        ``a`` and not in ``b``) or ``"symmetric_difference"`` (in exactly one).  The result is a set: every value once,
        ascending, bit-exact -- ``np.intersect1d`` / ``union1d`` / ``setdiff1d`` / ``setxor1d`` on sorted inputs, without
        sorting or concatenating anything.

        Values are told apart by their BITS and floats ordered by IEEE-754 totalOrder, as everywhere in this library:
        -0.0 and +0.0 are two values (-0.0 below +0.0), so with -0.0 only in ``b`` and +0.0 only in ``a`` both are in the
        union and neither is in the intersection; NaNs with equal bits are one value and intersect, NaNs of different
        sign or payload do not.  numpy and torch compare floats by value: they merge the zeros and keep every NaN apart.

        Returns ``(num, out)`` or, with ``origin=True`` (or ``out_origin``), ``(num, out, origin)``.  ``num`` is a
        one-element int64 tensor on the device: the true number of results, also when it exceeds ``cap``.  ``out`` has
        ``cap`` elements (default: the most the operation can give -- min(n, m), n + m, n, n + m in the order above), of
        which the first min(num, cap) are written.  ``origin`` (int64, ``cap`` elements) names, per result, the index in
        ``torch.cat([a, b])`` of the first occurrence of that value; a value that both sides hold is taken from ``a``.
        ``out`` and ``out_origin`` (contiguous, shape ``(cap,)``) receive the results and must not overlap an input.
        The inputs are not modified.  Nothing waits on the host."""
        torch = _torch()
        kt = _args.sorted_pair("set_sorted", a, b)
        code = _args.op_code(self.SET_OPS, op)
        n, m = a.numel(), b.numel()
        cap = _args.cap_or(cap, self._set_bound(op, n, m))
        want_origin = origin or out_origin is not None
        wanted = [("out", out, a.dtype)] + ([("out_origin", out_origin, torch.int64)] if want_origin else [])
        for name, t, dt in wanted:
            _args.output(t, dt, (cap,), name + " must be a contiguous {dtype} tensor of shape {shape}")
        self._on_gpu(a, b, out, out_origin)
        num = _args.count_cell(a.device)
        res = [_args.output(t, dt, (cap,), None, a.device) for _, t, dt in wanted]
        self._ok(self._L.msd_set_sorted(self._h, code, ptr(a), n, ptr(b), m, kt, cap, ptr(res[0]),
                                        ptr(res[1] if want_origin else None), ptr(num)))
        return (num, *res)

    def _set1d(self, a, b, op: str, name: str):
        _args.sorted_pair(name, a, b, contiguous_too=False)   # (the copies are contiguous)
        self._on_gpu(a, b)
        sa, sb = a.clone(), b.clone()   # (contiguous copies)
        self.sort_typed(sa)
        self.sort_typed(sb)
        num, out = self.set_sorted(sa, sb, op)
        return out[:int(num.item())]

    def intersect1d(self, a, b):
        """``np.intersect1d(a, b)`` for UNSORTED 1-D tensors of one dtype (float32, int32, float64, int64, uint32 or
        uint64): the distinct values that both hold, in the dtype's order.  Copies of both are sorted
        (:meth:`sort_typed`) and handed to :meth:`set_sorted`; the inputs are not modified.  Floats are told apart by
        their BITS and ordered by totalOrder: where numpy says -0.0 == +0.0 and NaN != NaN, here -0.0 and +0.0 do not
        intersect and NaNs with equal bits do.  One host wait beyond the sorts' own: the count sizes the result."""
        return self._set1d(a, b, "intersection", "intersect1d")

    def union1d(self, a, b):
        """``np.union1d(a, b)`` for UNSORTED 1-D tensors, as :meth:`intersect1d`: the distinct values of both.  Floats by
        their BITS: -0.0 and +0.0 are both in the result (-0.0 first) where numpy keeps one zero, and NaNs with equal
        bits are one value, -NaNs in front of -inf and +NaNs behind +inf, where numpy collapses all NaNs into one at the end."""
        return self._set1d(a, b, "union", "union1d")

    def setdiff1d(self, a, b):
        """``np.setdiff1d(a, b)`` for UNSORTED 1-D tensors, as :meth:`intersect1d`: the distinct values of ``a`` that
        ``b`` does not hold.  Floats by their BITS: +0.0 in ``a`` survives a -0.0 in ``b`` where numpy removes it, and
        a NaN in ``a`` is removed by a NaN with the same bits in ``b`` where numpy keeps it."""
        return self._set1d(a, b, "difference", "setdiff1d")

    def setxor1d(self, a, b):
        """``np.setxor1d(a, b)`` for UNSORTED 1-D tensors, as :meth:`intersect1d`: the distinct values that exactly one
        of the two holds.  Floats by their BITS: -0.0 in one and +0.0 in the other are both in the result where numpy
        drops both, and NaNs with equal bits on both sides cancel where numpy keeps them."""
        return self._set1d(a, b, "symmetric_difference", "setxor1d")

    # ---- sort-merge join of two sorted arrays (include/msd_join_hip.h)
    def join_limits(self, key_bytes: int) -> Tuple[int, int, int]:
        """``(tile, scan_tile, pair_tile)`` of ``msd_join_limits``: the elements (of both inputs together) one workgroup
        of the groups call takes for that key width, the counts one workgroup of a scan takes, and the pair ranks one
        workgroup of the expansion takes."""
        return self._limits("msd_join_limits", 3, key_bytes, "key_bytes")

    def join_groups(self, a, b, cap: Optional[int] = None, keys: bool = True):
        """The matched groups of two sorted tensors: ``a`` and ``b`` are 1-D, contiguous, of the same dtype (float32,
        int32, float64, int64, uint32 or uint64) and each ascending as :meth:`sort_typed` leaves it (trusted; duplicates
        are allowed).  For every value that both hold, ascending: the key (bit-exact), the index of its first occurrence
        in ``a`` and the length of its run there, and the same for ``b`` -- the sort-merge join in CSR form: group g
        stands for ``a_count[g] * b_count[g]`` pairs, which :meth:`join_pairs` expands.

        Values are told apart by their BITS and floats ordered by IEEE-754 totalOrder, as everywhere in this library:
        -0.0 and +0.0 do not join, NaNs with equal bits do.  ``keys`` and ``a_first`` are what
        :meth:`set_sorted` ``(a, b, "intersection", origin=True)`` gives.

        Returns ``(num_groups, keys, a_first, a_count, b_first, b_count)``: ``num_groups`` is a one-element int64
        tensor on the device, the true number of groups also when it exceeds ``cap``; the five arrays have ``cap``
        elements (default: min(n, m), which holds every group), of which the first min(num_groups, cap) are written;
        ``keys`` has the inputs' dtype (``None`` with ``keys=False``), the others are int64.  The inputs are not
        modified.  Nothing waits on the host."""
        torch = _torch()
        kt = _args.sorted_pair("join_groups", a, b)
        n, m = a.numel(), b.numel()
        cap = _args.cap_or(cap, min(n, m))
        self._on_gpu(a, b)
        num = _args.count_cell(a.device)
        k = torch.empty(cap, dtype=a.dtype, device=a.device) if keys else None
        four = [torch.empty(cap, dtype=torch.int64, device=a.device) for _ in range(4)]
        self._ok(self._L.msd_join_groups(self._h, ptr(a), n, ptr(b), m, kt, cap, ptr(k), *[ptr(t) for t in four],
                                         ptr(num)))
        return (num, k, *four)

    def join_pairs(self, groups, n: int, m: int, cap: int, positions_a=None, positions_b=None, out_a=None, out_b=None):
        """The index pairs of matched groups: ``groups`` is what :meth:`join_groups` returned (the keys are not looked
        at), ``n`` and ``m`` the lengths of its inputs.  Pair r, in lexicographic order of (index in ``a``, index in
        ``b``), lies in the group g that the running sum of ``a_count * b_count`` puts it in, at local rank t:
        ``ia = a_first[g] + t // b_count[g]``, ``ib = b_first[g] + t % b_count[g]``.  If the groups were truncated by
        their ``cap``, the pairs are those of the stored groups.

        Returns ``(num_pairs, ia, ib)``: ``num_pairs`` is a one-element int64 tensor on the device, the true total also
        when it exceeds ``cap``; ``ia`` and ``ib`` (int64, ``cap`` elements; ``out_a`` / ``out_b`` where given) hold the
        first min(num_pairs, cap) pairs.  ``cap=0`` only counts.  ``positions_a`` (int64, ``n`` elements) stores
        ``positions_a[ia]`` in place of ``ia``, ``positions_b`` likewise: the positions of a sort with positions, so
        that the pairs index the unsorted tensors.  Nothing waits on the host."""
        torch = _torch()
        num_groups, _, a_first, a_count, b_first, b_count = groups
        n, m, cap = int(n), int(m), int(cap)
        _args.non_negative("n, m and cap", n, m, cap)
        four = (a_first, a_count, b_first, b_count)
        gcap = a_first.numel()
        if num_groups.dtype != torch.int64 or num_groups.numel() != 1:
            raise MsdError("num_groups must be a one-element int64 tensor")
        if any(t.dtype != torch.int64 or t.dim() != 1 or t.numel() != gcap or not t.is_contiguous() for t in four):
            raise MsdError("the groups must be contiguous 1-D int64 tensors of one length")
        _args.positions(positions_a, n, name="positions_a")
        _args.positions(positions_b, m, name="positions_b")
        for name, t in (("out_a", out_a), ("out_b", out_b)):
            _args.output(t, torch.int64, (cap,), name + " must be a contiguous int64 tensor of shape {shape}")
        self._on_gpu(num_groups, *four, positions_a, positions_b, out_a, out_b)
        dev = num_groups.device
        num = _args.count_cell(dev)
        ia = _args.output(out_a, torch.int64, (cap,), None, dev)
        ib = _args.output(out_b, torch.int64, (cap,), None, dev)
        self._ok(self._L.msd_join_pairs(self._h, gcap, ptr(num_groups), ptr(a_first), ptr(a_count), ptr(b_first), ptr(b_count), n, m, ptr(positions_a),
                                        ptr(positions_b), cap, ptr(ia), ptr(ib), ptr(num)))
        return num, ia, ib

    def join(self, a, b):
        """The inner equi-join of two UNSORTED 1-D tensors of one dtype (float32, int32, float64, int64, uint32 or
        uint64): ``(ia, ib)``, int64 indices into ``a`` and ``b`` with ``a[ia[r]]`` bit-equal to ``b[ib[r]]``, every such
        pair exactly once.  The order is that of :meth:`join_pairs` on the sorted copies: ascending by key, and within
        a key by the place in the sorted copy of ``a``, then of ``b``.  Values are told apart by their BITS: -0.0 and
        +0.0 do not join, NaNs with equal bits do.  Both inputs are sorted with positions (copies; the inputs are not
        modified), :meth:`join_groups` finds the groups and :meth:`join_pairs` expands them through both position
        arrays.  One host wait beyond the sorts' own: the number of pairs sizes the result."""
        _args.sorted_pair("join", a, b, contiguous_too=False)   # (the sorts take contiguous copies)
        self._on_gpu(a, b)
        n, m = a.numel(), b.numel()
        if n == 0 or m == 0:
            none = _torch().empty(0, dtype=_torch().int64, device=a.device)
            return none, none.clone()
        sa, pa = self._sorted_with_positions(a.contiguous())
        sb, pb = self._sorted_with_positions(b.contiguous())
        groups = self.join_groups(sa, sb, keys=False)
        total, _, _ = self.join_pairs(groups, n, m, 0)
        _, ia, ib = self.join_pairs(groups, n, m, int(total.item()), positions_a=pa, positions_b=pb)
        return ia, ib

    # ---- synthetic inputs
    def gen_uniform_u32(self, keys, seed: int = 0x5EED0001, first: int = 0) -> None:
        self._ok(self._L.msd_gen_uniform_u32(self._h, self._ptr(keys, 4), keys.numel(), seed, first))

    def gen_uniform_u64(self, keys, seed: int = 0x5EED0005, first: int = 0, shift_right: int = 0) -> None:
        self._ok(self._L.msd_gen_uniform_u64(self._h, self._ptr(keys, 8), keys.numel(), seed, first, shift_right))

    def gen_zipf_u32(self, keys, seed: int = 0x5EED0003, first: int = 0) -> None:
        self._ok(self._L.msd_gen_zipf_u32(self._h, self._ptr(keys, 4), keys.numel(), seed, first))

    def gen_dup_u32(self, keys, distinct: int, seed: int = 0x5EED0009, first: int = 0) -> None:
        self._ok(self._L.msd_gen_dup_u32(self._h, self._ptr(keys, 4), keys.numel(), seed, first, distinct))

    def gen_mt19937_64(self, keys, seed: int, shift_right: int = 0) -> None:
        """The reference's own RNG stream (src/rand.c:47-86) into an int64 tensor."""
        self._ok(self._L.msd_gen_mt19937_64(self._h, self._ptr(keys, 8), keys.numel(), seed, shift_right))

    def gen_iota_u64(self, vals, first: int = 0) -> None:
        self._ok(self._L.msd_gen_iota_u64(self._h, self._ptr(vals, 8), vals.numel(), first))

    def set_option(self, name: str, value: int) -> None:
        """Tuning knob of include/msd_radix_hip.h (``direct_mode``, ``direct_min``, ``select_cap``, ``topk_rows_mode``, ...) or
        of include/msd_sort_rows_hip.h: ``sort_rows_mode`` (0 the library chooses, 1 always the segment path, 2 always the
        row kernel) and ``sort_rows_lanes`` (0 by the shape of the matrix, 64 / 256 / 1024 forced where the row fits); of
        include/msd_search_hip.h: ``search_mode`` (sorted needles: 0 the library chooses, 1 always the direct path, 2 always
        the merge path) and ``search_merge_ratio`` (R >= 1: the library chooses the merge path when m >= n / R)."""
        self._ok(self._L.msd_set_option(self._h, name.encode(), int(value)))

    # ---- phase report
    def set_profiling(self, on: bool) -> None:
        self._ok(self._L.msd_set_profiling(self._h, int(on)))

    def phases(self) -> List[Tuple[str, float]]:
        n = self._L.msd_phase_count(self._h)
        return [(self._L.msd_phase_name(self._h, i).decode(), float(self._L.msd_phase_us(self._h, i))) for i in range(n)]

    def stats(self) -> Dict[str, int]:
        """The counters of the last call that msd_stat knows by now (:data:`STAT_NAMES`)."""
        out = {}
        for name in STAT_NAMES:
            v = C.c_uint64()
            if self._L.msd_stat(self._h, name.encode(), C.byref(v)) == 0:
                out[name] = int(v.value)
        return out


class MsdShard:
    """One rank of a sharded sort behind the C ABI (include/msd_sharded_hip.h): RCCL is called from C, no
    torch.distributed on the data path.  ``nccl_comm``: the address of the caller's ncclComm_t -- e.g.
    :func:`torch_nccl_comm` for the process group torch.distributed has set up -- or None for a single rank."""

    def __init__(self, ctx: MsdContext, nccl_comm: Optional[int] = None):
        self._L = _lib.load_rccl()
        self.ctx = ctx
        h = C.c_void_p()
        rc = self._L.msd_shard_create(C.byref(h), ctx._h, C.c_void_p(nccl_comm or 0))
        if rc != 0 or not h:
            raise MsdError(f"msd_shard_create failed with {rc}")
        self._h = h
        self.rank = int(self._L.msd_shard_rank(h))
        self.world = int(self._L.msd_shard_world(h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.msd_shard_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ok(self, rc: int) -> None:
        if rc == -5:
            from .dist import ReceiveOverflow
            raise ReceiveOverflow(self._L.msd_shard_last_error(self._h).decode())
        if rc != 0:
            raise MsdError(f"error {rc}: {self._L.msd_shard_last_error(self._h).decode()}")

    def set_option(self, name: str, value: int) -> None:
        self._ok(self._L.msd_shard_set_option(self._h, name.encode(), int(value)))

    def sort_u32(self, keys, recv, work=None, scheme: Optional[str] = None):
        """``msd_sort_u32_sharded``: returns this rank's sorted key range -- a view of ``work`` (fine scheme), ``recv``
        (coarse) or ``keys`` (single rank)."""
        p = self.ctx._ptr
        out, n_out = C.c_void_p(), C.c_uint64()
        sc = {None: 0, "fine": 1, "coarse": 2}[scheme]
        self._ok(self._L.msd_sort_u32_sharded(self._h, p(keys, 4), keys.numel(), p(recv, 4) if recv is not None else None,
                                              recv.numel() if recv is not None else 0, p(work, 4) if work is not None else None,
                                              work.numel() if work is not None else 0, sc, C.byref(out), C.byref(n_out)))
        for t in (work, recv, keys):
            if t is not None and t.data_ptr() == out.value:
                return t[:n_out.value]
        raise MsdError("msd_sort_u32_sharded returned an unknown buffer")

    def sort_pairs_u64(self, keys, rids, recv_keys, recv_rids):
        p = self.ctx._ptr
        ok_, or_, n_out = C.c_void_p(), C.c_void_p(), C.c_uint64()
        cap = min(recv_keys.numel(), recv_rids.numel()) if recv_keys is not None else 0
        self._ok(self._L.msd_sort_pairs_u64_sharded(self._h, p(keys, 8), p(rids, 8), keys.numel(),
                                                    p(recv_keys, 8) if recv_keys is not None else None,
                                                    p(recv_rids, 8) if recv_rids is not None else None, cap,
                                                    C.byref(ok_), C.byref(or_), C.byref(n_out)))
        if ok_.value == keys.data_ptr():
            return keys[:n_out.value], rids[:n_out.value]
        return recv_keys[:n_out.value], recv_rids[:n_out.value]


def torch_nccl_comm(device: int) -> int:
    """Address of the ncclComm_t (RCCL) behind torch.distributed's default process group on ``device`` (backend "nccl";
    the communicator exists once a collective has run on it)."""
    import torch
    import torch.distributed as dist
    pg = dist.distributed_c10d._get_default_group()
    be = pg._get_backend(torch.device("cuda", device))
    return int(be._comm_ptr())


def plan_first_round(n: int, key_bytes: int = 4, val_bytes: int = 0, end_bit: Optional[int] = None,
                     compute_units: int = 256) -> Dict[str, int]:
    """Host-only pass planner (the counterpart of the reference's schedule_passes,
    src/msb_64.c:1334-1400); needs no GPU."""
    L = _lib.load()
    p = _lib.MsdPlan()
    rc = L.msd_plan_first_round(n, key_bytes, val_bytes, key_bytes * 8 if end_bit is None else end_bit,
                                compute_units, C.byref(p))
    if rc != 0:
        raise MsdError(f"msd_plan_first_round failed with {rc}")
    return {f: int(getattr(p, f)) for f, _ in p._fields_}


# ---------------------------------------------------------------------------
# the reference's own surface, on host numpy arrays
# ---------------------------------------------------------------------------

_u64p = C.POINTER(C.c_uint64)


def mamalloc(n_bytes: int) -> np.ndarray:
    """64-byte aligned host buffer, as the reference's mamalloc (src/msb_64.c:111-115)."""
    L = _lib.load()
    p = L.mamalloc(n_bytes)
    if not p:
        raise MemoryError(n_bytes)
    buf = (C.c_uint8 * n_bytes).from_address(p)
    arr = np.frombuffer(buf, dtype=np.uint8)
    return arr  # freed by the C library's allocator only at process exit (tests use small sizes)


def sort(keys: Sequence[np.ndarray], rids: Sequence[np.ndarray], size: Sequence[int], threads: int = 64,
         numa: Optional[int] = None, fudge: float = 1.0):
    """``sort(keys, rids, size, threads, numa, fudge, description, times)`` of
    include/msb_64.h:37-39 on lists of uint64 numpy arrays (sorted in place).
    Returns (description, times) as the reference fills them."""
    L = _lib.load()
    numa = len(keys) if numa is None else numa
    for a in list(keys) + list(rids):
        if a.dtype != np.uint64 or not a.flags.c_contiguous:
            raise MsdError("arrays must be contiguous uint64")
    # size[] is REWRITTEN by the call (the reference does the same, src/msb_64.c:2180): it must be writable ...
    if isinstance(size, tuple) or (isinstance(size, np.ndarray) and not size.flags.writeable):
        raise MsdError("size must be a mutable sequence: sort() rewrites it")
    # ... and with fudge > 1 an array may come back with up to size[a] * fudge tuples (the capacity the reference
    # requires of the caller, :1574-1578): the arrays must have that room
    for a in range(numa):
        cap = int(float(size[a]) * fudge) if fudge > 1.0 else int(size[a])
        if keys[a].size < cap or rids[a].size < cap:
            raise MsdError(f"array {a} holds {min(keys[a].size, rids[a].size)} elements but needs room for int(size * fudge) = {cap}")
    KA = (_u64p * numa)(*[a.ctypes.data_as(_u64p) for a in keys[:numa]])
    RA = (_u64p * numa)(*[a.ctypes.data_as(_u64p) for a in rids[:numa]])
    sz = np.array(list(size)[:numa], dtype=np.uint64)
    desc = (C.c_char_p * 11)()
    times = np.zeros(10, dtype=np.uint64)
    L.sort(KA, RA, sz.ctypes.data_as(_u64p), threads, numa, fudge, desc, times.ctypes.data_as(_u64p))
    for i, s in enumerate(sz):
        size[i] = int(s)
    err = L.msb_64_last_error()
    if err:
        raise MsdError(err.decode())
    return [d.decode() if d is not None else None for d in desc], times


def check(keys: Sequence[np.ndarray], rids: Optional[Sequence[np.ndarray]], size: Sequence[int], numa: Optional[int] = None,
          same: bool = True) -> int:
    """``check(keys, rids, size, numa, same)`` of src/msb_64.c:2470: returns the key
    checksum; aborts the process on an order or key!=rid violation, as the
    reference's asserts do."""
    L = _lib.load()
    numa = len(keys) if numa is None else numa
    KA = (_u64p * numa)(*[a.ctypes.data_as(_u64p) for a in keys[:numa]])
    RA = (_u64p * numa)(*[a.ctypes.data_as(_u64p) for a in rids[:numa]]) if rids is not None else None
    sz = np.array(list(size)[:numa], dtype=np.uint64)
    return int(L.check(KA, RA, sz.ctypes.data_as(_u64p), numa, int(same)))

"""The torch side of what the GPU tests of several families share (a helper module like guardband.py, not a test): integer
dtypes for bit patterns, uploads and read-backs, the dtypes of the Python wrappers, and the flat key distributions of the
direct rounds' tests.  The numpy side -- key types, tables by width, expectations and inputs -- is sort_rows_expect.py.

Plain module, no fixture: ``import gpu_support`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np
import torch

import sort_rows_expect as E

TAIL = 64                           # elements of every output buffer behind the ones that a call may write
_INT = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
# Every name msd_set_option takes, with its default: the table MSD_OPTIONS of csrc/msd_options.hpp restated
# (tests/test_option_defaults.py has tests/options_main.cpp print that table and compares).  Whoever changes an option on the session's
# context restores DEFAULTS[name], never a literal: the next file is to meet the library as it ships.
DEFAULTS = {
    "direct_mode": 1, "direct_min": 1 << 22, "direct_min_parent": 1 << 17, "regpart": 1, "count16": 1, "leaf17": 1, "mid_leaf": 1,
    "early_leaves": 1, "early_plan": 1, "front_count": 1, "front_min": 1 << 29, "merge_leaf": 0, "select_cap": 1 << 20,
    "topk_rows_mode": 0, "topk_rows_lanes": 0, "sort_rows_mode": 0, "sort_rows_lanes": 0, "search_mode": 0, "search_merge_ratio": 32,
}


def restore_defaults(ctx, *names):
    """put the named options (all of them if none is named) back to the library's defaults"""
    for name in names or DEFAULTS:
        ctx.set_option(name, DEFAULTS[name])


def int_dtype(es):
    """the torch integer dtype that carries bit patterns of es bytes"""
    return _INT[es]


def int_dtype_of_key(kt):
    return _INT[np.dtype(E.UT[kt]).itemsize]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_bits(a):
    """unsigned bit patterns as the signed tensor of their width"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()


def host_bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a.view(np.uint64)


def dtypes():
    """(torch dtype, key type) of every dtype the wrappers take"""
    dts = [(torch.int32, E.I32), (torch.float32, E.F32), (torch.int64, E.I64), (torch.float64, E.F64)]
    for name, kt in (("uint32", E.U32), ("uint64", E.U64)):        # (not in every torch)
        if hasattr(torch, name):
            dts.append((getattr(torch, name), kt))
    return dts


def to_gpu(bits, dt):
    return torch.from_numpy(bits.view(np.int32 if bits.itemsize == 4 else np.int64)).cuda().view(dt)


def bits(t):
    return t.view(int_dtype(t.element_size())).cpu().numpy().view(E.UW[t.element_size()])


def shapes(rng, n, kind, bits):
    from oracle import oracle as O
    full = (1 << bits) - 1
    dt = np.uint32 if bits == 32 else np.uint64
    if kind == "uniform":
        k = rng.integers(0, full, n, dtype=np.uint64, endpoint=True)
    elif kind == "sorted":
        k = np.sort(rng.integers(0, full, n, dtype=np.uint64, endpoint=True))
    elif kind == "reversed":
        k = np.sort(rng.integers(0, full, n, dtype=np.uint64, endpoint=True))[::-1].copy()
    elif kind == "stride":      # top digit cycles with the position: every stripe sees one bucket at a time
        k = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 & full)) & np.uint64(full)
    elif kind == "runs":        # long runs of one top digit each (a piece is read long before it can be written)
        top = (np.arange(n, dtype=np.uint64) // np.uint64(4096)) % np.uint64(256)
        k = (top << np.uint64(bits - 8)) | rng.integers(0, (1 << (bits - 8)) - 1, n, dtype=np.uint64)
    elif kind == "lowbits":     # uniform top digit, everything below it constant
        k = rng.integers(0, 255, n, dtype=np.uint64, endpoint=True) << np.uint64(bits - 8)
    elif kind == "zipf":
        k = O.gen_zipf_u32(n, seed=int(rng.integers(1, 1 << 30))).astype(np.uint64)
        if bits == 64:
            k = k << np.uint64(32) | k
    elif kind == "heavy":       # one value takes a third of the input
        k = rng.integers(0, full, n, dtype=np.uint64, endpoint=True)
        k[rng.random(n) < 0.33] = np.uint64(0x5A5A5A5A5A5A5A5A & full)
    else:
        raise ValueError(kind)
    return (k & np.uint64(full)).astype(dt)

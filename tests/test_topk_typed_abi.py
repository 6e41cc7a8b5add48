"""Typed top-k / select (msd_topk_keys, msd_select_key, msd_key_encode, msd_key_decode) without a GPU: the header declares
them with the agreed enum values, the library exports them, arguments are refused before anything touches a device, and
the key codec -- through the two host-only C functions alone -- is a bijection whose unsigned order is the order of the
key type.  Every expectation is computed here with numpy, never with the library."""
import ctypes as C
import re

import numpy as np
import pytest

import abi_support as A
from sort_rows_expect import VIEWS

KEY_TYPES = {"MSD_KEY_U32": 0, "MSD_KEY_I32": 1, "MSD_KEY_F32": 2, "MSD_KEY_U64": 3, "MSD_KEY_I64": 4, "MSD_KEY_F64": 5}
NEW = ["msd_topk_keys", "msd_select_key", "msd_key_encode", "msd_key_decode"]


def test_header_declares_the_functions_and_the_enum():
    _, flat = A.header("msd_radix_hip.h")
    for name, value in KEY_TYPES.items():
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), flat), name
    for f in NEW:
        assert re.search(r"\bint %s\s*\(" % f, flat), f
    for f in ("msd_topk_keys", "msd_select_key"):
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % f, flat)
        args = [a.strip() for a in m.group(1).split(",")]
        assert args[0] == "msd_ctx *ctx" and args[1] == "const void *d_keys" and args[2] == "int key_type", args
    m = re.search(r"\bint msd_topk_keys\s*\(([^)]*)\)", flat)
    assert [a.strip() for a in m.group(1).split(",")][-2:] == ["void *d_out_keys", "uint64_t *d_out_idx"]


def test_library_exports_and_binding_lists_them():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    for f in NEW:
        assert hasattr(L, f), f
        assert f in _lib.EXPORTS, f
        assert getattr(L, f).argtypes is not None, f


def test_arguments_refused_without_a_device():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    v = C.c_uint64(77)
    assert L.msd_topk_keys(None, None, 2, 10, 1, 0, None, None) == -1       # null context
    assert L.msd_select_key(None, None, 2, 10, 1, 0, C.byref(v)) == -1
    assert v.value == 77
    for bad in (6, -1, 100):
        assert L.msd_key_encode(bad, 5, C.byref(v)) == -1 and v.value == 77  # unknown key type
        assert L.msd_key_decode(bad, 5, C.byref(v)) == -1 and v.value == 77
    assert L.msd_key_encode(2, 5, None) == -1 and L.msd_key_decode(2, 5, None) == -1
    for kt in range(6):
        assert L.msd_key_encode(kt, 0, C.byref(v)) == 0


# ---- the codec

def _codec(fn, kt, bits):
    out = np.empty(len(bits), np.uint64)
    v = C.c_uint64()
    for i, b in enumerate(bits.tolist()):
        assert fn(kt, b, C.byref(v)) == 0
        out[i] = v.value
    return out


def _encode(kt, bits):
    from inplacemsdradixsort_amd import _lib
    e = _codec(_lib.load().msd_key_encode, kt, bits)
    if VIEWS[kt][0] == np.uint32:
        assert (e >> np.uint64(32) == 0).all(), "a 32-bit code lives in the low 32 bits"
    return e.astype(VIEWS[kt][0])


def _decode(kt, codes):
    from inplacemsdradixsort_amd import _lib
    return _codec(_lib.load().msd_key_decode, kt, codes).astype(VIEWS[kt][0])


def _float_specials(ut):
    """bit patterns, in ASCENDING totalOrder: -NaN < -inf < ... < -denormal < -0 < +0 < +denormal < ... < +inf < +NaN"""
    if ut == np.uint32:
        sign, inf, qnan, one_mant, max_mant, W = 0x80000000, 0x7F800000, 0x7FC00000, 0x00000001, 0x007FFFFF, 32
        min_normal, max_normal = 0x00800000, 0x7F7FFFFF
    else:
        sign, inf, qnan, one_mant, max_mant, W = 1 << 63, 0x7FF << 52, 0x7FF8 << 48, 1, (1 << 52) - 1, 64
        min_normal, max_normal = 1 << 52, (0x7FE << 52) | ((1 << 52) - 1)
    snan_lo, snan_hi = inf | one_mant, inf | 0x1234    # signalling: quiet bit clear, payload non-zero
    qnan_lo, qnan_hi = qnan, qnan | 0x5555              # quiet, without and with a payload
    all_ones_nan = inf | max_mant
    pos = [0, one_mant, max_mant, min_normal, max_normal, inf, snan_lo, snan_hi, qnan_lo, qnan_hi, all_ones_nan]
    neg = [sign | p for p in reversed(pos)]
    return np.array(neg + pos, dtype=ut), W


def _int_specials(ut, W):
    mn, mx = 1 << (W - 1), (1 << (W - 1)) - 1
    # ascending as signed: MIN, MIN+1, -2, -1, 0, 1, MAX-1, MAX
    m = (1 << W) - 1
    return np.array([mn, mn + 1, m - 1, m, 0, 1, mx - 1, mx], dtype=ut)


def _random_bits(ut, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, np.iinfo(ut).max, n, dtype=ut, endpoint=True)


@pytest.mark.parametrize("kt", range(6))
def test_codec_round_trip_and_order(kt):
    ut, tt = VIEWS[kt]
    W = 32 if ut == np.uint32 else 64
    kind = kt % 3
    if kind == 2:
        specials, _ = _float_specials(ut)
    elif kind == 1:
        specials = _int_specials(ut, W)
    else:
        specials = np.array([0, 1, (1 << (W - 1)) - 1, 1 << (W - 1), (1 << W) - 2, (1 << W) - 1], dtype=ut)
    bits = np.concatenate([_random_bits(ut, 1 << 16, 100 + kt), specials])
    codes = _encode(kt, bits)
    # a bijection: decode(encode(b)) == b, and (on this sample) no two patterns share a code
    assert (_decode(kt, codes) == bits).all()
    assert len(np.unique(codes)) == len(np.unique(bits))
    # the specials, written out in ascending order above, have strictly ascending codes
    sc = codes[len(bits) - len(specials):]
    assert (sc[1:] > sc[:-1]).all(), [hex(int(x)) for x in sc]
    # the expectation in numpy's own words (not the library's formula): unsigned = the pattern; signed = value + 2^(W-1);
    # float = sign clear: pattern with the sign bit set, sign set: all bits inverted
    top = ut(1 << (W - 1))
    if kind == 0:
        want = bits
    elif kind == 1:
        want = bits + top                      # (wraps: two's complement value + 2^(W-1) as an unsigned number)
    else:
        want = np.where(bits & top, ~bits, bits | top)
    assert (codes == want).all()
    # sorting by code = np.sort of the typed view wherever numpy's order is total
    typed = bits.view(tt)
    if kind == 2:
        ok = np.isfinite(typed) & (typed != 0)
        typed, tc, tb = typed[ok], codes[ok], bits[ok]
    else:
        tc, tb = codes, bits
    order = np.argsort(tc, kind="stable")
    assert (typed[order] == np.sort(typed)).all()
    # ... bit for bit (equal values of these subsets have equal bits)
    assert (tb[order] == np.sort(typed).view(ut)).all()


@pytest.mark.parametrize("kt", (2, 5))
def test_float_chain_of_special_values(kt):
    """-NaN < -inf < -max < -min normal < -denormals < -0 < +0 < +denormals < min normal < max < +inf < +NaN, by code"""
    ut, tt = VIEWS[kt]
    specials, W = _float_specials(ut)
    f = specials.view(tt)
    n = len(specials) // 2
    # the list itself is what the chain says (checked with numpy on the values, NaN classes by isnan + signbit)
    assert np.isnan(f[:5]).all() and np.signbit(f[:5]).all() and np.isnan(f[-5:]).all() and not np.signbit(f[-5:]).any()
    assert np.isneginf(f[5]) and np.isposinf(f[-6])
    mid = f[5:-5]
    assert (np.diff(mid.astype(np.float64)) >= 0).all() and mid[n - 6] == 0 and np.signbit(mid[n - 6]) and mid[n - 5] == 0 and not np.signbit(mid[n - 5])
    codes = _encode(kt, specials)
    assert (codes[1:] > codes[:-1]).all()
    # shuffled: sorting by code restores the chain
    rng = np.random.default_rng(kt)
    p = rng.permutation(len(specials))
    assert (specials[p][np.argsort(_encode(kt, specials[p]))] == specials).all()


def test_python_dispatch_refuses_unknown_dtypes():
    """MsdContext._key_type needs no device: the dtype table and its error."""
    import torch
    from inplacemsdradixsort_amd import MsdContext, MsdError
    ctx = A.bare_ctx()
    want = {torch.float32: 2, torch.int32: 1, torch.float64: 5, torch.int64: 4}
    if hasattr(torch, "uint32"):
        want[torch.uint32] = 0
    if hasattr(torch, "uint64"):
        want[torch.uint64] = 3
    for dt, kt in want.items():
        assert ctx._key_type(torch.empty(0, dtype=dt)) == kt
    for dt in (torch.float16, torch.bfloat16, torch.int16, torch.uint8, torch.bool):
        with pytest.raises(MsdError):
            ctx._key_type(torch.empty(0, dtype=dt))
    assert callable(MsdContext.topk_typed) and callable(MsdContext.select_typed)

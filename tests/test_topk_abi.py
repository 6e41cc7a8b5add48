"""Radix select / top-k at the ABI level (no GPU): include/msd_radix_hip.h declares the five entry points and the
MSD_SMALLEST / MSD_LARGEST enum, the built library exports the symbols, the Python binding lists them."""
import re

import abi_support as A

SYMBOLS = ["msd_topk_u32", "msd_topk_u64", "msd_topk_pairs_u64", "msd_select_u32", "msd_select_u64"]


def test_header_declares_topk_and_select():
    _, h = A.header("msd_radix_hip.h")
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*msd_ctx\s*\*" % s, h), s
    # inputs are const: the calls do not modify the caller's arrays
    assert re.search(r"msd_topk_u32\s*\(\s*msd_ctx\s*\*\s*\w*\s*,\s*const\s+uint32_t\s*\*", h)
    assert re.search(r"msd_topk_pairs_u64\s*\(\s*msd_ctx\s*\*\s*\w*\s*,\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*const\s+uint64_t\s*\*", h)
    assert re.search(r"msd_select_u64\s*\(\s*msd_ctx\s*\*\s*\w*\s*,\s*const\s+uint64_t\s*\*", h)


def test_enum_values():
    m = re.search(r"enum\s*\{([^}]*MSD_SMALLEST[^}]*)\}", A.header("msd_radix_hip.h")[1])
    assert m, "enum with MSD_SMALLEST not found"
    vals = dict((k, int(v)) for k, v in re.findall(r"(MSD_\w+)\s*=\s*(-?\d+)", m.group(1)))
    assert vals == {"MSD_SMALLEST": 0, "MSD_LARGEST": 1}


def test_library_exports_topk_and_select():
    from inplacemsdradixsort_amd import _lib
    L = _lib.load()
    missing = [s for s in SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert set(SYMBOLS) <= set(_lib.EXPORTS)
    # a null context is refused before anything else is looked at (MSD_EINVAL = -1)
    assert L.msd_topk_u32(None, None, 0, 0, 0, None) == -1
    assert L.msd_select_u64(None, None, 1, 0, 0, None) == -1

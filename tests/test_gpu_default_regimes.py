"""The whole-array sorts with the library's DEFAULT options at the sizes where its planner changes path, and at full
size -- with an exact verdict.  numpy cannot sort these inputs in a test's time, and the tests that lower thresholds to
reach a path at a small size run another configuration than the one that ships; here no option is ever set, the inputs
are made on the device, and the verdict is that of tests/exact_verdict.py (ascending + the input's multiset by a
fingerprint taken in place before the sort: that is the definition of the sorted array).  Nothing crosses to the host
but scalars.

Thresholds T (csrc/msd_radix.hip, SortRun), each at n = T - 3 and n = T + 5 (odd lengths: keys behind the last 16-byte
vector, a short last chunk):
  2^22  `direct_min`: the first round places its blocks directly from here on
  2^24  the leading-bit skip trusts a sample and is verified later (skip_leading_bits)
  2^25  u64 keys / tuples: round 1's 256 parents reach `direct_min_parent` = 2^17 on evenly spread keys (necessary for a
        direct round 1, not sufficient: their digit is still narrower than 8 bits, see check_path)
  2^27  u32 keys: two 8-bit rounds (pick_width)
  2^28  u64 keys / tuples: 2 and 4 GiB; round 1's parents (2^20 elements) get an 8-bit digit as tuples, a 7-bit one as keys
  2^29  `front_min`: the front pass (csrc/msd_front16.hpp) counts the top 16 bits once
  2^32  the front pass's upper bound, and element indices that no longer fit 32 bits

The path is asserted only where the code's rule fixes it for the input; everywhere the failure message carries
ctx.stats().  The cases are ordered small, large, small, ...: workspace growth, reuse after a larger call and the path
switches all happen on one context."""
import pytest
import torch

import exact_verdict as V

pytestmark = pytest.mark.gpu

U32_ALL = ["uniform", "zipf", "dup", "sorted", "reversed", "topzero", "outlier"]
U64_ALL = ["uniform", "upperzero", "zipf64", "dup", "sorted"]
DISTINCT = 5000


def _cases():
    out = []
    for log in (22, 24, 27, 29):
        for d in (U32_ALL if log != 27 else ["uniform"]):
            out += [("u32", (1 << log) + delta, d) for delta in (-3, 5)]
    for d in ("uniform", "zipf"):
        out += [("u32", (1 << 32) + delta, d) for delta in (-3, 5)]
    for layout in ("u64", "tuples"):
        for log in (22, 24, 25, 28):
            for d in U64_ALL:
                out += [(layout, (1 << log) + delta, d) for delta in (-3, 5)]
    out.sort(key=lambda c: (c[1] * (4 if c[0] == "u32" else 8 if c[0] == "u64" else 16), c))   # by bytes ...
    mixed = []
    while out:                                                                                   # ... then small, large, small, ...
        mixed.append(out.pop(0))
        if out:
            mixed.append(out.pop())
    return mixed


def _name(n):
    log = (n + 3).bit_length() - 1
    return f"2^{log}{n - (1 << log):+d}"


@pytest.fixture(scope="module")
def dctx():
    """a context of its own on which no option is ever set: the library's defaults, whatever the session's context went through"""
    from inplacemsdradixsort_amd import MsdContext
    c = MsdContext(0)

    def refuse(*a, **k):
        raise AssertionError("this file runs the defaults: no set_option on its context")
    c.set_option = refuse
    yield c
    c.close()
    torch.cuda.empty_cache()


def make_u32(c, n, dist):
    t = torch.empty(n, dtype=torch.int32, device="cuda")
    if dist == "zipf":
        c.gen_zipf_u32(t)
    elif dist == "dup":
        c.gen_dup_u32(t, DISTINCT)
    else:
        c.gen_uniform_u32(t, first=n & 0xFFFF)
    if dist in ("sorted", "reversed"):
        c.sort_u32(t)
        assert V.order_violations(t) == 0, "the input of this case is not sorted"
        if dist == "reversed":
            t = torch.flip(t, dims=[0])
    if dist in ("topzero", "outlier"):            # 8 constant leading bits (a logical shift) ...
        t.bitwise_right_shift_(8).bitwise_and_(0x00FFFFFF)
        if dist == "outlier":                     # ... but for one key, where the strided sample does not look
            t[12345] |= 1 << 29
    return t


def make_u64(c, n, dist):
    t = torch.empty(n, dtype=torch.int64, device="cuda")
    if dist in ("zipf64", "dup"):                 # (z << 32) | z of a 4-byte value
        z = torch.empty(n, dtype=torch.int32, device="cuda")
        if dist == "zipf64":
            c.gen_zipf_u32(z)
        else:
            c.gen_dup_u32(z, DISTINCT)
        t.copy_(z).bitwise_and_(0xFFFFFFFF)
        del z
        t.bitwise_or_(t << 32)
    else:
        c.gen_uniform_u64(t, first=n & 0xFFFF, shift_right=32 if dist == "upperzero" else 0)
    if dist == "sorted":
        c.sort_u64(t)
        assert V.order_violations(t) == 0, "the input of this case is not sorted"
    return t


def check_path(layout, n, dist, st):
    """what SortRun's rules fix for these inputs"""
    if layout == "u32" and dist == "uniform":
        if n in ((1 << 22) - 3, (1 << 22) + 5):                      # direct_min (classify_direct: round_keys >= direct_min)
            assert (st.get("direct_rounds", 0) >= 1) == (n > 1 << 22), st
        tried = st.get("front_count_sorts", 0) + st.get("front_count_declined", 0)
        assert tried == (1 if (1 << 29) <= n < (1 << 32) else 0), st   # front_count(): front_min <= n < 2^32
        if n == (1 << 29) + 5:
            assert st.get("front_count_sorts", 0) == 1, st
        if n == (1 << 32) - 3:                                       # taken or declined (classify_direct's 16-bit piece bound): recorded
            print(f"front pass at 2^32-3: sorts {st.get('front_count_sorts', 0)}, declined {st.get('front_count_declined', 0)}, stats {st}")
    if layout == "u32" and dist == "outlier" and n > 1 << 24:        # skip_leading_bits: a sampled skip from 2^24 on, refuted later
        assert st.get("bit_skip_restarts", 0) == 1, st
    if layout != "u32" and dist == "uniform":
        # Round 0 is direct from direct_min on.  Round 1 needs more than parents of direct_min_parent = 2^17 elements (n =
        # 2^25): classify_direct tries a round only if every parent has an 8-bit digit, and pick_width gives one to parents
        # of more than 128 * small_max / 2 elements.  u64 keys (small_max 17408): 1114112, more than the 2^20 of n = 2^28
        # -- measured: 4352 children = 256 + 256 * 16 at 2^25 + 5, 33024 = 256 + 256 * 128 at 2^28 +- , direct_rounds 1 at
        # both.  Tuples (small_max 3072): 196608, so round 1 is direct at 2^28 and not yet at 2^25.
        if n < 1 << 22:
            assert st.get("direct_rounds", 0) == 0, st
        else:
            assert st.get("direct_rounds", 0) >= (2 if layout == "tuples" and n > 1 << 27 else 1), st


@pytest.mark.parametrize("layout,n,dist", _cases(), ids=lambda v: _name(v) if isinstance(v, int) else v)
def test_default_regime(dctx, layout, n, dist):
    rids = None
    if layout == "u32":
        keys = make_u32(dctx, n, dist)
    else:
        keys = make_u64(dctx, n, dist)
        if layout == "tuples":
            rids = torch.empty(n, dtype=torch.int64, device="cuda")
            dctx.gen_iota_u64(rids)
    fp = V.fingerprint(keys, rids)
    assert fp[0] == n
    if layout == "u32":
        dctx.sort_u32(keys)
    elif layout == "u64":
        dctx.sort_u64(keys)
    else:
        dctx.sort_pairs_u64(keys, rids)
    st = dctx.stats()
    try:
        V.assert_sorted_permutation(fp, keys, rids)
    except AssertionError as e:
        raise AssertionError(f"{layout} {_name(n)} {dist}: {e}; stats {st}") from None
    check_path(layout, n, dist, st)
    del keys, rids
    if n >= 1 << 29:
        torch.cuda.empty_cache()

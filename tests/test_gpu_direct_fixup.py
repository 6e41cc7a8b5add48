"""GPU parity of a round's fix-up and of the leaves that follow a last round without waiting for it.

What is under test: the child scan spread over stripe groups (child_scan_part_kernel / child_scan_split_kernel), the
cleanup launch that also checks the chains' lists and places the excess blocks, collect_kernel run behind the child scan,
the plan brought over by round_init_kernel, and the counting leaves enqueued behind a last round from an early copy of
the counters (`early_leaves`, stat `leaves_behind_round`).  The oracle is numpy's sort of the same keys, bit-exact; for
tuples the rid permutation as in tests/test_gpu_direct.py.  Every buffer is guard-banded (tests/guardband.py).
"""
import numpy as np
import pytest

import guardband
from gpu_support import restore_defaults, shapes

pytestmark = pytest.mark.gpu

U32_SMALL_MAX = 24576       # Cfg<u32>: what one LDS sort takes
U64_SMALL_MAX = 17408
STRIPE_MIN = 4 * 4096       # plan_round: a stripe has at least four classify tiles
# kChildScanSplit (csrc/msd_device.hpp): parents of this many stripes are scanned by stripe groups.  (A copy: the cases
# around it also assert, through the stat `child_scan_split_rounds`, which kernels ran -- if the library's constant moves,
# they fail instead of passing beside the threshold.)
CHILD_SCAN_SPLIT = 64


@pytest.fixture()
def dctx(ctx):
    ctx.set_option("direct_min", 1 << 16)
    ctx.set_option("direct_min_parent", 1 << 12)
    ctx.set_option("direct_mode", 1)
    ctx.set_option("early_leaves", 1)
    yield ctx
    restore_defaults(ctx, "direct_min", "direct_min_parent", "direct_mode", "early_leaves")


def sort_checked(ctx, k, typ="u32", lead=0, what=""):
    """Sorts k (numpy u32 / u64) inside guard bands, asserts the result against numpy, returns stats()."""
    import torch
    n = k.size
    a = guardband.Arena(torch.int32 if typ == "u32" else torch.int64, n, lead_bytes=lead, guard=1 << 16).fill(k)
    if typ == "pairs":
        r = np.arange(n, dtype=np.uint64)
        ar = guardband.Arena(torch.int64, n, guard=1 << 16).fill(r)
        ctx.sort_pairs_u64(a.payload, ar.payload)
        ko, ro = a.host(np.uint64), ar.host(np.uint64)
        ar.check(what + " rids")
        assert (k[ro] == ko).all() and (np.sort(ro) == r).all(), what
    elif typ == "u32":
        ctx.sort_u32(a.payload)
        ko = a.host(np.uint32)
    else:
        ctx.sort_u64(a.payload)
        ko = a.host(np.uint64)
    st = ctx.stats()
    a.check(what)
    assert (ko == np.sort(k)).all(), (what, st)
    return st


# ---------------------------------------------------------------- direct rounds, every distribution

@pytest.mark.parametrize("n", [(1 << 16) + 5, (1 << 22) + 131])
def test_uniform_u32_direct(dctx, n):
    if n < 1 << 22:
        dctx.set_option("direct_mode", 2)   # (a digit narrower than 8 bits is placed directly only when forced)
    k = shapes(np.random.default_rng(n), n, "uniform", 32)
    st = sort_checked(dctx, k, what=f"uniform n={n}")
    assert st.get("direct_rounds", 0) >= 1, st


@pytest.mark.parametrize("kind", ["zipf", "heavy", "sorted", "runs"])
@pytest.mark.parametrize("typ", ["u32", "u64", "pairs"])
def test_forced_direct_any_distribution(dctx, kind, typ):
    dctx.set_option("direct_mode", 2)
    rng = np.random.default_rng(11 + len(kind) * 17 + len(typ))
    n = (1 << 21) + 77
    st = sort_checked(dctx, shapes(rng, n, kind, 32 if typ == "u32" else 64), typ, what=f"{kind} {typ}")
    assert st.get("direct_rounds", 0) >= 1, st


def test_no_holes_at_all(dctx):
    """`lowbits`: 256 values, every block of a direct round is in place or one short list."""
    dctx.set_option("direct_mode", 2)
    k = shapes(np.random.default_rng(3), (1 << 20) + 64, "lowbits", 32)
    st = sort_checked(dctx, k, what="lowbits")
    assert st.get("direct_rounds", 0) == 1, st


# ---------------------------------------------------------------- the child scan, by the parent's stripe count

@pytest.mark.parametrize("stripes", [1, 3, CHILD_SCAN_SPLIT - 1, CHILD_SCAN_SPLIT, CHILD_SCAN_SPLIT + 1, 2 * CHILD_SCAN_SPLIT + 7])
def test_child_scan_one_parent(dctx, stripes):
    """u64 keys, one round of one parent: n = stripes x the smallest stripe (+ a little: the last stripe takes the rest)."""
    n = STRIPE_MIN * stripes + (100 if stripes > 1 else 3616)
    assert n > U64_SMALL_MAX
    k = shapes(np.random.default_rng(100 + stripes), n, "uniform", 64)
    st = sort_checked(dctx, k, "u64", what=f"{stripes} stripes")
    assert st["rounds"] == 1 and st["parents"] == 1 and st["stripes"] == stripes, st
    assert st.get("child_scan_split_rounds", 0) == (1 if stripes >= CHILD_SCAN_SPLIT else 0), st


@pytest.mark.parametrize("stripes", [CHILD_SCAN_SPLIT - 1, CHILD_SCAN_SPLIT + 1])
def test_child_scan_one_parent_direct_u32(dctx, stripes):
    """The same around the threshold for a direct round of u32 keys (B = 64; the digit has 7 bits at this size: forced)."""
    dctx.set_option("direct_mode", 2)
    n = STRIPE_MIN * stripes + 321
    k = shapes(np.random.default_rng(200 + stripes), n, "uniform", 32)
    st = sort_checked(dctx, k, lead=16, what=f"{stripes} stripes, direct")
    assert st["direct_rounds"] == 1 and st["stripes"] == stripes, st
    assert st.get("child_scan_split_rounds", 0) == (1 if stripes >= CHILD_SCAN_SPLIT else 0), st


def test_child_scan_many_parents_second_round(dctx):
    """2^26 + 12345 keys, both rounds placed directly (as test_direct_second_round_u32): the first round's parent is
    scanned by stripe groups, the second round's 256 parents by one workgroup each.  (Its digit is 5 bits wide: 19 bits
    stay open, so it is no last round and its children go to the LDS leaves.)"""
    dctx.set_option("direct_mode", 2)
    n = (1 << 26) + 12345
    k = shapes(np.random.default_rng(31), n, "uniform", 32)
    st = sort_checked(dctx, k, what="two direct rounds")
    assert st.get("direct_rounds", 0) == 2 and st.get("leaves_behind_round", 0) == 0 and st["children"] == 256 + 256 * 32, st
    assert st.get("child_scan_split_rounds", 0) == 1, st


# ---------------------------------------------------------------- cleanup: leftovers, excess blocks

def test_cleanup_short_and_empty_children(dctx):
    """Children shorter than a block (no interior slot), an empty bucket between two that have leftovers, and one whose
    few keys lie across the block grid: top digits 5, 6, 7, 8 hold 3, 0, 10 and 70 keys."""
    dctx.set_option("direct_mode", 2)
    rng = np.random.default_rng(77)
    n = (1 << 20) + 37
    k = shapes(rng, n, "uniform", 32)
    top = k >> 24
    k[(top >= 5) & (top <= 8)] |= np.uint32(0x10000000)          # empty the four buckets ...
    for digit, cnt in ((5, 3), (7, 10), (8, 70)):                  # ... and put a few keys back
        at = rng.choice(n, cnt, replace=False)
        k[at] = (np.uint32(digit) << 24) | (k[at] & np.uint32(0xFFFFFF))
    cnt = np.bincount(k >> 24, minlength=256)
    assert cnt[6] == 0 and 0 < cnt[5] < 64 and 0 < cnt[7] < 64 and 64 <= cnt[8] < 128
    st = sort_checked(dctx, k, lead=48, what="short children")
    assert st.get("direct_rounds", 0) >= 1, st


@pytest.mark.parametrize("typ", ["u32", "pairs"])
def test_cleanup_excess_blocks(dctx, typ):
    """Descending keys: stripes full of one bucket leave children with more full blocks than interior slots.  (The plan
    of a direct round declines keys that come in runs: this round streams, the cleanup launch is the same.)"""
    n = 1 << 21
    k = shapes(np.random.default_rng(5), n, "reversed", 32 if typ == "u32" else 64)
    st = sort_checked(dctx, k, typ, what="reversed")
    assert st.get("excess_blocks", 0) >= 1 and st.get("direct_rounds", 0) == 0, st


def test_cleanup_reversed_forced_direct(dctx):
    """The same keys placed directly (forced)."""
    dctx.set_option("direct_mode", 2)
    k = shapes(np.random.default_rng(5), 1 << 21, "reversed", 32)
    st = sort_checked(dctx, k, what="reversed, forced direct")
    assert st.get("direct_rounds", 0) >= 1, st


# ---------------------------------------------------------------- leaves behind the last round

def low24(seed, n):
    return (shapes(np.random.default_rng(seed), n, "uniform", 32) & np.uint32(0xFFFFFF)).astype(np.uint32)


def leaf_case(name):
    n = (1 << 22) + 9
    k = low24(901, n)
    if name == "crowded":          # one value 300 times inside one child: a byte counter overflows, the segment is handed on
        k[np.random.default_rng(902).choice(n, 300, replace=False)] = np.uint32(0x00ABCDEF)
    elif name == "third":          # one value on a third of the input: its child is a big counting segment
        k[np.random.default_rng(903).random(n) < 1 / 3] = np.uint32(0x00123456)
    return k


# stats of the parent commit 7828197 for these seeded inputs (every round ended with its own readback there)
LEAF_STATS = {
    "uniform": {"rounds": 1, "count_segments": 256, "big_count_segments": 0},
    "crowded": {"rounds": 1, "count_segments": 256, "big_count_segments": 0},
    "third": {"rounds": 1, "count_segments": 255, "big_count_segments": 1},
}


@pytest.mark.parametrize("name", sorted(LEAF_STATS))
def test_leaves_behind_last_round(dctx, name):
    """u32 keys below 2^24 (24 open bits behind the bit skip): the one round is the last, its children go to the counting
    leaves while its fix-up runs."""
    k = leaf_case(name)
    st = sort_checked(dctx, k, what=name)
    print(name, st)
    assert st.get("leaves_behind_round", 0) == 1 and st.get("skipped_bits", 0) == 8, st
    assert {key: st.get(key, 0) for key in LEAF_STATS[name]} == LEAF_STATS[name], st
    assert st.get("direct_rounds", 0) == (0 if name == "third" else 1), st
    if name == "crowded":
        # the crowded segment overflows a byte counter in both register-resident kernels: it is handed on twice, on top
        # of whatever the same keys without the 300 copies hand on
        base = sort_checked(dctx, leaf_case("uniform"), what="uniform, for comparison")
        for key in ("count16_rejected", "count_slow_segments"):
            assert st.get(key, 0) == base.get(key, 0) + 1, (key, st, base)
    dctx.set_option("early_leaves", 0)                       # the same with every round's own readback
    st0 = sort_checked(dctx, k, what=name + " early_leaves=0")
    assert st0.get("leaves_behind_round", 0) == 0, st0
    for key in ("rounds", "parents", "stripes", "children", "slots", "count_segments", "big_count_segments", "small_segments", "direct_rounds"):
        assert st0.get(key, 0) == st.get(key, 0), (key, st0, st)


RESTART_STATS = {"rounds": 3, "count_segments": 256, "big_count_segments": 0, "bit_skip_restarts": 1}   # parent commit 7828197


def test_wrong_sampled_bit_skip_restarts_before_any_leaf(dctx):
    """2^24 + 1 keys below 2^24 but one, which the strided sample does not see: the exact check fails behind the first
    round, before any leaf has run; the sort starts over and its last round is followed by the leaves."""
    n = (1 << 24) + 1
    k = low24(904, n)
    stride = n // 8192
    k[5 * stride + 1001] |= np.uint32(0x80000000)
    st = sort_checked(dctx, k, what="wrong skip")
    print(st)
    assert {key: st.get(key, 0) for key in RESTART_STATS} == RESTART_STATS, st
    assert st.get("leaves_behind_round", 0) == 1, st


def test_three_sorts_back_to_back(dctx):
    """Different sizes on one context: nothing of a round that the leaves followed may leak into the next call."""
    for seed, n in ((1, (1 << 22) + 9), (2, (1 << 19) + 1), (3, (1 << 23) + 4097)):
        st = sort_checked(dctx, low24(seed, n), what=f"n={n}")
        assert st.get("leaves_behind_round", 0) == 1, st
        st = sort_checked(dctx, shapes(np.random.default_rng(seed), n, "uniform", 32), what=f"n={n} 32 bits")
        assert st["rounds"] >= 1, st

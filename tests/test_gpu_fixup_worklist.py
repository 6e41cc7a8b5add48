"""GPU parity of the fix-up's slot sweeps over marked groups, of the cleanup by runs and of the early plan of a next round.

What is under test: slot_classify_kernel marks the groups of 8 slots that are not settled and walks only those
(csrc/msd_device.hpp), cleanup_kernel copies each bucket's leftovers as a run, and a round that is not the last has the
next round planned and enqueued while its fix-up runs (`early_plan`, stat `rounds_planned_early`).  The oracle is numpy's
sort of the same keys, bit-exact; for tuples the rid permutation as in tests/test_gpu_direct.py.  Every buffer is
guard-banded (tests/guardband.py).  A lost or doubled list entry is caught by the library's own invariants (the chains must
use up every list exactly: sites 3-5, MSD_EINTERNAL) and by the comparison.  Nothing here asserts a number that varies
from run to run (holes, chain steps).

The marking has no capacity an input can reach: its list holds every group of the longest part a stripe can have (a stripe
has at most 1.5 x 2^20 elements, a block at least 32, a part is half a stripe), and a longer part would be swept in full
like a streaming round's.  So there is no case at or above a capacity.
"""
import numpy as np
import pytest

import guardband
from gpu_support import restore_defaults, shapes

pytestmark = pytest.mark.gpu

STRIPE_MIN = 4 * 4096       # plan_round: a stripe has at least four classify tiles
PLAN_STATS = ("rounds", "parents", "stripes", "children", "slots", "direct_rounds", "leaves_behind_round", "bit_skip_restarts")


@pytest.fixture()
def wctx(ctx):
    ctx.set_option("direct_min", 1 << 16)
    ctx.set_option("direct_min_parent", 1 << 12)
    ctx.set_option("direct_mode", 1)
    ctx.set_option("early_plan", 1)
    yield ctx
    restore_defaults(ctx, "direct_min", "direct_min_parent", "direct_mode", "early_plan")


def sort_checked(ctx, k, typ="u32", lead=0, what="", expect=None):
    """Sorts k (numpy u32 / u64) inside guard bands, asserts the result against numpy (`expect`: np.sort(k), if the caller
    has it already), returns stats()."""
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
    assert (ko == (np.sort(k) if expect is None else expect)).all(), (what, st)
    return st


def short_children(seed=77, counts=((5, 3), (7, 10), (8, 70))):
    """The input of test_gpu_direct_fixup.test_cleanup_short_and_empty_children: 2^20 + 37 uniform u32 keys whose top
    digits 5 .. 8 are emptied, and `counts` = (digit, keys) put back."""
    rng = np.random.default_rng(seed)
    n = (1 << 20) + 37
    k = shapes(rng, n, "uniform", 32)
    top = k >> 24
    lo, hi = min(d for d, _ in counts) & ~1, max(d for d, _ in counts) | 1
    k[(top >= lo) & (top <= hi)] |= np.uint32(0x40000000)
    for digit, cnt in counts:
        at = rng.choice(n, cnt, replace=False)
        k[at] = (np.uint32(digit) << 24) | (k[at] & np.uint32(0xFFFFFF))
    got = np.bincount(k >> 24, minlength=256)
    for d in range(lo, hi + 1):
        assert got[d] == dict(counts).get(d, 0), (d, got[d])
    return k


# ---------------------------------------------------------------- slot sweeps, direct placement forced

def test_no_odd_slot(wctx):
    """`lowbits`: 256 values, every block of the direct round is in place or in one short list."""
    wctx.set_option("direct_mode", 2)
    k = shapes(np.random.default_rng(3), (1 << 20) + 64, "lowbits", 32)
    st = sort_checked(wctx, k, what="lowbits")
    assert st.get("direct_rounds", 0) == 1, st


def test_many_odd_slots(wctx):
    """Uniform keys: sampled boundaries, stolen and empty slots."""
    wctx.set_option("direct_mode", 2)
    n = (1 << 22) + 131
    st = sort_checked(wctx, shapes(np.random.default_rng(n), n, "uniform", 32), what="uniform")
    assert st.get("direct_rounds", 0) >= 1, st


def test_uniform_at_the_smallest_direct_round(wctx):
    """2^16 + 5 uniform u32 keys: one direct round of 4 stripes, parts of 128 slots."""
    wctx.set_option("direct_mode", 2)
    n = (1 << 16) + 5
    st = sort_checked(wctx, shapes(np.random.default_rng(n), n, "uniform", 32), what=f"n={n}")
    assert st.get("direct_rounds", 0) == 1 and st["rounds"] == 1, st


def test_children_shorter_than_a_group(wctx):
    """64 neighbouring children of 3 .. 5 blocks each (interiors of 2 .. 4 slots, starts anywhere on the block grid): no
    group of 8 slots there lies inside one child's interior, every group spans several children.  (Uniform keys cannot
    give such children: the planner picks the digit so that a child has about 12288 keys, 3 bits at 2^16 keys and 7 at
    2^20 -- so the keys are built, for the 7-bit digit this size gets; with an 8-bit digit the children would be half as
    long, 1 .. 3 blocks.  `children` says that the digit was no narrower.)"""
    wctx.set_option("direct_mode", 2)
    rng = np.random.default_rng(99)
    n = (1 << 20) + 37
    k = shapes(rng, n, "uniform", 32)
    mid = np.flatnonzero(((k >> 25) >= 8) & ((k >> 25) < 72))
    # empty the 64 children: their keys go, evenly, to the children behind them ...
    k[mid] = (rng.integers(72, 128, mid.size, dtype=np.uint64).astype(np.uint32) << 25) | (k[mid] & np.uint32(0x1FFFFFF))
    at = rng.permutation(n)
    o = 0
    for c in range(8, 72):                                 # ... and each gets 192 .. 320 keys back
        cnt = 192 + (c * 37) % 129
        sel = at[o:o + cnt]
        o += cnt
        k[sel] = (np.uint32(c) << 25) | (k[sel] & np.uint32(0x1FFFFFF))
    per_child = np.bincount(k >> 25, minlength=128)
    assert ((per_child[8:72] >= 192) & (per_child[8:72] <= 320)).all() and per_child.max() <= 24576, per_child
    st = sort_checked(wctx, k, what="short children in a row")
    assert st.get("direct_rounds", 0) >= 1 and st["children"] >= 128, st


@pytest.mark.parametrize("lead", [16, 48])
@pytest.mark.parametrize("stripes", [1, 3, 63, 65])
def test_parts_off_the_group_grid(wctx, stripes, lead):
    """Stripe parts that start off the 8-slot grid (the payload starts 16 or 48 bytes behind a page boundary, the stripes
    321 keys off any round size), parts of 128 slots.  (The two small sizes lie below the fixture's `direct_min`: it is
    lowered for them.  16705 u32 keys fit one LDS leaf: no round at all, the case only stays for the list's sake.)"""
    wctx.set_option("direct_mode", 2)
    n = STRIPE_MIN * stripes + 321
    if n < 1 << 16:
        wctx.set_option("direct_min", 1 << 14)
    st = sort_checked(wctx, shapes(np.random.default_rng(200 + stripes), n, "uniform", 32), lead=lead, what=f"{stripes} stripes, lead {lead}")
    if stripes > 1:
        assert st["stripes"] == stripes and st.get("direct_rounds", 0) >= (1 if n >= 1 << 16 else 0), st


def test_groups_across_interior_ends(wctx):
    """Buckets of 3, 0, 10 and 70 keys between full ones: groups full of one bucket's blocks that reach or cross that
    bucket's interior end, children without an interior slot."""
    wctx.set_option("direct_mode", 2)
    st = sort_checked(wctx, short_children(), lead=48, what="short children")
    assert st.get("direct_rounds", 0) >= 1, st


@pytest.mark.parametrize("kind", ["uniform", "zipf", "sorted", "runs"])
@pytest.mark.parametrize("typ", ["u64", "pairs"])
def test_other_types(wctx, kind, typ):
    """B = 32."""
    wctx.set_option("direct_mode", 2)
    n = (1 << 21) + 77
    st = sort_checked(wctx, shapes(np.random.default_rng(11 + len(kind) * 17 + len(typ)), n, kind, 64), typ, what=f"{kind} {typ}")
    assert st.get("direct_rounds", 0) >= 1, st


@pytest.mark.parametrize("kind", ["zipf", "reversed"])
def test_streaming_rounds(wctx, kind):
    """No direct placement: there is no map of full slots, nearly every block is misplaced, and the sweeps take every group."""
    wctx.set_option("direct_mode", 0)
    st = sort_checked(wctx, shapes(np.random.default_rng(21 + len(kind)), 1 << 21, kind, 32), what=kind)
    assert st.get("direct_rounds", 0) == 0, st


# ---------------------------------------------------------------- cleanup by runs

@pytest.mark.parametrize("typ", ["u32", "pairs"])
def test_cleanup_excess_blocks_and_streams(wctx, typ):
    """Descending keys: the round streams (the plan of a direct round declines runs), children have excess blocks."""
    k = shapes(np.random.default_rng(5), 1 << 21, "reversed", 32 if typ == "u32" else 64)
    st = sort_checked(wctx, k, typ, what="reversed")
    assert st.get("excess_blocks", 0) >= 1 and st.get("direct_rounds", 0) == 0, st


@pytest.mark.parametrize("lead", [0, 16, 48])
def test_cleanup_runs_cross_head_to_tail(wctx, lead):
    """Children of B + a few, 2 B + a few and 3 B + a few keys (B = 64) that start off the block grid: their keys are
    leftovers of many stripes, a few each, and the runs go from the child's head across its interior to its tail."""
    wctx.set_option("direct_mode", 2)
    k = short_children(78 + lead, counts=((4, 64 + 3), (6, 128 + 5), (8, 192 + 7), (10, 5)))
    st = sort_checked(wctx, k, lead=lead, what=f"head to tail, lead {lead}")
    assert st.get("direct_rounds", 0) >= 1, st


# ---------------------------------------------------------------- the next round planned under the fix-up

def low24(seed, n):
    return (shapes(np.random.default_rng(seed), n, "uniform", 32) & np.uint32(0xFFFFFF)).astype(np.uint32)


def test_two_general_rounds_planned_early_or_not(wctx):
    n = (1 << 23) + 4097
    k = shapes(np.random.default_rng(41), n, "uniform", 32)
    expect = np.sort(k)
    sort_checked(wctx, k, what="warm-up (buffers grow once)", expect=expect)
    st1 = sort_checked(wctx, k, what="early_plan=1", expect=expect)
    wctx.set_option("early_plan", 0)
    st0 = sort_checked(wctx, k, what="early_plan=0", expect=expect)
    print(st1, st0)
    assert st1["rounds"] >= 2, st1
    assert st1.get("rounds_planned_early", 0) >= 1 and st0.get("rounds_planned_early", 0) == 0, (st1, st0)
    for key in PLAN_STATS:
        assert st1.get(key, 0) == st0.get(key, 0), (key, st1, st0)


def test_early_plan_not_behind_a_wrong_bit_skip(wctx):
    """The input of test_gpu_direct_fixup.test_wrong_sampled_bit_skip_restarts_before_any_leaf: the one round behind the
    wrong skip leaves no parent (nothing to plan early) and the sort starts over; only the round behind the restart has a
    next round to plan."""
    n = (1 << 24) + 1
    k = low24(904, n)
    k[5 * (n // 8192) + 1001] |= np.uint32(0x80000000)
    expect = np.sort(k)
    sort_checked(wctx, k, what="warm-up", expect=expect)
    st = sort_checked(wctx, k, what="wrong skip", expect=expect)
    print(st)
    assert st.get("bit_skip_restarts", 0) == 1 and st["rounds"] == 3 and st.get("leaves_behind_round", 0) == 1, st
    assert st.get("rounds_planned_early", 0) <= 1, st
    wctx.set_option("early_plan", 0)
    st0 = sort_checked(wctx, k, what="wrong skip, early_plan=0", expect=expect)
    for key in PLAN_STATS:
        assert st.get(key, 0) == st0.get(key, 0), (key, st, st0)


@pytest.mark.parametrize("typ", ["u64", "pairs"])
def test_early_plan_falls_back_register_resident(wctx, typ):
    """u64 keys and tuples at 2^21: the next parents take a register-resident pass, nothing is enqueued ahead."""
    k = shapes(np.random.default_rng(43), 1 << 21, "uniform", 64)
    sort_checked(wctx, k, typ, what="warm-up")
    st = sort_checked(wctx, k, typ, what=typ)
    assert st.get("rounds_planned_early", 0) == 0, st


def test_early_plan_one_round(wctx):
    """A one-round sort: the leaves follow the round as before."""
    st = sort_checked(wctx, low24(901, (1 << 22) + 9), what="one round")
    assert st.get("rounds_planned_early", 0) == 0 and st.get("leaves_behind_round", 0) == 1 and st["rounds"] == 1, st


def test_three_sorts_back_to_back(wctx):
    """Different sizes on one context: nothing of an early-planned round may leak into the next call."""
    for seed, n in ((1, (1 << 23) + 4097), (2, (1 << 19) + 1), (3, (1 << 22) + 9), (4, (1 << 23) + 4097)):
        st = sort_checked(wctx, shapes(np.random.default_rng(seed), n, "uniform", 32), what=f"n={n}")
        assert st["rounds"] >= 1, st
        st = sort_checked(wctx, low24(seed, n), what=f"n={n}, 24 bits")
        assert st.get("leaves_behind_round", 0) == 1, st


def test_parked_round_blocks_the_next_plan(wctx):
    """A round is parked, the round behind it must not plan ahead -- its ordinary summary brings the parked counters --
    and a later round plans ahead again.  2^25 + 4097 u64 keys made on the device: bits 63, 55, 47 and 39 are independent
    random bits, the low 32 bits uniform, everything else zero, and no register-resident pass (`regpart` 0).  So the general
    rounds have 1, 2, 4, 8 and 16 parents (an 8-bit digit each, of which one bit varies); rounds 0 and 2 are planned early,
    round 1 finds round 0 parked, round 3 finds round 2 parked (and its average child, 16384 keys, is below the leaf
    capacity, 17408), round 4 is the last.  The verdict is that of tests/exact_verdict.py.
    (The stats of the commit before the host code was rewritten, `early_plan` 1 and 0 alike but for the first: rounds_planned_early
    2 / 0, rounds 5, parents 31, stripes 4555, children 7936, slots 5243496, small_segments 4096, no direct round, no leaves
    behind a round, no restart.)"""
    import torch

    import exact_verdict as V
    from gpu_support import DEFAULTS
    n = (1 << 25) + 4097
    g = torch.Generator("cuda").manual_seed(52)
    src = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device="cuda", generator=g)
    for bit in (63, 55, 47, 39):
        coin = torch.randint(0, 2, (n,), dtype=torch.int64, device="cuda", generator=g)
        src.bitwise_or_(coin.mul_(1 << bit if bit < 63 else -(1 << 63)))
        del coin
    fp = V.fingerprint(src)
    t = torch.empty_like(src)
    wctx.set_option("regpart", 0)
    try:
        stats = []
        for early_plan, what in ((1, "warm-up (buffers grow once)"), (1, "early_plan=1"), (0, "early_plan=0")):
            wctx.set_option("early_plan", early_plan)
            t.copy_(src)
            wctx.sort_u64(t)
            stats.append(wctx.stats())
            V.assert_sorted_permutation(fp, t)
    finally:
        wctx.set_option("regpart", DEFAULTS["regpart"])
    _, st1, st0 = stats
    print(st1, st0)
    assert st1["rounds"] >= 5, st1
    assert 2 <= st1.get("rounds_planned_early", 0) < st1["rounds"], st1
    assert st1.get("bit_skip_restarts", 0) == 0, st1
    for key in PLAN_STATS:
        assert st1.get(key, 0) == st0.get(key, 0), (key, st1, st0)

"""CPU tests of tests/exact_verdict.py, the verifier behind the exact full-size GPU tests: its mix is splitmix64 bit for
bit, it accepts correct sorts of every layout at lengths around a chunk border, and it rejects the errors that order, sum
and xor let through."""
import numpy as np
import pytest
import torch

import exact_verdict as V

CHUNK = 1024
LENGTHS = [0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
KINDS = ["uniform", "zipf", "fewdistinct", "constant", "sorted", "reversed", "upperhalfzero"]
LAYOUTS = ["u32", "u64", "tuples"]


def mix_np(x):
    """the same finaliser restated on numpy uint64, where >> is logical and the arithmetic wraps"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def t(a):
    """unsigned numpy array -> the signed tensor of its width"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.int64).copy())


def make(rng, n, kind, bits):
    dt = np.uint32 if bits == 32 else np.uint64
    full = (1 << bits) - 1
    u = rng.integers(0, full, n, dtype=np.uint64, endpoint=True)
    if kind == "uniform":
        k = u
    elif kind == "zipf":
        k = np.minimum(rng.zipf(1.2, n).astype(np.float64), float(1 << 31)).astype(np.uint64)
        if bits == 64:
            k = k << np.uint64(32) | k
    elif kind == "fewdistinct":
        k = (u % np.uint64(7)) * np.uint64(0x2492492492492492 & full)      # (its top value has the sign bit set)
    elif kind == "constant":
        k = np.full(n, 0xDEADBEEFDEADBEEF & full, np.uint64)
    elif kind == "sorted":
        k = np.sort(u)
    elif kind == "reversed":
        k = np.sort(u)[::-1].copy()
    elif kind == "upperhalfzero":
        k = u >> np.uint64(bits // 2)
    else:
        raise ValueError(kind)
    return k.astype(dt)


def unstable_sort(rng, k):
    """a correct output of an unstable tuple sort with rids = iota: equal keys carry their rids in a shuffled order"""
    perm = rng.permutation(k.size)
    order = perm[np.argsort(k[perm], kind="stable")].astype(np.uint64)
    return k[order], order


def old_triple(a):
    """(order violations, sum mod 2^64, xor): what the full-size tests checked before this module"""
    a64 = a.astype(np.uint64)
    return V.order_violations(t(a), CHUNK), int(a64.sum(dtype=np.uint64)), int(np.bitwise_xor.reduce(a64)) if a.size else 0


def rejects(fp, keys, rids=None):
    with pytest.raises(AssertionError):
        V.assert_sorted_permutation(fp, keys, rids, chunk=CHUNK)
    return True


def test_constants_are_the_int64_forms():
    for signed, pattern in ((V._GAMMA, 0x9E3779B97F4A7C15), (V._MUL1, 0xBF58476D1CE4E5B9), (V._MUL2, 0x94D049BB133111EB)):
        assert signed & V.M64 == pattern and -(1 << 63) <= signed < 0


def test_mix_equals_numpy_uint64():
    rng = np.random.default_rng(1)
    x = rng.integers(0, (1 << 64) - 1, 1 << 20, dtype=np.uint64, endpoint=True)
    x[:3] = [0, (1 << 64) - 1, 1 << 63]
    src = t(x)
    keep = src.clone()
    got = V.mix(src).numpy().view(np.uint64)
    assert (got == mix_np(x)).all()
    assert torch.equal(src, keep)                                   # mix() leaves its argument alone
    assert int(got[0]) == 0xE220A8397B1DCDAF                        # splitmix64's first output from state 0
    assert np.unique(got).size == got.size == np.unique(x).size     # (a bijection: distinct in, distinct out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_accepts_correct_sorts(layout, kind):
    rng = np.random.default_rng(len(kind) * 7 + len(layout))
    for n in LENGTHS:
        k = make(rng, n, kind, 32 if layout == "u32" else 64)
        if layout == "tuples":
            r = np.arange(n, dtype=np.uint64)
            fp = V.fingerprint(t(k), t(r), chunk=CHUNK)
            ko, ro = unstable_sort(rng, k)
            assert (k[ro.astype(np.int64)] == ko).all()
            V.assert_sorted_permutation(fp, t(ko), t(ro), chunk=CHUNK)
        else:
            fp = V.fingerprint(t(k), chunk=CHUNK)
            V.assert_sorted_permutation(fp, t(np.sort(k)), chunk=CHUNK)
        assert fp[0] == n
        if n == 0:
            assert fp == (0, 0)


@pytest.mark.parametrize("bits", [32, 64])
def test_fingerprint_is_the_sum_of_mixed_values(bits):
    """the definition, restated in numpy -- and independent of the chunk length"""
    rng = np.random.default_rng(bits)
    k = make(rng, 3 * CHUNK + 5, "uniform", bits)
    want = int(mix_np(k.astype(np.uint64)).sum(dtype=np.uint64))
    for chunk in (CHUNK, 7, 1 << 26):
        assert V.fingerprint(t(k), chunk=chunk) == (k.size, want)
    r = rng.integers(0, (1 << 64) - 1, k.size, dtype=np.uint64, endpoint=True)
    with np.errstate(over="ignore"):
        want = int(mix_np(mix_np(k.astype(np.uint64)) + r).sum(dtype=np.uint64))
    assert V.fingerprint(t(k), t(r), chunk=CHUNK) == (k.size, want)
    assert V.key_sum(t(k), CHUNK) == int(k.astype(np.uint64).sum(dtype=np.uint64))


@pytest.mark.parametrize("bits", [32, 64])
def test_order_violations_counts_unsigned_and_across_chunks(bits):
    rng = np.random.default_rng(3)
    k = make(rng, 3 * CHUNK + 5, "uniform", bits)
    want = int((k[1:] < k[:-1]).sum())
    assert want > CHUNK and V.order_violations(t(k), CHUNK) == want == V.order_violations(t(k), 1 << 26)
    s = np.sort(k)
    assert s[-1] >> (bits - 1) == 1 and s[0] >> (bits - 1) == 0      # (both signs present: signed order would count one)
    assert V.order_violations(t(s), CHUNK) == 0
    s[CHUNK - 1], s[CHUNK] = s[CHUNK], s[CHUNK - 1]                  # the only violation sits on a chunk border
    assert V.order_violations(t(s), CHUNK) == 1


@pytest.mark.parametrize("bits", [32, 64])
def test_rejects_wrong_outputs(bits):
    rng = np.random.default_rng(bits + 1)
    n = 3 * CHUNK + 5
    dt = np.uint32 if bits == 32 else np.uint64
    k = np.unique(make(rng, 2 * n, "uniform", bits) >> dt(1))[:n]    # distinct, top bit clear
    assert k.size == n
    k = rng.permutation(k)
    fp = V.fingerprint(t(k), chunk=CHUNK)
    good = np.sort(k)
    V.assert_sorted_permutation(fp, t(good), chunk=CHUNK)

    bad = good.copy()                                                # two keys swapped across a chunk border
    bad[CHUNK - 1], bad[CHUNK] = good[CHUNK], good[CHUNK - 1]
    assert V.fingerprint(t(bad), chunk=CHUNK) == fp and rejects(fp, t(bad))

    bad = good.copy()                                                # one key overwritten by its neighbour
    bad[777] = good[778]
    assert V.order_violations(t(bad), CHUNK) == 0 and rejects(fp, t(bad))

    bad = good.copy()                                                # a high bit flipped in the last element
    bad[-1] ^= dt(1 << (bits - 1))
    assert V.order_violations(t(bad), CHUNK) == 0 and rejects(fp, t(bad))

    assert rejects(fp, t(good[:-1]))                                 # one element short
    assert rejects(fp, t(np.append(good, good[-1])))                 # and one too many


@pytest.mark.parametrize("bits", [32, 64])
def test_rejects_the_trade_that_order_sum_and_xor_accept(bits):
    """4k+1, 4k+2 -> 4k, 4k+3 between neighbours that keep the order: what a leaf that regenerates keys from counters
    and a prefix can produce.  The old triple cannot see it; that is why this module exists."""
    rng = np.random.default_rng(bits + 2)
    n = 3 * CHUNK + 5
    dt = np.uint32 if bits == 32 else np.uint64
    good = np.sort(make(rng, n, "uniform", bits) & dt(((1 << bits) - 1) & ~15))   # multiples of 16 ...
    i = CHUNK + 10
    assert good[i - 1] <= good[i] and good[i + 2] > good[i] + dt(3)
    good[i + 1] = good[i] + dt(2)                                                   # ... except the pair 4k+1, 4k+2
    good[i] += dt(1)
    fp = V.fingerprint(t(rng.permutation(good)), chunk=CHUNK)
    V.assert_sorted_permutation(fp, t(good), chunk=CHUNK)
    bad = good.copy()
    bad[i] -= dt(1)
    bad[i + 1] += dt(1)
    assert bad[i] % 4 == 0 and bad[i + 1] == bad[i] + dt(3)
    assert old_triple(bad) == old_triple(good) and old_triple(bad)[0] == 0
    assert rejects(fp, t(bad))


def test_rejects_a_sign_extended_u32():
    """4-byte keys count as their zero extension: the same values in 8-byte elements pass, a sign-extended one does not
    (as the largest key it keeps the order)."""
    rng = np.random.default_rng(5)
    k = make(rng, 3 * CHUNK + 5, "uniform", 32)
    fp = V.fingerprint(t(k), chunk=CHUNK)
    good = np.sort(k)
    assert good[-1] >> 31 == 1
    wide = good.astype(np.uint64)
    V.assert_sorted_permutation(fp, t(wide), chunk=CHUNK)
    wide[-1] |= np.uint64(0xFFFFFFFF00000000)
    assert V.order_violations(t(wide), CHUNK) == 0 and rejects(fp, t(wide))


def test_rejects_rids_exchanged_between_keys():
    rng = np.random.default_rng(6)
    n = 3 * CHUNK + 5
    k = make(rng, n, "uniform", 64)
    r = np.arange(n, dtype=np.uint64)
    fp = V.fingerprint(t(k), t(r), chunk=CHUNK)
    ko, ro = unstable_sort(rng, k)
    V.assert_sorted_permutation(fp, t(ko), t(ro), chunk=CHUNK)
    assert ko[100] != ko[2 * CHUNK + 1]
    bad = ro.copy()
    bad[100], bad[2 * CHUNK + 1] = ro[2 * CHUNK + 1], ro[100]        # keys right, rids a permutation, two tuples wrong
    assert V.fingerprint(t(ko), chunk=CHUNK) == V.fingerprint(t(k), chunk=CHUNK) and (np.sort(bad) == r).all()
    assert rejects(fp, t(ko), t(bad))
    assert rejects(fp, t(ko))                                        # (and a tuple fingerprint is not a key fingerprint)

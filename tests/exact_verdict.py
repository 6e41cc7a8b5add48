"""An exact verdict on a sort at any size, from plain torch alone (a helper module like gpu_support.py, not a test; it
imports nothing from the package under test and works on CPU and GPU tensors alike).

The argument.  "Ascending, and the same multiset as the input" is the definition of the sorted array: there is exactly
one such array, so an output that has both properties IS the right answer, bit for bit, without anybody having sorted
the input a second time.  For (key, rid) tuples the sort is unstable, and what it promises is "keys ascending, and the
same multiset of tuples": again both halves are checked here and nothing else is promised.
 - order: ``order_violations`` compares every neighbouring pair as unsigned numbers, chunk borders included.
 - multiset: ``fingerprint`` is (n, the sum mod 2^64 of a mixed value per element).  The mix is the splitmix64 finaliser,
   a bijection of 64-bit words with full avalanche, so unlike a plain sum or xor the fingerprint does not survive
   trading one pair of values for another (4k+1, 4k+2 -> 4k, 4k+3 keeps order, sum and xor), losing one value and
   doubling its neighbour, or moving a rid to another key.  A tuple is mixed as mix(mix(key) + rid): the inner mix
   ties the rid to its key, the outer one keeps (key, rid) pairs from trading places.
The only gap is a collision of two 64-bit sums of mixed values: about 2^-64 per comparison for any error that was not
built against this very hash.

How to use it: take the fingerprint of the input IN PLACE, before the sort; sort in place; then
``assert_sorted_permutation(fp, keys[, rids])``.  No clone of the input is needed, so a 2^32-key case costs the array and
one chunk's temporaries.  Nothing crosses to the host but scalars.

int32 / int64 tensors hold unsigned bit patterns, as everywhere in these tests; 4-byte elements are zero-extended, so a
u32 array and the u64 array of the same values have the same fingerprint."""
import torch

M64 = (1 << 64) - 1
# the constants of splitmix64 as the int64 values of their bit patterns (torch's int64 add and multiply wrap)
_GAMMA = -7046029254386353131    # 0x9E3779B97F4A7C15
_MUL1 = -4658895280553007687     # 0xBF58476D1CE4E5B9
_MUL2 = -7723592293110705685     # 0x94D049BB133111EB


def _xor_lsr_(x, a):
    """x ^= x >>> a, in place.  torch's >> on int64 is arithmetic: the sign copies are masked off, or the xor would lose
    the sign bit's information."""
    x.bitwise_xor_(torch.bitwise_right_shift(x, a).bitwise_and_((1 << (64 - a)) - 1))
    return x


def _mix_(x):
    x.add_(_GAMMA)
    _xor_lsr_(x, 30).mul_(_MUL1)
    _xor_lsr_(x, 27).mul_(_MUL2)
    return _xor_lsr_(x, 31)


def mix(x):
    """the splitmix64 finaliser (with its increment) of every element of an int64 tensor; a new tensor"""
    assert x.dtype == torch.int64
    return _mix_(x.clone())


def _wide(c):
    """a fresh int64 tensor of the chunk's unsigned values"""
    if c.dtype == torch.int64:
        return c.clone()
    assert c.dtype == torch.int32, c.dtype
    return c.to(torch.int64).bitwise_and_(0xFFFFFFFF)


def fingerprint(keys, rids=None, chunk=1 << 26):
    """(n, F): F = sum of mix(key) mod 2^64 for keys alone, sum of mix(mix(key) + rid) mod 2^64 for tuples.  Chunk by chunk:
    the temporaries are two or three int64 tensors of `chunk` elements, and nothing is copied to the host."""
    n = keys.numel()
    assert keys.dim() == 1 and (rids is None or (rids.dim() == 1 and rids.numel() == n))
    total = 0
    for a in range(0, n, chunk):
        m = _mix_(_wide(keys[a:a + chunk]))
        if rids is not None:
            r = rids[a:a + chunk]
            m.add_(r if r.dtype == torch.int64 else _wide(r))
            _mix_(m)
        total += int(m.sum().item())                  # (the int64 sum wraps: it is the sum mod 2^64, read as signed)
        del m
    return n, total & M64


def order_violations(keys, chunk=1 << 26):
    """the number of positions i with keys[i + 1] < keys[i] as unsigned numbers, chunk borders included"""
    n, viol, prev = keys.numel(), 0, None
    flip = -(1 << 63) if keys.dtype == torch.int64 else -(1 << 31)
    assert keys.dtype in (torch.int64, torch.int32), keys.dtype
    for a in range(0, n, chunk):
        u = keys[a:a + chunk] ^ flip                  # unsigned order as signed order
        viol += int((u[1:] < u[:-1]).sum().item())
        if prev is not None and int(u[0].item()) < prev:
            viol += 1
        prev = int(u[-1].item())
        del u
    return viol


def key_sum(keys, chunk=1 << 26):
    """the plain sum of the unsigned values mod 2^64 (what the library's own check reports; no evidence of a permutation)"""
    total = 0
    for a in range(0, keys.numel(), chunk):
        c = keys[a:a + chunk]
        total += int((c if c.dtype == torch.int64 else _wide(c)).sum().item())
    return total & M64


def mismatches(a, b, chunk=1 << 26):
    """the number of positions where two tensors of the same length differ"""
    assert a.numel() == b.numel()
    return sum(int((a[i:i + chunk] != b[i:i + chunk]).sum().item()) for i in range(0, a.numel(), chunk))


def assert_sorted_permutation(before_fp, keys, rids=None, chunk=1 << 26):
    """`keys` (with `rids`) is the sorted form of the array whose fingerprint -- taken before the sort -- is before_fp"""
    viol = order_violations(keys, chunk)
    assert viol == 0, f"{viol} order violations in {keys.numel()} keys"
    n, f = fingerprint(keys, rids, chunk)
    assert n == before_fp[0], f"{n} elements, {before_fp[0]} went in"
    assert f == before_fp[1], f"not the input's multiset: fingerprint {f:#018x}, the input's was {before_fp[1]:#018x}"

"""What msd_sort_rows has to produce, and the rows its tests feed it (a helper module like guardband.py, not a test); and
the numpy side of what the tests of every family share: the key types, the tables by key type and by width, the key codec
and the flat inputs.  The torch side is gpu_support.py.

The expectation is defined HERE: the keys' bit patterns become order-preserving unsigned codes with the numpy expressions of
this file, np.sort orders the codes along axis 1, the inverse map gives the sorted bit patterns, and descending is that
reversed along axis 1.  Floats are therefore in IEEE-754 totalOrder.

Plain module, no fixture: ``import sort_rows_expect`` (tests/ is on sys.path under pytest's default import mode)."""
import numpy as np

U32, I32, F32, U64, I64, F64 = range(6)
UT = {U32: np.uint32, I32: np.uint32, F32: np.uint32, U64: np.uint64, I64: np.uint64, F64: np.uint64}
NAMES = {U32: "u32", I32: "i32", F32: "f32", U64: "u64", I64: "i64", F64: "f64"}
# key type -> (unsigned view, typed view)
VIEWS = {U32: (np.uint32, np.uint32), I32: (np.uint32, np.int32), F32: (np.uint32, np.float32),
         U64: (np.uint64, np.uint64), I64: (np.uint64, np.int64), F64: (np.uint64, np.float64)}
# by element width in bytes
WIDTHS = (4, 8)
UW = {1: np.uint8, 4: np.uint32, 8: np.uint64}
UKT = {4: U32, 8: U64}              # the unsigned key type of a width: code == bits


def np_encode(bits, kt):
    ut = bits.dtype.type
    top = ut(1 << (bits.itemsize * 8 - 1))
    if kt % 3 == 0:
        return bits.copy()
    if kt % 3 == 1:
        return bits + top
    return np.where(bits & top, ~bits, bits | top)


def np_decode(codes, kt):
    ut = codes.dtype.type
    top = ut(1 << (codes.itemsize * 8 - 1))
    if kt % 3 == 0:
        return codes.copy()
    if kt % 3 == 1:
        return codes - top
    return np.where(codes & top, codes ^ top, ~codes)


def expected(bits, kt, descending=False):
    """every row of the bit patterns (rows x row_len) in the order of key type kt"""
    codes = np_encode(bits, kt)
    codes.sort(axis=1)
    out = np_decode(codes, kt)
    return np.ascontiguousarray(out[:, ::-1]) if descending else out


# ---- inputs: row r is a function of (seed + r, column), and of a scale of its own

def _splitmix(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def row_bits(rows, n, seed):
    """rows x n uint64: row r is the stream of the generator seeded with splitmix(seed + r)"""
    with np.errstate(over="ignore"):
        s = _splitmix(np.arange(rows, dtype=np.uint64) + np.uint64(seed))
        return _splitmix(s[:, None] + np.arange(n, dtype=np.uint64)[None, :])


def row_normal(rows, n, seed, tt):
    """N(0, scale_r^2): Box-Muller on the two halves of the row's bits, scale_r = 2^(r % 9 - 4)"""
    b = row_bits(rows, n, seed)
    u1 = ((b >> np.uint64(32)).astype(np.float64) + 1.0) / 4294967296.0
    u2 = (b & np.uint64(0xFFFFFFFF)).astype(np.float64) / 4294967296.0
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    scale = np.exp2((np.arange(rows) % 9) - 4.0)[:, None]
    return (z * scale).astype(tt)


def float_specials(tt):
    """both NaN signs with payloads, +-0, +-inf, denormals, the extremes"""
    i = np.finfo(tt)
    ut = np.uint32 if tt == np.float32 else np.uint64
    if tt == np.float32:
        nan_bits = [0x7FC00000, 0x7FC05555, 0x7F800001, 0x7F801234, 0x7FFFFFFF]
        sign = 0x80000000
    else:
        nan_bits = [0x7FF8 << 48, (0x7FF8 << 48) | 0x5555, (0x7FF << 52) | 1, (0x7FF << 52) | 0x1234, (1 << 63) - 1]
        sign = 1 << 63
    nans = np.array(nan_bits + [b | sign for b in nan_bits], dtype=ut).view(tt)
    den_min, den_max = np.array([1], ut).view(tt)[0], np.nextafter(i.tiny, tt(0), dtype=tt)
    vals = np.array([0.0, -0.0, np.inf, -np.inf, den_min, -den_min, den_max, -den_max, i.tiny, -i.tiny, i.max, -i.max], dtype=tt)
    return np.concatenate([nans, vals])


# kinds every key type has; "normal" and "specials" are float kinds, "extremes" an integer kind
COMMON_KINDS = ["bits", "const", "two", "sorted", "reverse", "lowbyte", "topbyte"]
FLOAT_KINDS = ["normal", "specials"] + COMMON_KINDS
INT_KINDS = ["extremes"] + COMMON_KINDS


def default_kind(kt):
    return "normal" if kt % 3 == 2 else "bits"


def make_rows(rows, n, kind, kt, seed):
    """rows x n bit patterns (unsigned view) of key type kt; every row has contents of its own"""
    ut = UT[kt]
    W = 32 if ut == np.uint32 else 64
    b = (row_bits(rows, n, seed) >> np.uint64(64 - W)).astype(ut)
    r = np.arange(rows, dtype=np.uint64)
    if kind == "bits":
        return b
    if kind == "const":      # all keys of a row equal (another value in every row)
        return np.repeat((ut(123456789) * (r.astype(ut) + ut(1)))[:, None], n, axis=1)
    if kind == "two":        # two values per row, one of them with the top bit
        lo = (ut(0x01234567) + r.astype(ut))[:, None]
        hi = (ut(1 << (W - 1)) | ut(0x00FEDCBA)) + r.astype(ut)[:, None]
        return np.where(b & ut(1), hi, lo).astype(ut)
    if kind == "lowbyte":    # only the low byte varies: one pass, every other digit is skipped
        return ((b & ut(0xFF)) | (ut(0x3C5A7700) + (r.astype(ut) << ut(8)))[:, None]).astype(ut)
    if kind == "topbyte":    # only the top byte varies
        return ((b & ut(0xFF << (W - 8))) | (ut(0x00123456) + r.astype(ut))[:, None]).astype(ut)
    if kind in ("sorted", "reverse"):
        src = make_rows(rows, n, default_kind(kt), kt, seed)
        s = expected(src, kt, descending=(kind == "reverse"))
        return s
    if kind == "extremes":
        top = 1 << (W - 1)
        table = np.array([top, top - 1, (1 << W) - 1, 0, 1, top + 1], dtype=ut)
        return table[(b % ut(len(table))).astype(np.int64)]
    tt = np.float32 if W == 32 else np.float64
    a = row_normal(rows, n, seed, tt)
    if kind == "specials":
        p = row_bits(rows, n, seed + 12345)
        sp = float_specials(tt)
        plant = (p % np.uint64(5)) == 0
        a = np.where(plant, sp[((p >> np.uint64(8)) % np.uint64(len(sp))).astype(np.int64)], a)
    elif kind != "normal":
        raise ValueError(kind)
    return np.ascontiguousarray(a).view(ut)


def seed_of(*xs):
    s = 17
    for x in xs:
        s = (s * 1000003 + int(x)) % (1 << 31)
    return s


# ---- flat inputs, as codes of an unsigned type (code == bits)

def top(kb):
    return (1 << (8 * kb)) - 1


def uniform(rng, count, kb, lo=0, hi=None):
    return rng.integers(lo, top(kb) if hi is None else hi, count, dtype=UW[kb], endpoint=True)


def special_bits(kt):
    ut = UT[kt]
    W = 8 * np.dtype(ut).itemsize
    if kt % 3 != 2:                                                 # integers: min, -1, 0, 1, max (as signed; as unsigned the same bits matter)
        return np.array([1 << (W - 1), (1 << W) - 1, 0, 1, (1 << (W - 1)) - 1], ut)
    if W == 32:
        sign, inf, q, s, den = 0x80000000, 0x7F800000, 0x7FC00000, 0x7F800001, 0x007FFFFF
    else:
        sign, inf, q, s, den = 1 << 63, 0x7FF << 52, 0x7FF8 << 48, (0x7FF << 52) | 1, (1 << 52) - 1
    pos = [0, 1, den, inf, q, q | 0x1234, s, s | 0x4320]           # zero, denormals, inf, quiet and signalling NaNs with two payloads each
    return np.array(pos + [p | sign for p in pos], ut)


# ---- flat typed inputs

def make_float(n, kind, tt, seed):
    rng = np.random.default_rng(seed)
    ut = np.uint32 if tt == np.float32 else np.uint64
    normal = lambda: rng.standard_normal(n).astype(tt)  # noqa: E731
    if kind == "normal":
        return normal()
    if kind == "bits":
        return rng.integers(0, np.iinfo(ut).max, n, dtype=ut, endpoint=True).view(tt)
    if kind == "specials":
        sp = np.repeat(float_specials(tt), 5)  # (a small n takes a random subset of them)
        a = np.concatenate([sp, rng.standard_normal(max(n - len(sp), 0)).astype(tt)])
        return np.ascontiguousarray(rng.permutation(a)[:n])
    if kind == "const":
        return np.full(n, -1.5, tt)
    if kind == "negative":
        return -(np.abs(normal()) + tt(1e-3))
    if kind == "sorted":
        return np.sort(normal())
    if kind == "reverse":
        return np.sort(normal())[::-1].copy()
    if kind == "coarse":
        return (np.round(normal() * 16) / 16).astype(tt)
    raise ValueError(kind)


def make_int(n, kind, tt, seed):
    rng = np.random.default_rng(seed)
    i = np.iinfo(tt)
    bits = lambda: rng.integers(i.min, i.max, n, dtype=tt, endpoint=True)  # noqa: E731
    if kind == "bits":
        return bits()
    if kind == "small":
        return rng.integers(-2048, 2048, n, dtype=tt)
    if kind == "const":
        return np.full(n, -123456789, tt)
    if kind == "extremes":
        return rng.choice(np.array([i.min, i.max, -1, 0], dtype=tt), n)
    if kind == "sorted":
        return np.sort(bits())
    if kind == "reverse":
        return np.sort(bits())[::-1].copy()
    raise ValueError(kind)


def check_positions(bits, values, positions):
    """positions (rows x n int64) beside values (rows x n bit patterns): every row's positions are a permutation of
    [0, n), and the input holds at each of them a key that is bit-equal to the value beside it"""
    rows, n = bits.shape
    assert positions.dtype == np.int64 and positions.shape == bits.shape
    assert ((positions >= 0) & (positions < n)).all(), "a position outside its row"
    assert (np.take_along_axis(bits, positions, axis=1) == values).all(), "a position does not hold the value written next to it"
    assert (np.sort(positions, axis=1) == np.arange(n, dtype=np.int64)[None, :]).all(), "a row's positions are not a permutation"

"""What the ABI tests of the families share (a helper module like guardband.py, not a test): reading a header, comparing
its declarations with the agreed argument lists, the binding's tables of exports, a context without a device and the
refusals of a limits call.  Every check asserts; the family's test calls it with its own header, table, words and signatures.

Plain module, no fixture: ``import abi_support`` (tests/ is on sys.path under pytest's default import mode)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def header(name):
    """(text, flat): include/<name> as it is, and without comments with all white space runs as one blank"""
    text = open(os.path.join(INCLUDE, name)).read()
    return text, re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def declared(flat):
    return re.findall(r"\bint (msd_\w+)\s*\(", flat)


def check_signatures(flat, signatures, exactly=True):
    """every function of `signatures` is declared with its argument list; `exactly`: and no other function is declared"""
    if exactly:
        assert sorted(declared(flat)) == sorted(signatures), declared(flat)
    for f, want in signatures.items():
        m = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % f, flat)
        assert m, f
        assert [a.strip() for a in m.group(1).split(",")] == want, f


def check_no_other_header_has(name, word, headers=None):
    """no header under include/ but `name` (or: none of `headers`) contains `word`, in a comment either"""
    for h in sorted(os.listdir(INCLUDE)) if headers is None else headers:
        if h != name:
            assert word not in open(os.path.join(INCLUDE, h)).read(), h


def check_exports(table, signatures, header_name, hpp):
    """the library exports every function, its argtypes are the ones of _lib.<table>, no other table of _lib lists it, and the
    build depends on the header and on the .hpp"""
    from inplacemsdradixsort_amd import _build, _lib
    L = _lib.load()
    own = getattr(_lib, table)
    assert sorted(own) == sorted(signatures)
    others = [getattr(_lib, t) for t in dir(_lib) if (t == "EXPORTS" or t.endswith("_EXPORTS")) and t != table]
    assert len(others) >= 11
    for f in signatures:
        assert hasattr(L, f), f
        assert not any(f in other for other in others), f
        assert getattr(L, f).argtypes is not None and list(getattr(L, f).argtypes) == list(own[f]), f
        assert len(own[f]) == len(signatures[f]), f
    assert any(d.endswith(header_name) for d in _build.DEPS)
    assert hpp in _build.DEPS


def bare_ctx():
    from inplacemsdradixsort_amd import MsdContext
    c = MsdContext.__new__(MsdContext)  # (no msd_create: there may be no GPU)
    c.device = 0
    return c


def check_limits_refusals(fn, outputs, bad_widths=(0, 2, 16, -4, 5)):
    """fn(width, *outputs): a bad width, and a null output with a good width, answer -1 and leave every output as it was"""
    cells = [C.c_uint64(77 + i) for i in range(outputs)]
    was = [c.value for c in cells]
    for width in bad_widths:
        assert fn(width, *[C.byref(c) for c in cells]) == -1 and [c.value for c in cells] == was, width
    for width in (4, 8):
        for null in range(outputs):
            assert fn(width, *[None if i == null else C.byref(c) for i, c in enumerate(cells)]) == -1 and [c.value for c in cells] == was, (width, null)
        assert fn(width, *[None] * outputs) == -1

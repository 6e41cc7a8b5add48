"""gpu_support.DEFAULTS against the source it restates: the names are those of msd_set_option's strcmp chain, the values
the initialisers of the same-named members of struct msd_ctx (csrc/msd_radix.hip), compared in both directions.  GPU test
files restore options on the session's context from that table; a default that moves in the library without moving
there (direct_min went from 2^26 to 2^22 once, and two fixtures kept "restoring" 2^26) fails here.  Needs no GPU."""
import os
import re

from gpu_support import DEFAULTS

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "inplacemsdradixsort_amd", "csrc", "msd_radix.hip")


def body(text, head):
    """the text between the line that starts with `head` and the first closing brace in column 0 behind it"""
    m = re.search(r"^" + re.escape(head) + r".*?^\}", text, re.S | re.M)
    assert m, head
    return m.group(0)


def c_int(expr):
    """a C integer initialiser such as `1`, `32` or `1ull << 22` as a number"""
    plain = re.sub(r"\b(\d+)[uUlL]+\b", r"\1", expr.strip())
    assert re.fullmatch(r"[\d\s<>()+*-]+", plain), expr
    return eval(plain, {"__builtins__": {}})


def source_defaults():
    text = open(SRC).read()
    names = re.findall(r'strcmp\(name, "(\w+)"\)', body(text, "int msd_set_option("))
    assert len(names) == len(set(names)) >= 19, names
    struct = body(text, "struct msd_ctx {")
    out = {}
    for name in names:
        m = re.findall(r"^\s*(?:int|uint64_t)\s+" + name + r"\s*=\s*([^;]+);", struct, re.M)
        assert len(m) == 1, f"option {name}: {len(m)} members of that name with an initialiser in struct msd_ctx"
        out[name] = c_int(m[0])
    return out


def test_the_parser_reads_c_initialisers():
    assert [c_int(s) for s in ("1", "0", "32", "1ull << 22", "1ull << 29", "(1u << 4) + 2")] == [1, 0, 32, 1 << 22, 1 << 29, 18]


def test_defaults_table_equals_the_source():
    src = source_defaults()
    assert sorted(set(src) - set(DEFAULTS)) == [], "options of msd_set_option that gpu_support.DEFAULTS does not have"
    assert sorted(set(DEFAULTS) - set(src)) == [], "names in gpu_support.DEFAULTS that msd_set_option does not take"
    assert {k: v for k, v in DEFAULTS.items() if src[k] != v} == {}, src
    assert src["direct_min"] == 1 << 22 and src["front_min"] == 1 << 29     # (the two that the size thresholds of tests/test_gpu_default_regimes.py stand on)

"""gpu_support.DEFAULTS and api.STAT_NAMES against the tables they restate (csrc/msd_options.hpp): tests/options_main.cpp
includes that header and nothing else of the project, a host compiler builds it, and it tries every rule at its edges and
prints both tables; the names and values are compared in both directions.  GPU test files restore options on the session's
context from DEFAULTS; a default that moves in the library without moving there (direct_min went from 2^26 to 2^22 once,
and two fixtures kept "restoring" 2^26) fails here.  Needs no GPU and no HIP toolchain."""
import os
import subprocess

import pytest

from gpu_support import DEFAULTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """({option: default}, [stat names]) as the program prints them; its own checks of the rules must hold"""
    exe = str(tmp_path_factory.mktemp("options") / "options")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "options_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    words = [line.split() for line in out.stdout.splitlines()]
    options = [(w[1], int(w[2])) for w in words if w[0] == "option"]
    stats = [w[1] for w in words if w[0] == "stat"]
    assert len(options) + len(stats) == len(words), out.stdout
    assert len(options) == len(dict(options)) >= 19, options
    return dict(options), stats


def test_defaults_table_equals_the_source(tables):
    src = tables[0]
    assert sorted(set(src) - set(DEFAULTS)) == [], "options of msd_set_option that gpu_support.DEFAULTS does not have"
    assert sorted(set(DEFAULTS) - set(src)) == [], "names in gpu_support.DEFAULTS that msd_set_option does not take"
    assert {k: v for k, v in DEFAULTS.items() if src[k] != v} == {}, src
    assert src["direct_min"] == 1 << 22 and src["front_min"] == 1 << 29     # (the two that the size thresholds of tests/test_gpu_default_regimes.py stand on)


def test_stat_names_of_the_wrapper_equal_the_source(tables):
    from inplacemsdradixsort_amd.api import STAT_NAMES
    stats = tables[1]
    assert len(stats) == len(set(stats)) and len(STAT_NAMES) == len(set(STAT_NAMES)), "a name twice"
    assert sorted(set(stats) - set(STAT_NAMES)) == [], "counters of msd_stat that MsdContext.stats() never asks for"
    assert sorted(set(STAT_NAMES) - set(stats)) == [], "names in api.STAT_NAMES that msd_stat does not know"

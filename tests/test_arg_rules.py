"""The argument rules of csrc/msd_args.hpp -- overlap, alignment, the extents of a matrix of rows, the width / flag / lanes
dispatch -- checked on the host: tests/arg_rules_main.cpp includes that header and nothing else of the project, a host compiler
builds it, and it exits with 0 if every rule holds.  Needs no GPU and no HIP toolchain."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rules_hold_on_a_host_compiler(tmp_path):
    exe = str(tmp_path / "arg_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "arg_rules_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr

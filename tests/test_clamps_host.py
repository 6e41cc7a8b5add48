"""The clamps of the merge path's index functions -- merge_tile_extent, lds_count, search_counts (csrc/msd_search.hpp) and
join_global_upper (csrc/msd_join.hpp) -- checked on the host: tests/clamp_main.hip includes the kernels' own headers, hipcc
builds it with the host's address and undefined-behaviour sanitizers, and it exits with 0 if every extent and every result
stays inside its array for inputs that are NOT ascending (every array is a heap block of exactly its length: a stray probe is
a sanitizer report).  Nothing is launched: needs no GPU.  The first of the three layers of DESIGN.md 10.13."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def test_the_clamps_hold_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "clamp_main")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "clamp_main.hip"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stdout + build.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 failed" in out.stdout, out.stdout

#!/usr/bin/env python3
"""Have the kernels of two builds of the library the same machine code?

    python tools/isa_diff.py OLD.so NEW.so

Takes the gfx950 code object out of each library (llvm-objcopy + clang-offload-bundler), disassembles it (llvm-objdump)
and compares the instruction text kernel by kernel (comments, which carry addresses, dropped).  Prints the kernels that
are missing, changed and added; exit status 1 if an old kernel is missing or changed.  An old kernel whose name is gone
but whose instruction text is that of exactly one added kernel (and of no other old kernel that is gone) counts as
renamed, not as missing.  Needs no GPU."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(lib, tmp):
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "code.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=" + TARGET, "--output=" + co])
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                          capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^<?([A-Za-z_0-9.$]+)>?:\s*$", line.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur:
            out[cur].append(re.sub(r"\s*//.*$", "", line.strip()))
    # A kernel ends at the s_endpgm that padding follows: the s_nop fill up to the next symbol's alignment -- and, behind
    # the last named kernel, whatever unnamed code comes next -- depends on the neighbours, not on the kernel.
    for v in out.values():
        for i in range(len(v) - 1):
            if v[i] == "s_endpgm" and v[i + 1] == "s_nop 0":
                del v[i + 1:]
                break
        while v and v[-1] == "":
            v.pop()
    return {k: hashlib.sha1("\n".join(v).encode()).hexdigest() for k, v in out.items() if v}


def main():
    old_lib, new_lib = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        old, new = kernels(old_lib, a), kernels(new_lib, b)
    missing = sorted(k for k in old if k not in new)
    changed = sorted(k for k in old if k in new and old[k] != new[k])
    added = sorted(k for k in new if k not in old)
    renamed = {}
    for k in missing:
        same = [a for a in added if new[a] == old[k]]
        if len(same) == 1 and sum(old[m] == old[k] for m in missing) == 1:
            renamed[k] = same[0]
    missing = [k for k in missing if k not in renamed]
    added = [a for a in added if a not in renamed.values()]
    print(f"{len(old)} kernels in {old_lib}, {len(new)} in {new_lib}")
    for title, names in (("missing", missing), ("changed", changed), ("added", added)):
        print(f"{title}: {len(names)}")
        for k in names:
            print("   ", k)
    print(f"renamed (same code): {len(renamed)}")
    for k in sorted(renamed):
        print("   ", k, "->", renamed[k])
    return 1 if missing or changed else 0


if __name__ == "__main__":
    sys.exit(main())

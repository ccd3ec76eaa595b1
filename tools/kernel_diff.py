#!/usr/bin/env python3
"""Compare two builds of the library kernel by kernel: the gfx950 disassembly with addresses and branch-target offsets dropped.
Prints "identical" or the two instruction counts per kernel (differing ones only with --diff-only), then the totals.

    python tools/kernel_diff.py OLD.so NEW.so [--diff-only]
"""
import collections, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin"

def kernels(so):
    """demangled symbol -> its instructions, position-independent"""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run([LLVM + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, tmp + "/fat.bin"], check=True)
        subprocess.run([LLVM + "/clang-offload-bundler", "--type=o", "--unbundle", "--input=" + tmp + "/fat.bin",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + tmp + "/k.co"], check=True)
        dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--demangle", "--no-show-raw-insn", tmp + "/k.co"], stdout=subprocess.PIPE, check=True).stdout.decode()
    out, cur = collections.OrderedDict(), None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = out.setdefault(re.sub(r"^void prt::", "", m.group(1)), [])
        elif cur is not None and line.strip():
            ins = re.sub(r"//.*$", "", line).strip()                       # the address
            ins = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<L>", ins)              # a branch target as symbol + offset ...
            cur.append(re.sub(r"^(s_c?branch\S*|s_call\S*)\s+\S+", r"\1 L", ins))   # ... and as a distance
    return out

if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = kernels(args[0]), kernels(args[1])
    same = [k for k in old if k in new and old[k] == new[k]]
    for k in sorted(set(old) | set(new)):
        if k in same:
            if "--diff-only" not in sys.argv: print("identical           %s" % k[:160])
        elif k in old and k in new:
            print("%6d -> %6d    %s" % (len(old[k]), len(new[k]), k[:160]))
        else:
            print("only in %s         %s" % ("OLD" if k in old else "NEW", k[:160]))
    print("%d kernels in OLD, %d in NEW: %d identical, %d differ or are in one only" % (len(old), len(new), len(same), len(set(old) | set(new)) - len(same)))

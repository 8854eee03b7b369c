#!/usr/bin/env python3
"""Per-kernel instruction count and hash of the gfx950 code objects in a directory of build.sh's objects (host only).

    tools/isa_table.py OBJ_DIR               symbol | instructions | sha1
    tools/isa_table.py PARENT_DIR NOW_DIR    symbol | instructions parent | instructions now | sha1 parent | sha1 now | same

For every .o: the fat binary section is dumped with llvm-objcopy, its gfx950 member unbundled with clang-offload-bundler
and disassembled with llvm-objdump -d; addresses and encodings are stripped and the remaining instruction text is hashed
per symbol.  With two directories the exit status is 1 if a symbol differs or the two sets of symbols differ: the check
that a change of source text left every kernel's machine code as it was.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name):
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    path = llvm if os.path.exists(llvm) else shutil.which(name)
    if not path:
        sys.exit("isa_table: %s not found (set ROCM_PATH)" % name)
    return path


def kernels(obj):
    """{symbol: (instructions, sha1[:12])} of the gfx950 member of one object; {} if it holds no device code."""
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
        dump = subprocess.run([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "copy.o")],
                              capture_output=True)
        if dump.returncode != 0 or not os.path.exists(fat):
            return {}
        subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat,
                        "--output=" + co], check=True)
        if os.path.getsize(co) == 0:
            return {}
        text = subprocess.run([tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    out, sym, lines = {}, None, []

    def close():
        if sym is not None:
            out[sym] = (len(lines), hashlib.sha1("\n".join(lines).encode()).hexdigest()[:12])

    for line in text.splitlines():
        head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if head:
            close()
            sym, lines = head.group(1), []
        elif sym is not None and line.startswith("\t"):
            ins = re.sub(r"\s*//.*$", "", line).strip()           # drop "// address: encoding"
            if ins != "...":   # objdump's mark for the zero padding up to the next symbol: there once another kernel follows
                lines.append(ins)
    close()
    return out


def objects(d):
    return sorted(f for f in os.listdir(d) if f.endswith(".o"))


def main(argv):
    if len(argv) == 2:
        for o in objects(argv[1]):
            k = kernels(os.path.join(argv[1], o))
            print("\n%s: %d symbols" % (o, len(k)))
            for s in sorted(k):
                print("%s | %d | %s" % (s, *k[s]))
        return 0
    if len(argv) != 3:
        sys.exit(__doc__)
    a_dir, b_dir = argv[1], argv[2]
    names = sorted(set(objects(a_dir)) | set(objects(b_dir)))
    rows, total, differing = [], 0, 0
    for o in names:
        a = kernels(os.path.join(a_dir, o)) if os.path.exists(os.path.join(a_dir, o)) else {}
        b = kernels(os.path.join(b_dir, o)) if os.path.exists(os.path.join(b_dir, o)) else {}
        rows.append("\n%s: %d symbols parent, %d now" % (o, len(a), len(b)))
        for s in sorted(set(a) | set(b)):
            ia, ha = a.get(s, ("-", "-"))
            ib, hb = b.get(s, ("-", "-"))
            same = s in a and s in b and a[s] == b[s]
            total += 1
            differing += not same
            rows.append("%s | %s | %s | %s | %s | %s" % (s, ia, ib, ha, hb, "yes" if same else "NO"))
    print("%d objects, %d kernel symbols, %s" % (len(names), total, "every one identical" if not differing else
                                                  "%d DIFFERING or on one side only" % differing))
    print("symbol | instructions parent | instructions now | sha1 parent | sha1 now | same")
    print("\n".join(rows))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

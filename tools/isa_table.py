#!/usr/bin/env python3
"""Per-kernel instruction count and hash of the gfx950 code objects in a directory of build.sh's objects (host only).

    tools/isa_table.py OBJ_DIR               symbol | instructions | sha1
    tools/isa_table.py PARENT_DIR NOW_DIR    symbol | instructions parent | instructions now | sha1 parent | sha1 now | same
    tools/isa_table.py --resources PARENT_DIR NOW_DIR    the same, then one line per differing symbol (below)
    tools/isa_table.py --by-symbol [--resources] PARENT_DIR NOW_DIR
        the two directories compared by kernel symbol across all their objects, for a change that moves kernels between
        files: symbol | object parent | object now | instructions | sha1 | same, with one line for each object whose symbols
        all stayed in it unchanged.  A symbol found in two objects of one side is reported and fails the comparison like a
        differing one.

For every .o: the fat binary section is dumped with llvm-objcopy, its gfx950 member unbundled with clang-offload-bundler
and disassembled with llvm-objdump -d; addresses and encodings are stripped and the remaining instruction text is hashed
per symbol.  With two directories the exit status is 1 if a symbol differs or the two sets of symbols differ: the check
that a change of source text left every kernel's machine code as it was.

--resources: for every symbol whose hash differs, the code object's metadata note (VGPR, AGPR and SGPR counts, LDS and scratch
bytes, spill counts) and the counts of matrix, LDS, global / buffer memory and barrier instructions, parent -> now where
they differ, and a verdict: "allocation only" when all of those are equal and the instruction count is within 1 % of the
parent's (registers renamed, independent instructions reordered, a wait more or less), "DIFFERENT" otherwise.  The table in
front of it and the exit status are the same with and without the option.
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


META = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "vgpr_spill_count", "sgpr_spill_count")
CLASSES = (("mfma", r"v_mfma"), ("lds", r"ds_"), ("vmem", r"(global|buffer|flat|scratch)_"), ("barrier", r"s_barrier"))


def metadata(co):
    """{symbol: {field of META: int}} from the AMDGPU metadata note of a code object."""
    text = subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(  - |    )\.(\w+):\s*(\S*)$", line)   # a kernel's own keys: its arguments are indented further
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == "name":
            out[m.group(3)] = cur
        elif m.group(2) in META:
            cur[m.group(2)] = int(m.group(3))
    return out


def kernels(obj, res=None):
    """{symbol: (instructions, sha1[:12])} of the gfx950 member of one object; {} if it holds no device code.
    With a dict `res`: res[symbol] = the symbol's metadata fields and instruction class counts."""
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
        meta = metadata(co) if res is not None else {}
    out, sym, lines = {}, None, []

    def close():
        if sym is not None:
            out[sym] = (len(lines), hashlib.sha1("\n".join(lines).encode()).hexdigest()[:12])
            if res is not None:
                res[sym] = dict(meta.get(sym, {}))
                for name, pat in CLASSES:
                    res[sym][name] = sum(1 for ins in lines if re.match(pat, ins))

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


def verdict(ia, ib, ra, rb):
    """One --resources line of a symbol that is on both sides with different hashes."""
    fields = META + tuple(name for name, _ in CLASSES)
    missing = [f for f in fields if f not in ra or f not in rb]
    moved = [f for f in fields if f not in missing and ra[f] != rb[f]]
    ok = not missing and not moved and abs(ib - ia) * 100 <= ia
    cells = ["%s %s" % (f, ra.get(f, "?")) if f not in moved and f not in missing else
             "%s %s -> %s" % (f, ra.get(f, "?"), rb.get(f, "?")) for f in fields]
    return "%s | instructions %+d (%+.2f %%) | %s" % ("allocation only" if ok else "DIFFERENT", ib - ia,
                                                    100.0 * (ib - ia) / ia, " | ".join(cells))


def by_symbol(a_dir, b_dir, resources):
    """Parent against now by kernel symbol, whichever object holds it: for a change that moves kernels between files."""
    sides, dup = [], []
    for d in (a_dir, b_dir):
        k, res, where = {}, {}, {}
        for o in objects(d):
            r = {} if resources else None
            for s, v in kernels(os.path.join(d, o), r).items():
                if s in k:
                    dup.append("%s | twice in %s: %s and %s" % (s, d, where[s], o))
                k[s], where[s] = v, o
                if resources:
                    res[s] = r[s]
        sides.append((k, res, where))
    (a, ra, wa), (b, rb, wb) = sides
    # an object whose symbols stayed where they were, every one identical, gets one line instead of a row per symbol
    names = set(wa.values()) | set(wb.values())
    quiet = {o for o in names if {s for s in a if wa[s] == o} == {s for s in b if wb[s] == o} and
             all(a[s] == b[s] for s in a if wa[s] == o)}
    rows, differing, detail = [], 0, []
    for o in sorted(quiet):
        rows.append("(%s: %d symbols, all in the same object on both sides and identical)" % (o, sum(1 for s in a if wa[s] == o)))
    for s in sorted(set(a) | set(b)):
        ia, ha = a.get(s, ("-", "-"))
        ib, hb = b.get(s, ("-", "-"))
        same = s in a and s in b and a[s] == b[s]
        differing += not same
        if wa.get(s) in quiet and wb.get(s) in quiet:
            continue
        rows.append("%s | %s | %s | %s | %s | %s | %s | %s" % (s, wa.get(s, "-"), wb.get(s, "-"), ia, ib, ha, hb, "yes" if same else "NO"))
        if resources and not same:
            one = ra.get(s) or rb.get(s) or {}
            detail.append("%s | %s" % (s, verdict(ia, ib, ra[s], rb[s]) if s in a and s in b else
                                       "DIFFERENT | on one side only (%s) | %s" % (
                                           "parent" if s in a else "now", " | ".join("%s %s" % kv for kv in one.items()))))
    print("%d objects parent, %d now, %d kernel symbols parent, %d now, %s%s" % (
        len(objects(a_dir)), len(objects(b_dir)), len(a), len(b),
        "every one identical" if not differing else "%d DIFFERING or on one side only" % differing,
        ", %d in two objects of one side" % len(dup) if dup else ""))
    print("symbol | object parent | object now | instructions parent | instructions now | sha1 parent | sha1 now | same")
    print("\n".join(rows))
    if dup:
        print("\nsymbols in two objects of one side:")
        print("\n".join(dup))
    if resources:
        print("\nresources of the %d differing symbols: verdict | instructions now - parent | metadata and instruction classes"
              % len(detail))
        print("\n".join(detail))
    return 1 if differing or dup else 0


def main(argv):
    resources = "--resources" in argv
    symbols = "--by-symbol" in argv
    argv = [a for a in argv if a not in ("--resources", "--by-symbol")]
    if symbols:
        if len(argv) != 3:
            sys.exit(__doc__)
        return by_symbol(argv[1], argv[2], resources)
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
    rows, total, differing, detail = [], 0, 0, []
    for o in names:
        ra, rb = ({}, {}) if resources else (None, None)
        a = kernels(os.path.join(a_dir, o), ra) if os.path.exists(os.path.join(a_dir, o)) else {}
        b = kernels(os.path.join(b_dir, o), rb) if os.path.exists(os.path.join(b_dir, o)) else {}
        rows.append("\n%s: %d symbols parent, %d now" % (o, len(a), len(b)))
        for s in sorted(set(a) | set(b)):
            ia, ha = a.get(s, ("-", "-"))
            ib, hb = b.get(s, ("-", "-"))
            same = s in a and s in b and a[s] == b[s]
            total += 1
            differing += not same
            rows.append("%s | %s | %s | %s | %s | %s" % (s, ia, ib, ha, hb, "yes" if same else "NO"))
            if resources and not same:
                one = ra.get(s) or rb.get(s) or {}
                detail.append("%s | %s" % (s, verdict(ia, ib, ra[s], rb[s]) if s in a and s in b else
                                           "DIFFERENT | on one side only (%s) | %s" % (
                                               "parent" if s in a else "now", " | ".join("%s %s" % kv for kv in one.items()))))
    print("%d objects, %d kernel symbols, %s" % (len(names), total, "every one identical" if not differing else
                                                  "%d DIFFERING or on one side only" % differing))
    print("symbol | instructions parent | instructions now | sha1 parent | sha1 now | same")
    print("\n".join(rows))
    if resources:
        print("\nresources of the %d differing symbols: verdict | instructions now - parent | metadata and instruction classes"
              % len(detail))
        print("\n".join(detail))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

#!/usr/bin/env python3
"""Is the device code of two builds the same?  compare_device_code.py LIB_A LIB_B [--arch gfx950] [--by-symbol [--renamed OLD=NEW]]

LIB_A / LIB_B: two gpslam_amd/lib directories (obj/*.o and libgpslam_hip.so, as `python -m gpslam_amd.build` leaves them).
Per object: the gfx950 code object is taken out of .hip_fatbin, and every kernel is compared by name, by the bytes of its code and
by its metadata (registers, LDS, scratch: the amdhsa.kernels note).  Per symbol, not per file: the order of instantiation moves
with the host code.  --by-symbol: kernels may move between objects (a refactor that gives a feature a translation unit of its own) --
every kernel of the whole library is compared by name whichever object holds it, a kernel may neither appear nor vanish, and the
moves are listed (kernel count per pair of object sets); --renamed OLD=NEW says that LIB_A's kernel OLD is LIB_B's NEW (a template
that became a plain kernel: same code, same metadata but for the name).  Also compares the C ABI (the exported gpslam_hip_* symbols) of the two libraries.  Exit status 1 on any difference.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM_LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def tool(name):
    p = os.path.join(ROCM_LLVM, name)
    return p if os.path.exists(p) else name


def kernels(obj, arch, tmp):
    """{kernel name: (sha256 of its code, its metadata block)} of one host object"""
    base = os.path.join(tmp, os.path.basename(obj))
    run(tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, base + ".fatbin")
    run(tool("clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + arch, "--input=" + base + ".fatbin",
        "--output=" + base + ".co", "--unbundle")
    text = None
    for line in run(tool("llvm-readelf"), "-SW", base + ".co").splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text = (int(m.group(1), 16), int(m.group(2), 16))
    blob = open(base + ".co", "rb").read()
    code = {}
    for line in run(tool("llvm-readelf"), "-sW", base + ".co").splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            addr, size = int(f[1], 16), int(f[2])
            off = text[1] + addr - text[0]
            code[f[7]] = hashlib.sha256(blob[off:off + size]).hexdigest()
    meta = {}
    notes = run(tool("llvm-readelf"), "--notes", base + ".co")
    for block in re.split(r"\n\s*- \.agpr_count", notes)[1:]:
        block = re.split(r"\n\s*amdhsa\.", block)[0]      # (the last kernel's block runs on into the tail of the note)
        name = re.search(r"\.name:\s+(\S+)", block)
        body = "\n".join(l.strip() for l in block.splitlines() if not l.strip().startswith("amdhsa.") and "---" not in l)
        meta[name.group(1)] = body.split("amdhsa.target")[0]
    return {k: (v, meta.get(k, "")) for k, v in code.items()}


def by_symbol(a, ta, tb):
    """whole library, per kernel: {name: {object: (code, metadata)}} of both builds; returns the number of differences"""
    bad = 0
    libs = []
    for d, tmp in ((a.lib_a, ta), (a.lib_b, tb)):
        per = {}
        for o in sorted(f for f in os.listdir(os.path.join(d, "obj")) if f.endswith(".o")):
            ks = kernels(os.path.join(d, "obj", o), a.arch, tmp)
            print("%s %-18s %4d kernels" % ("A" if d == a.lib_a else "B", o, len(ks)))
            for k, v in ks.items():
                per.setdefault(k, {})[o] = v
        libs.append(per)
    la, lb = libs
    for old, new in (r.split("=") for r in a.renamed):      # compared, code and metadata, under its new name
        la[new] = {o: (code, meta.replace(old, new)) for o, (code, meta) in la.pop(old).items()}      # (.name and .symbol carry it)
        print("renamed: %s -> %s" % (old, new))
    moves = {}
    for k in sorted(set(la) | set(lb)):
        if k not in la or k not in lb:
            print("%s only in %s (%s)" % (k, "A" if k in la else "B", ", ".join(sorted((la if k in la else lb)[k]))))
            bad += 1
            continue
        va, vb = set(la[k].values()), set(lb[k].values())
        if len(va) > 1 or len(vb) > 1:
            print("%s: its copies differ inside one library" % k)
            bad += 1
        elif {v[0] for v in va} != {v[0] for v in vb}:
            print("%s: code differs" % k)
            bad += 1
        elif va != vb:
            print("%s: metadata differs" % k)
            bad += 1
        oa, ob = tuple(sorted(la[k])), tuple(sorted(lb[k]))
        if oa != ob:
            moves.setdefault((oa, ob), []).append(k)
    for (oa, ob), ks in sorted(moves.items()):
        print("%4d kernels moved: %s -> %s" % (len(ks), " + ".join(oa), " + ".join(ob)))
        if a.verbose:
            for k in ks:
                print("       " + k)
    print("%d kernel names in A, %d in B" % (len(la), len(lb)))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--by-symbol", action="store_true", help="whole library, per kernel: kernels may have moved between objects")
    ap.add_argument("--verbose", action="store_true", help="--by-symbol: name the kernels that moved")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW", help="--by-symbol: kernel OLD of LIB_A is kernel NEW of LIB_B (mangled names)")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        objs = [] if a.by_symbol else sorted(f for f in os.listdir(os.path.join(a.lib_a, "obj")) if f.endswith(".o"))
        if a.by_symbol:
            bad += by_symbol(a, ta, tb)
        elif objs != sorted(f for f in os.listdir(os.path.join(a.lib_b, "obj")) if f.endswith(".o")):
            print("different sets of objects")
            bad += 1
        for o in objs:
            ka, kb = kernels(os.path.join(a.lib_a, "obj", o), a.arch, ta), kernels(os.path.join(a.lib_b, "obj", o), a.arch, tb)
            for k in sorted(set(ka) | set(kb)):
                if k not in ka or k not in kb:
                    print("%s: %s only in %s" % (o, k, "A" if k in ka else "B"))
                    bad += 1
                elif ka[k][0] != kb[k][0]:
                    print("%s: %s: code differs" % (o, k))
                    bad += 1
                elif ka[k][1] != kb[k][1]:
                    print("%s: %s: metadata differs" % (o, k))
                    bad += 1
            print("%-16s %4d kernels in A, %4d in B" % (o, len(ka), len(kb)))
    sym = [sorted(l.split()[-1] for l in run("nm", "-D", "--defined-only", os.path.join(d, "libgpslam_hip.so")).splitlines() if l.split()[-1].startswith("gpslam_hip_"))
           for d in (a.lib_a, a.lib_b)]
    if sym[0] != sym[1]:
        print("exported symbols differ:", sorted(set(sym[0]) ^ set(sym[1])))
        bad += 1
    print("%d exported gpslam_hip_* symbols in A, %d in B" % (len(sym[0]), len(sym[1])))
    print("IDENTICAL" if not bad else "%d DIFFERENCES" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

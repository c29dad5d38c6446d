#!/usr/bin/env python3
"""Which kernel sits in which object, and is it the same kernel?  No GPU needed.

   python scripts/code_objects.py OBJ_DIR                 one JSON record per kernel of every *.o in OBJ_DIR (gpslam_amd/lib/obj)
   python scripts/code_objects.py --compare OBJ_A OBJ_B   exit status 1 if a kernel of A is missing from B or a record differs

Each object's gfx950 code object is taken out of its .hip_fatbin section (llvm-objcopy, clang-offload-bundler); a record is the
object, the kernel's mangled name, the sha256 of its code bytes and its descriptor's metadata (the amdhsa.kernels note: VGPRs,
SGPRs, AGPRs, scratch bytes, LDS bytes, kernarg size, workgroup size).  --compare goes by kernel name, whichever objects hold it: the
kernels whose records differ, the kernels of A that B lacks, and per kernel the number of objects that hold it in A and in B.  Where
only the code bytes differ, both copies are disassembled (llvm-objdump) and compared with the addresses stripped: a kernel that moved
to another code object sits at another offset, so the literals of its pc-relative address computations may differ -- the report says
whether that is all, or an instruction differs.  The tools are the ones next to hipcc (ROCM_LLVM, default /opt/rocm/llvm/bin).
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROCM_LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
ARCH = "gfx950"
FIELDS = {"vgprs": ".vgpr_count", "sgprs": ".sgpr_count", "agprs": ".agpr_count", "scratch_bytes": ".private_segment_fixed_size",
          "lds_bytes": ".group_segment_fixed_size", "kernarg_bytes": ".kernarg_segment_size", "workgroup_size": ".max_flat_workgroup_size"}


def run(name, *args):
    return subprocess.run([os.path.join(ROCM_LLVM, name)] + list(args), check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """the gfx950 code object of a host object, as a file under tmp"""
    base = os.path.join(tmp, os.path.basename(obj))
    run("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, base + ".fatbin")
    run("clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + ARCH, "--input=" + base + ".fatbin", "--output=" + base + ".co", "--unbundle")
    return base + ".co"


def records(obj, tmp):
    """one record per kernel of a host object"""
    co = code_object(obj, tmp)
    with open(co, "rb") as f:
        blob = f.read()
    text = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", run("llvm-readelf", "-SW", co))
    addr0, off0 = int(text.group(1), 16), int(text.group(2), 16)
    code = {}
    for line in run("llvm-readelf", "-sW", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            off = off0 + int(f[1], 16) - addr0
            code[f[7]] = hashlib.sha256(blob[off:off + int(f[2])]).hexdigest()
    out = []
    for block in re.split(r"\n\s*- \.agpr_count", "\n" + run("llvm-readelf", "--notes", co))[1:]:
        block = ".agpr_count" + re.split(r"\n\s*amdhsa\.", block)[0]      # (the last kernel's block runs on into the tail of the note)
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        rec = {"object": os.path.basename(obj), "kernel": name, "code_sha256": code[name]}
        for key, field in FIELDS.items():
            rec[key] = int(re.search(re.escape(field) + r":\s+(\d+)", block).group(1))
        out.append(rec)
    return out


def dump(objdir, tmp):
    return [r for o in sorted(os.listdir(objdir)) if o.endswith(".o") for r in records(os.path.join(objdir, o), tmp)]


def disassembly(obj, kernel, tmp):
    """the instructions of a kernel of an object records() has unbundled into tmp, one per line, without addresses and encodings"""
    text = run("llvm-objdump", "-d", "--disassemble-symbols=" + kernel, os.path.join(tmp, obj + ".co"))
    return [l.split("//")[0].strip() for l in text.splitlines() if "//" in l]


PCREL = re.compile(r"(s_(?:add|addc|sub|subb)_u32 s\d+, s\d+, )(?:0x[0-9a-f]+|-?\d+)$")


def code_difference(a, b):
    """what differs between two disassemblies: nothing, the literals of pc-relative address computations only, or an instruction"""
    if len(a) != len(b):
        return "instructions differ (%d against %d)" % (len(a), len(b))
    n = 0
    for x, y in zip(a, b):
        if x != y:
            mx, my = PCREL.match(x), PCREL.match(y)
            if not mx or not my or mx.group(1) != my.group(1):
                return "an instruction differs: '%s' against '%s'" % (x, y)
            n += 1
    return "%d pc-relative literals differ, every instruction is the same" % n if n else "the bytes differ, the disassembly does not"


def compare(dir_a, dir_b):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        by = []
        for d, tmp in ((dir_a, ta), (dir_b, tb)):
            per = {}
            for r in dump(d, tmp):
                per.setdefault(r["kernel"], []).append(r)
            by.append(per)
        A, B = by
        bad = 0
        for k in sorted(A):
            if k not in B:
                print("absent from B: %s (A: %s)" % (k, ", ".join(r["object"] for r in A[k])))
                bad += 1
                continue
            strip = lambda r: {f: v for f, v in r.items() if f != "object"}
            forms = [strip(r) for r in A[k] + B[k]]
            if all(f == forms[0] for f in forms):
                continue
            bad += 1
            ra, rb = next((x, y) for x in A[k] for y in B[k] if strip(x) != strip(y))
            fields = [f for f in strip(ra) if ra[f] != rb[f]]
            why = ""
            if fields == ["code_sha256"]:
                why = ": " + code_difference(disassembly(ra["object"], k, ta), disassembly(rb["object"], k, tb))
            print("differs: %s (%s; A %s, B %s)%s" % (k, ", ".join("%s %s -> %s" % (f, ra[f], rb[f]) for f in fields if f != "code_sha256") or "code", ra["object"], rb["object"], why))
        copies = {}
        for k in sorted(set(A) | set(B)):
            copies.setdefault((len(A.get(k, [])), len(B.get(k, []))), []).append(k)
        for (na, nb), ks in sorted(copies.items()):
            print("%4d kernels in %2d objects of A and %2d of B%s" % (len(ks), na, nb, "" if na == nb else ": " + ", ".join(ks[:3]) + (" ..." if len(ks) > 3 else "")))
        for k in sorted(set(A) | set(B)):
            if len(A.get(k, [])) != len(B.get(k, [])):
                print("  %2d -> %2d  %s" % (len(A.get(k, [])), len(B.get(k, [])), k))
        print("%d kernels in A, %d in B; %d of A absent from B or different" % (len(A), len(B), bad))
        return 1 if bad else 0


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        for r in dump(sys.argv[1], tmp):
            print(json.dumps(r))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Builds gpslam_amd/lib/libgpslam_hip.so (hand-written HIP for gfx950) with hipcc.

hipcc cross-compiles for gfx950 without a GPU present, so this runs in the CPU-only container as well;
the built .so is git-ignored but travels to the GPU box with the repo snapshot.

What a translation unit is made from is what the compiler says it read: every compile writes a depfile (-MD -MF), the project files
in it are recorded next to the object (<object>.deps), and that list -- with the contents of its files, this file and the flags --
is what decides whether the object, and the library linked from the objects, is current.  No table of headers is kept by hand.
"""
import fcntl
import hashlib
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libgpslam_hip.so")
# one object each, compiled side by side, linked into the one library: the C ABI, the fp64-row and the fp32-row half of the
# optimiser (both are api_impl.inc -- launchers, compile() -- followed by api_iterate.inc -- the iteration driver; round 3: they
# were one 3.5-minute translation unit), the upper solver levels, the marginals (gtsam::Marginals: selected inversion of the chain)
# and their closure term on handles in column passes (marginals_clo.hip), the marginals of the segmented landmark path
# (marginals_fs.hip: fp64 only), the loop closures' launches (closures.hip: fp64 only), and fixed-lag smoothing (fixedlag.hip: state
# Gaussians, the head's marginalisation; fp64 only), the marginals of any two states with the closure gate (marginals_pairs.hip),
# Powell's dogleg optimiser (dogleg.hip: fp64 only; its C declarations are include/gpslam_hip_dogleg.h), and log det H with the
# Laplace log-evidence (evidence.hip: fp64 only; include/gpslam_hip_evidence.h), learning Qc from the marginals (qc_learn.hip: fp64
# only; include/gpslam_hip_qc.h), posterior sampling by perturbed solves (sampling.hip: fp64 only; include/gpslam_hip_sampling.h),
# learning measurement noise from the marginals (meas_noise.hip: fp64 only; include/gpslam_hip_noise.h),
# and the level-0 row and fused kernels with their launchers (level0.hip: the only unit that includes level0.hpp, so every form of
# k_fused_level0, k_chunk_forward_rows and k_chunk_backward_rows is compiled once), and the segmented landmark elimination with
# compile()'s plan for it (fatsep.hip: the only unit that includes fatsep.hpp, so every k_fs_* / k_fat_* kernel is compiled there, with
# fp64 and with fp32 rows; the other units see fatsep_plan.hpp, the plan without a kernel).
# A unit holds the kernels its own launch statements name; a header that launches none costs its includers no device code.
SOURCES = ["api.hip", "api_impl64.hip", "api_impl32.hip", "level0.hip", "upper.hip", "marginals.hip", "marginals_clo.hip", "marginals_fs.hip", "closures.hip", "fixedlag.hip", "marginals_pairs.hip",
           "dogleg.hip", "evidence.hip", "qc_learn.hip", "sampling.hip", "meas_noise.hip", "fatsep.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast"]
# where a translation unit's project files live: read and hashed BEFORE hipcc starts (a unit that reads a project file from anywhere
# else is refused: its contents as of the start of the compile are not known)
TREES = [CSRC, os.path.join(ROOT, "include")]


def _variant(extra):
    """Ablation / A-B builds (GPSLAM_HIPCC_FLAGS=-DGPS_ABLATE_*: results wrong on purpose) never share file names with the
    product build: their objects and library are keyed by a hash of the extra flags."""
    if not extra:
        return ""
    return "_" + hashlib.sha1(" ".join(extra).encode()).hexdigest()[:10]


def _paths(extra):
    tag = _variant(extra)
    return os.path.join(LIBDIR, "obj" + tag), os.path.join(LIBDIR, "libgpslam_hip%s.so" % tag)


OBJDIR = _paths([])[0]


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP library cannot be built (there is no CPU fallback)")


def _obj(src, objdir=None):
    return os.path.join(objdir or OBJDIR, os.path.splitext(src)[0] + ".o")


def read_depfile(text, cwd=CSRC, root=ROOT):
    """The project files a make-style depfile names as prerequisites: paths under `root`, relative to it and normalised
    (csrc/../../include/x.h is include/x.h), sorted, each once.  Relative names are relative to `cwd`, the compiler's working
    directory.  Everything outside `root` -- system and ROCm headers -- is dropped."""
    found = set()
    for rule in text.replace("\\\n", " ").splitlines():
        if ":" not in rule:
            continue
        for tok in re.findall(r"(?:\\.|\S)+", rule.split(":", 1)[1]):
            rel = os.path.relpath(os.path.normpath(os.path.join(cwd, tok.replace("\\ ", " "))), root)
            if not rel.startswith(os.pardir + os.sep) and rel != os.pardir:
                found.add(rel)
    return sorted(found)


class _Hashes(dict):
    """sha256 of a project file's contents by its path relative to the repository, read at first use (OSError if it is gone)"""
    def __missing__(self, rel):
        with open(os.path.join(ROOT, rel), "rb") as f:
            self[rel] = hashlib.sha256(f.read()).hexdigest()
        return self[rel]


def _snapshot():
    """every file a translation unit may be made from (TREES and this file), hashed now"""
    snap = _Hashes()
    for tree in TREES:
        for d, _dirs, files in os.walk(tree):
            for f in files:
                snap[os.path.relpath(os.path.join(d, f), ROOT)]
    snap[os.path.relpath(os.path.abspath(__file__), ROOT)]
    return snap


def _deps(obj):
    """the project files the compiler read for this object as the last compile recorded them, or None"""
    try:
        with open(obj + ".deps") as f:
            return f.read().split("\n")[:-1]
    except OSError:
        return None


def _digest(extra, deps, hashes):
    """Content hash of everything one object is made from: the recorded list of the files the compiler read and their contents
    (`hashes`), this file (the flags live here) and the extra flags; None without a list, or when a file of it is gone.  Round 5:
    modification times are not evidence -- an edit made WHILE hipcc runs leaves a library newer than every source and built from
    none of them (it happened), and a `touch` makes a stale one look fresh."""
    if deps is None:
        return None
    h = hashlib.sha256(" ".join(FLAGS + list(extra)).encode())
    try:
        for d in deps + [os.path.relpath(os.path.abspath(__file__), ROOT)]:
            h.update(b"\0" + d.encode() + b"\0" + hashes[d].encode())
    except OSError:
        return None
    return h.hexdigest()


def _recorded(path):
    try:
        with open(path + ".srchash") as f:
            return f.read().strip()
    except OSError:
        return None


def _record(path, text, suffix=".srchash"):
    tmp = path + suffix + ".tmp%d" % os.getpid()
    with open(tmp, "w") as f:
        f.write(text + "\n")
    os.replace(tmp, path + suffix)


def _lib_digest(digests):
    return None if None in digests else hashlib.sha256("".join(digests).encode()).hexdigest()


def up_to_date(extra=()):
    """True when the library on disk was linked from objects compiled from exactly the current sources and flags (the
    digests are written next to the outputs, taken from the file contents read BEFORE the compiler starts).  Reads and hashes
    the recorded lists' files; starts no compiler."""
    extra = list(extra)
    objdir, lib = _paths(extra)
    hashes = _Hashes()
    want = _lib_digest([_digest(extra, _deps(_obj(s, objdir)), hashes) for s in SOURCES])
    return os.path.exists(lib) and want is not None and _recorded(lib) == want


def build(force=False, verbose=False, extra=None):
    """Returns the path of the library.  Several processes may call this at once (pytest children, one rank per GPU): the
    build runs under a file lock, every output is written to a temporary name and renamed into place."""
    if extra is None:
        extra = os.environ.get("GPSLAM_HIPCC_FLAGS", "").split()   # A/B builds of kernel variants under their own file names
    objdir, lib = _paths(extra)
    if not force and up_to_date(extra):
        return lib
    os.makedirs(objdir, exist_ok=True)
    with open(os.path.join(LIBDIR, ".build.lock"), "a") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and up_to_date(extra):        # another process built it while this one waited
            return lib
        snap = _snapshot()      # the contents as they are NOW, before hipcc reads them
        digests = {}
        procs = []
        for src in SOURCES:
            obj = _obj(src, objdir)
            digests[src] = _digest(extra, _deps(obj), snap)
            if not force and os.path.exists(obj) and digests[src] is not None and _recorded(obj) == digests[src]:
                continue
            tmp = obj + ".tmp%d" % os.getpid()
            cmd = [_hipcc()] + FLAGS + list(extra) + ["-MD", "-MF", tmp + ".d", "-c", os.path.join(CSRC, src), "-o", tmp]
            if verbose:
                print(" ".join(cmd))
            procs.append((cmd, tmp, obj, src, subprocess.Popen(cmd, cwd=CSRC)))
        failed = None
        for cmd, tmp, final, src, p in procs:
            rc, deps = p.wait(), None
            if rc == 0:
                with open(tmp + ".d") as f:
                    deps = read_depfile(f.read())
            for leftover in [tmp + ".d"] + ([tmp] if rc != 0 else []):
                if os.path.exists(leftover):
                    os.remove(leftover)
            if rc != 0:
                failed = failed or subprocess.CalledProcessError(rc, cmd)
                continue
            now = _Hashes()
            outside = [d for d in deps if d not in snap]
            if outside or any(now[d] != snap[d] for d in deps):
                # the source changed under the compiler: the object is of neither version for sure -- drop it, build again
                os.remove(tmp)
                failed = failed or RuntimeError(
                    "%s reads %s, outside the directories build.py hashes before a compile (TREES)" % (src, ", ".join(outside)) if outside else
                    "%s (or a header it includes) was edited while it was being compiled; run the build again" % src)
                continue
            digests[src] = _digest(extra, deps, snap)
            os.replace(tmp, final)
            _record(final, "\n".join(deps), ".deps")
            _record(final, digests[src])
        if failed:
            raise failed
        tmp = lib + ".tmp%d" % os.getpid()
        link = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + [_obj(s, objdir) for s in SOURCES] + ["-o", tmp]
        if verbose:
            print(" ".join(link))
        subprocess.check_call(link, cwd=CSRC)
        os.replace(tmp, lib)
        _record(lib, _lib_digest([digests[s] for s in SOURCES]))
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))

"""Posterior sampling's interface without a device (include/gpslam_hip_sampling.h): the symbols exist in the library, the header and
the binding's own list, ABI 2.4 and gpslam_hip.h are untouched, the NULL-handle and argument answers, and samplePosterior of
gpslam_amd/host/gpslam_host.hpp (tests/cpp/posterior_host_tests.cpp) compiles with -Wall -Werror and links.  On the GPU the C++ draw
of a small Pose2 graph equals the Python binding's on the same numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(r"\b(gpslam_hip_[a-z0-9_]+)\s*\(", f.read())))


def test_symbols_exist_in_the_library_the_header_and_the_binding():
    lib = gp.load_library()
    assert _declared("gpslam_hip_sampling.h") == sorted(chain.SAMPLING_SYMBOLS)
    assert len(chain.SAMPLING_SYMBOLS) == 3
    for name in chain.SAMPLING_SYMBOLS:
        assert hasattr(lib, name), name
        assert name not in chain.ABI_SYMBOLS + chain.DOGLEG_SYMBOLS + chain.EVIDENCE_SYMBOLS + chain.QC_SYMBOLS
    for name in ("posterior_noise_dim", "posterior_noise", "sample_posterior"):
        assert callable(getattr(gp.ChainSolver, name))


def test_abi_and_the_old_header_are_untouched():
    lib = gp.load_library()
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    assert _declared("gpslam_hip.h") == sorted(chain.ABI_SYMBOLS)
    with open(os.path.join(ROOT, "include", "gpslam_hip.h")) as f:
        text = f.read().lower()
    assert "sample_posterior" not in text and "posterior_noise" not in text


def test_null_handle_and_argument_answers():
    lib = chain._sampling_lib()
    n, x = C.c_int32(7), (C.c_double * 4)()
    assert lib.gpslam_hip_posterior_noise_dim(None, C.byref(n)) == -1 and n.value == 7
    assert lib.gpslam_hip_posterior_noise(None, 1, 0, 1, x) == -1
    assert lib.gpslam_hip_sample_posterior(None, 1, 1, 0, None, x, None, None, None) == -1
    # count <= 0 and all-NULL outputs: refused before the handle is looked at
    for count in (0, -3):
        assert lib.gpslam_hip_sample_posterior(None, count, 1, 0, None, x, x, x, x) == -1
        assert lib.gpslam_hip_posterior_noise(None, 1, 0, count, x) == -1
    assert lib.gpslam_hip_sample_posterior(None, 1, 1, 0, None, None, None, None, None) == -1


def _build(tmp_path):
    gp.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "posterior_host_tests.cpp")
    exe = str(tmp_path / "posterior_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_sample_posterior_compiles_links_and_refuses_without_a_device(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=60)      # (no argument: no device call)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "posterior_host_tests: all tests passed" in out.stdout


def test_host_header_type_checks_next_to_the_gtsam_declarations(tmp_path):
    """the adapter (over tests/cpp/gtsam_decl) and the sampling header in one translation unit"""
    decl = os.path.join(ROOT, "tests", "cpp", "gtsam_decl")
    src = str(tmp_path / "posterior_tu.cpp")
    with open(src, "w") as f:
        f.write('#include "%s"\n#include "%s"\n' % (os.path.join(ROOT, "gpslam_amd", "host", "gtsam_adapter.hpp"), os.path.join(ROOT, "include", "gpslam_hip_sampling.h")))
        f.write("int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", decl, src])


@pytest.mark.gpu
def test_a_draw_equals_the_python_bindings(tmp_path):
    from test_evidence_cpp import _python_twin
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "posterior_host_tests: all tests passed" in out.stdout
    cpp = np.array([float(v) for v in re.search(r"draw 1 state 3: (.*)", out.stdout).group(1).split()])
    dev = _python_twin()
    _, poses, vels, _ = dev.sample_posterior(1, seed=(9 << 40) + 77, first=6)
    py = np.concatenate([poses[0, 3], vels[0, 3]])
    # the same device arithmetic on the same numbers up to the last place of sin / cos in the states: the project's per-step bound
    print("C++ %s\nPython %s" % (cpp, py))
    assert np.abs(cpp - py).max() <= 1e-9 * max(1.0, np.abs(py).max())

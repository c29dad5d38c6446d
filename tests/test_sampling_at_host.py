"""Posterior sampling at query times, the interface without a device (include/gpslam_hip_sampling_at.h): the three symbols exist in
the library, the header and the binding's own list and in no other, ABI 2.4, gpslam_hip.h and gpslam_hip_sampling.h declare what
they declared, the NULL-handle and argument answers, and samplePosteriorAt of gpslam_amd/host/gpslam_host.hpp
(tests/cpp/sampling_at_host_tests.cpp) compiles with -Wall -Werror and links.  On the GPU the C++ draw of a small Pose2 graph equals
the Python binding's on the same numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpslam_hip_posterior_noise_at", "gpslam_hip_posterior_noise_dim_at", "gpslam_hip_sample_posterior_at"]


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(r"\b(gpslam_hip_[a-z0-9_]+)\s*\(", f.read())))


def test_symbols_exist_in_the_library_the_header_and_the_binding():
    lib = gp.load_library()
    assert _declared("gpslam_hip_sampling_at.h") == sorted(chain.SAMPLING_AT_SYMBOLS) == NAMES
    others = chain.ABI_SYMBOLS + chain.DOGLEG_SYMBOLS + chain.EVIDENCE_SYMBOLS + chain.QC_SYMBOLS + chain.SAMPLING_SYMBOLS + chain.NOISE_SYMBOLS
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name not in others
    for name in ("posterior_noise_dim_at", "posterior_noise_at", "sample_posterior_at"):
        assert callable(getattr(gp.ChainSolver, name))
    with open(os.path.join(ROOT, "include", "gpslam_hip_sampling_at.h")) as f:
        assert '#include "gpslam_hip_sampling.h"' in f.read()


def test_abi_and_the_older_headers_are_untouched():
    lib = gp.load_library()
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    assert _declared("gpslam_hip.h") == sorted(chain.ABI_SYMBOLS)
    assert _declared("gpslam_hip_sampling.h") == sorted(chain.SAMPLING_SYMBOLS)
    assert len(chain.SAMPLING_SYMBOLS) == 3
    for header in ("gpslam_hip.h", "gpslam_hip_sampling.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            text = f.read().lower()
        assert "sample_posterior_at" not in text and "noise_dim_at" not in text and "posterior_noise_at" not in text


def test_null_handle_and_argument_answers():
    lib = chain._sampling_at_lib()
    n, x = C.c_int32(7), (C.c_double * 4)()
    left, dt, tau = (C.c_int32 * 1)(0), (C.c_double * 1)(1.0), (C.c_double * 1)(0.5)
    assert lib.gpslam_hip_posterior_noise_dim_at(None, 1, C.byref(n)) == -1 and n.value == 7
    assert lib.gpslam_hip_posterior_noise_at(None, 1, 0, 1, 1, x) == -1
    assert lib.gpslam_hip_sample_posterior_at(None, 1, 1, 0, None, 1, left, dt, tau, x, None, None, None, None, None) == -1
    # count <= 0, n_queries <= 0, missing query arrays and all-NULL outputs: refused before the handle is looked at
    for bad in (0, -3):
        assert lib.gpslam_hip_sample_posterior_at(None, bad, 1, 0, None, 1, left, dt, tau, x, x, x, x, x, x) == -1
        assert lib.gpslam_hip_sample_posterior_at(None, 1, 1, 0, None, bad, left, dt, tau, x, x, x, x, x, x) == -1
        assert lib.gpslam_hip_posterior_noise_at(None, 1, 0, bad, 1, x) == -1
        assert lib.gpslam_hip_posterior_noise_at(None, 1, 0, 1, bad, x) == -1
    assert lib.gpslam_hip_sample_posterior_at(None, 1, 1, 0, None, 1, None, dt, tau, x, None, None, None, None, None) == -1
    assert lib.gpslam_hip_sample_posterior_at(None, 1, 1, 0, None, 1, left, dt, tau, None, None, None, None, None, None) == -1


def _build(tmp_path):
    gp.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "sampling_at_host_tests.cpp")
    exe = str(tmp_path / "sampling_at_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_sample_posterior_at_compiles_links_and_refuses_without_a_device(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=60)      # (no argument: no device call)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sampling_at_host_tests: all tests passed" in out.stdout


@pytest.mark.gpu
def test_a_dense_draw_equals_the_python_bindings(tmp_path):
    from test_evidence_cpp import _python_twin
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sampling_at_host_tests: all tests passed" in out.stdout
    cpp = np.array([float(v) for v in re.search(r"draw 1 query 2: (.*)", out.stdout).group(1).split()])
    dev = _python_twin()
    N, dt = dev.N, 0.25
    qp = dev.sample_posterior_at([0, 4, 4, N - 2], [dt] * 4, [0.1, 0.05, 0.2, 0.125], 1, seed=(9 << 40) + 77, first=6)[0]
    py = qp[0, 2]
    # the same device arithmetic on the same numbers up to the last place of sin / cos in the states: the project's per-step bound
    print("C++ %s\nPython %s" % (cpp, py))
    assert np.abs(cpp - py).max() <= 1e-9 * max(1.0, np.abs(py).max())

"""Marginals on handles whose loop closures go in column passes, host side: gpslam_hip_marginals_keep_closure_columns is exported and
listed, the ABI stays 2.4 (added without a bump, as the closure-pass calls were), and a C++ program that builds gtsam::Marginals
on a graph with 12 non-adjacent BetweenFactor<Pose2> (tests/cpp/marginals_passes_host_tests.cpp) compiles with -Wall -Werror and
links; on the GPU the same program compares the class's blocks with gpslam_hip_get_marginals on its handle."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "gpslam_hip_marginals_keep_closure_columns"


def test_library_exports_the_opt_in_and_keeps_abi_2_4():
    import gpslam_amd
    from gpslam_amd import chain
    lib = gpslam_amd.load_library()
    assert hasattr(lib, SYMBOL)
    assert SYMBOL in chain.ABI_SYMBOLS
    assert hasattr(chain.ChainSolver, "marginals_keep_closure_columns")
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    assert (chain.ABI_MAJOR, chain.ABI_MINOR) == (2, 4)
    # the argument check needs no device
    assert lib.gpslam_hip_marginals_keep_closure_columns(None, 1) == -1


def test_header_declares_the_opt_in_with_its_memory_formula():
    with open(os.path.join(ROOT, "include", "gpslam_hip.h")) as f:
        text = f.read()
    assert "int gpslam_hip_marginals_keep_closure_columns(gpslam_hip_handle *h, int32_t enable);" in text
    assert "#define GPSLAM_HIP_ABI_MINOR 4" in text
    assert "N * nc * b * 8 bytes" in text


def _build(tmp_path):
    import gpslam_amd
    gpslam_amd.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "marginals_passes_host_tests.cpp")
    exe = str(tmp_path / "marginals_passes_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_host_program_compiles_and_links(tmp_path):
    assert subprocess.run([_build(tmp_path)], timeout=60).returncode == 0      # (no argument: the NULL-handle check, no device call)


@pytest.mark.gpu
def test_marginals_class_on_12_closures(tmp_path):
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "marginals_passes_host_tests: all tests passed" in out.stdout

"""Loop closures in column passes, host side: the two entry points are exported and listed, the ABI stays 2.4 (they were added without
a bump), and a C++ program that hands 12 non-adjacent BetweenFactor<Pose2> to the host classes (tests/cpp/closure_passes_host_tests.cpp)
compiles with -Wall -Werror and links; on the GPU the same program optimises that graph."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gpslam_hip_set_closure_passes", "gpslam_hip_closure_info"]


def test_library_exports_the_closure_pass_calls_and_keeps_abi_2_4():
    import gpslam_amd
    from gpslam_amd import chain
    lib = gpslam_amd.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in chain.ABI_SYMBOLS, s
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    # argument checks that need no device
    assert lib.gpslam_hip_set_closure_passes(None, 4, 0) == -1
    assert lib.gpslam_hip_closure_info(None, None) == -1


def _build(tmp_path):
    import gpslam_amd
    gpslam_amd.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "closure_passes_host_tests.cpp")
    exe = str(tmp_path / "closure_passes_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_host_program_with_12_closures_compiles_and_links(tmp_path):
    assert subprocess.run([_build(tmp_path)], timeout=60).returncode == 0      # (no argument: no device call)


@pytest.mark.gpu
def test_host_classes_switch_the_column_passes_on(tmp_path):
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "closure_passes_host_tests: all tests passed" in out.stdout

"""Fixed-lag smoothing with landmarks, host side: a C++ program that uses gtsam::LinearContainerFactor over (x, v, landmarks) and
gtsam::BatchFixedLagSmoother::marginalizeOntoLandmarks (tests/cpp/fixed_lag_border_host_tests.cpp) compiles with -Wall -Werror and
links; on the GPU the same program checks the container factor against the priors it restates and lets the smoother slide over a
range graph."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import gpslam_amd
    gpslam_amd.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "fixed_lag_border_host_tests.cpp")
    exe = str(tmp_path / "fixed_lag_border_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_host_program_compiles_and_links(tmp_path):
    assert subprocess.run([_build(tmp_path)], timeout=60).returncode == 0      # (no argument: the NULL-handle checks, no device call)


@pytest.mark.gpu
def test_smoother_and_container_factor_over_landmarks(tmp_path):
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fixed_lag_border_host_tests: all tests passed" in out.stdout

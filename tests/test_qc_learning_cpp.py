"""qcStatistic of gpslam_amd/host/gpslam_host.hpp (tests/cpp/qc_host_tests.cpp): compiles with -Wall -Werror and links; without a device
it checks the three host-arithmetic entry points and the NULL-handle answer; on the GPU the statistic of a small Pose2 graph equals the
Python binding's on the same numbers, and GP priors on another Qc_model are left out."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_evidence_cpp import _python_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import gpslam_amd
    gpslam_amd.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "qc_host_tests.cpp")
    exe = str(tmp_path / "qc_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_host_functions_and_null_answers(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=60)      # (no argument: no device call)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "qc_host_tests: all tests passed" in out.stdout


@pytest.mark.gpu
def test_qc_statistic_equals_the_python_bindings(tmp_path):
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "qc_host_tests: all tests passed" in out.stdout
    nums = re.search(r"qcStatistic at_start (.*)", out.stdout).group(1).split()
    n_cpp, A_cpp = int(nums[0]), np.array([float(v) for v in nums[1:]]).reshape(3, 3)
    dev = _python_twin()
    dev.marginals()
    A, n_f = dev.qc_statistic()
    print("C++ %s\nPython %s" % (A_cpp, A))
    assert n_cpp == n_f == 11
    # the same device arithmetic on the same numbers up to the last place of sin / cos in the states; the marginals answer a
    # relative change eps of H with kappa eps, kappa the condition number the marginals tests cap at 4.5e6: 1e-9
    assert np.abs(A_cpp - A).max() <= 1e-9 * np.abs(A).max()

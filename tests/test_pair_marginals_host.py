"""Joint marginals over any states and the closure gate, host side: a C++ program that builds gtsam::Marginals on a Pose2 graph with a
loop closure and two landmarks (tests/cpp/pair_marginals_host_tests.cpp) compiles with -Wall -Werror and links; on the GPU the same
program checks that {x0, x2} still throws by default, that after Marginals::serveAnyStates() the set {x0, v7, x31, l1} equals the
blocks of the C getters, and that Marginals::betweenChiSquared equals gpslam_hip_gate_between_pairs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import gpslam_amd
    gpslam_amd.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "pair_marginals_host_tests.cpp")
    exe = str(tmp_path / "pair_marginals_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_host_program_compiles_and_links(tmp_path):
    assert subprocess.run([_build(tmp_path)], timeout=60).returncode == 0      # (no argument: the NULL-handle checks, no device call)


@pytest.mark.gpu
def test_marginals_class_serves_any_states_and_gates(tmp_path):
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pair_marginals_host_tests: all tests passed" in out.stdout

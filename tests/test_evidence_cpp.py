"""logDeterminant / logEvidence of gpslam_amd/host/gpslam_host.hpp (tests/cpp/evidence_host_tests.cpp): compiles with -Wall -Werror next
to the declaration headers of tests/cpp/gtsam_decl and links; without a device it checks the two host-arithmetic entry points and the
NULL-handle answers; on the GPU the logEvidence of a small Pose2 graph equals the Python binding's on the same numbers."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import gpslam_amd
    gpslam_amd.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "evidence_host_tests.cpp")
    exe = str(tmp_path / "evidence_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_host_functions_and_null_answers(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=60)      # (no argument: no device call)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "evidence_host_tests: all tests passed" in out.stdout


def test_host_header_type_checks_next_to_the_gtsam_declarations(tmp_path):
    """the adapter (over tests/cpp/gtsam_decl) and the host classes with logDeterminant / logEvidence in one translation unit"""
    decl = os.path.join(ROOT, "tests", "cpp", "gtsam_decl")
    src = str(tmp_path / "evidence_tu.cpp")
    with open(src, "w") as f:
        f.write('#include "%s"\n#include "%s"\n' % (os.path.join(ROOT, "gpslam_amd", "host", "gtsam_adapter.hpp"), os.path.join(ROOT, "include", "gpslam_hip_evidence.h")))
        f.write("int main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", decl, src])


def _python_twin():
    """the graph of test_log_evidence_of_a_pose2_chain at its start, through the Python binding"""
    import gpslam_amd as gp
    N, dt, w, v = 12, 0.25, 0.6, 1.0
    th = dt * w
    step = np.array([v * dt * np.sin(th) / th, v * dt * (1 - np.cos(th)) / th, th])
    truth = np.zeros((N, 3))
    for k in range(N - 1):
        a = truth[k]
        truth[k + 1] = [a[0] + np.cos(a[2]) * step[0] - np.sin(a[2]) * step[1], a[1] + np.sin(a[2]) * step[0] + np.cos(a[2]) * step[1], a[2] + step[2]]
    k = np.arange(N)
    pose = truth + np.stack([0.03 * np.sin(0.7 * k), -0.02 * np.cos(0.4 * k), 0.04 * np.sin(0.3 * k)], -1)
    dev = gp.ChainSolver(gp.POSE2, chart=gp.CHART_FIRST_ORDER)
    dev.set_qc(0.5 * np.eye(3))
    dev.set_states(pose, np.tile([v, 0.0, w], (N, 1)))
    dev.add_pose_priors(np.array([0], dtype=np.int32), truth[:1], np.full((1, 3), 1e-2))
    dev.add_gp_priors(np.arange(N - 1, dtype=np.int32), np.full(N - 1, dt))
    dev.add_between(np.arange(N - 1, dtype=np.int32), np.tile(step, (N - 1, 1)), np.full((N - 1, 3), 2e-2))
    dev.compile()
    return dev


@pytest.mark.gpu
def test_log_evidence_equals_the_python_bindings(tmp_path):
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "evidence_host_tests: all tests passed" in out.stdout
    cpp = float(re.search(r"logEvidence at_start (\S+)", out.stdout).group(1))
    logZ, cost, logdet, lognorm, mn = _python_twin().log_evidence()
    # the same device arithmetic on the same numbers up to the last place of sin / cos in the states: 1e-11, the bound of the scalars
    scale = abs(cost) + abs(lognorm) + 0.5 * abs(logdet) + 0.5 * abs(mn) * np.log(2 * np.pi)
    print("C++ %.15g, Python %.15g" % (cpp, logZ))
    assert mn == 3 + 11 * 9 - 12 * 6
    assert abs(cpp - logZ) <= 1e-11 * scale

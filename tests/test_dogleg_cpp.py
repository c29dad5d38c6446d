"""gtsam::DoglegOptimizer of gpslam_amd/host/gpslam_host.hpp (tests/cpp/dogleg_host_tests.cpp): compiles with -Wall -Werror next to the
declaration headers of tests/cpp/gtsam_decl and links; without a device it checks the mapping of DoglegParams onto the arguments of
gpslam_hip_iterate_dogleg, the two host-arithmetic entry points and the NULL-handle answers; on the GPU it runs a Pose2 chain with range
landmarks to the fixed point LevenbergMarquardtOptimizer reaches."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    import gpslam_amd
    gpslam_amd.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "dogleg_host_tests.cpp")
    exe = str(tmp_path / "dogleg_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_dogleg_optimizer_compiles_and_maps_its_parameters(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=60)      # (no argument: no device call)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dogleg_host_tests: all tests passed" in out.stdout


def test_host_header_type_checks_next_to_the_gtsam_declarations(tmp_path):
    """the adapter (over tests/cpp/gtsam_decl) and the host classes with DoglegOptimizer in one translation unit"""
    decl = os.path.join(ROOT, "tests", "cpp", "gtsam_decl")
    src = str(tmp_path / "dogleg_tu.cpp")
    with open(src, "w") as f:
        f.write('#include "%s"\n#include "%s"\n' % (os.path.join(ROOT, "gpslam_amd", "host", "gtsam_adapter.hpp"), os.path.join(ROOT, "include", "gpslam_hip_dogleg.h")))
        f.write("static_assert(GPSLAM_DOGLEG_SEARCH_REDUCE_ONLY == 2, \"modes\");\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", decl, src])


@pytest.mark.gpu
def test_dogleg_optimizer_reaches_the_levenberg_marquardt_fixed_point(tmp_path):
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dogleg_host_tests: all tests passed" in out.stdout

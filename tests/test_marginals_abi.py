"""CPU: the marginals entry points (ABI 2.3) are exported, the library reports ABI 2.4, and gtsam::Marginals of the C++ host header compiles and links."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gpslam_hip_marginals", "gpslam_hip_get_marginals", "gpslam_hip_interpolate_covariances"]


def test_library_exports_the_marginals_and_reports_abi_2_3():
    """(the test keeps the name it got with ABI 2.3, whose symbols it looks for; the version it pins is the current one, 2.4)"""
    import gpslam_amd
    from gpslam_amd import chain
    lib = gpslam_amd.load_library()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in chain.ABI_SYMBOLS, s
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)


def test_marginals_host_program_compiles_and_links(tmp_path):
    import gpslam_amd
    gpslam_amd.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = tmp_path / "marginals_user.cpp"
    src.write_text(r'''
#include "gpslam_amd/host/gpslam_host.hpp"
using namespace gtsam;
int main(int argc, char **) {
  if (argc < 2) return 0;   // (link check only: running it needs a device)
  NonlinearFactorGraph graph;
  Values values;
  Marginals m(graph, values);
  Matrix P = m.marginalCovariance(Symbol('x', 0));
  Matrix I = m.marginalInformation(Symbol('v', 0));
  JointMarginal j = m.jointMarginalCovariance(KeyVector{Symbol('x', 0), Symbol('x', 1)});
  Matrix X = j(Symbol('x', 0), Symbol('x', 1));
  std::vector<Matrix> c = m.interpolatePoseCovariances(KeyVector{Symbol('x', 0)}, {0.1}, {0.05});
  return (int)(P.rows + I.rows + X.rows + j.fullMatrix().rows + c.size());
}
''')
    exe = tmp_path / "marginals_user"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe), "-L", libdir,
                           "-lgpslam_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.run([str(exe)], timeout=60).returncode == 0

"""The host arithmetic of measurement-noise learning (include/gpslam_hip_noise.h) on the CPU: gpslam_hip_noise_gradient,
gpslam_hip_noise_em_update and gpslam_hip_noise_em_scale against numpy, their refusals, the NULL-handle answers of the two device
calls, and the binding's bookkeeping (the new symbols exist in the library, the new header and the binding's own list; the other
headers and ABI 2.4 are untouched).  tests/cpp/noise_host_tests.cpp compiles with -Wall -Werror and links measNoiseStatistic; on the
GPU its statistic of a small 2-D linear chain with odometry equals the Python binding's on the same numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import chain
import noise_learning_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-11     # the project's bound for scalar host arithmetic


def _spd(r, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((r, r))
    return G @ G.T + 0.5 * np.eye(r)


@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 39, 10 ** 6, 2 ** 40])
def test_the_three_functions_against_numpy(r, n):
    Cov, B = _spd(r, 3 + r), float(n) * _spd(r, 40 + r)
    assert r == 1 or np.count_nonzero(Cov - np.diag(np.diag(Cov))) == r * r - r       # full, not diagonal
    G = gp.noise_gradient(Cov, B, n)
    assert np.abs(G - NM.gradient(Cov, B, n)).max() <= REL * 0.5 * (n * np.abs(Cov).max() + np.abs(B).max())
    C1 = gp.noise_em_update(B, n)
    assert np.array_equal(C1, C1.T)
    assert np.abs(C1 - NM.em_update(B, n)).max() <= REL * np.abs(C1).max()
    assert np.abs(gp.noise_gradient(C1, B, n)).max() <= REL * np.abs(B).max()      # G = 0 at the M-step
    ratio, rows = gp.noise_em_scale(B, n)
    ref, ref_rows = NM.em_scale(B, n)
    assert abs(ratio - ref) <= REL * ref and np.abs(rows - ref_rows).max() <= REL * ref_rows.max()     # (a sum of positive terms)
    assert gp.noise_em_scale(float(n) * 0.37 * np.eye(r), n)[0] == pytest.approx(0.37, rel=1e-13)


def test_refusals():
    Cov, B = _spd(3, 1), _spd(3, 2)
    bad = Cov.copy()
    bad[2, 2] = -1.0
    indefinite = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    nan = Cov.copy()
    nan[0, 1] = nan[1, 0] = float("nan")
    inf = Cov.copy()
    inf[1, 1] = float("inf")
    for M in (bad, indefinite, np.zeros((3, 3)), nan, inf):
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.noise_gradient(M, B, 5)                 # C must be SPD
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.noise_em_update(M, 5)                   # B must be SPD for the answer to be one
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.noise_em_scale(M, 5)
    for M in (nan, inf):
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.noise_gradient(Cov, M, 5)
    assert np.all(np.isfinite(gp.noise_gradient(Cov, np.zeros((3, 3)), 5)))     # (B = 0 is a statistic: G = n C / 2)
    for n in (0, -3):
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.noise_gradient(Cov, B, n)
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.noise_em_update(B, n)
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.noise_em_scale(B, n)
    with pytest.raises(gp.GpslamHipError, match="square"):
        gp.noise_em_update(np.zeros((2, 3)), 1)
    with pytest.raises(gp.GpslamHipError, match="differ in size"):
        gp.noise_gradient(_spd(2, 0), B, 1)
    lib = chain._noise_lib()
    c, b, out, th = (C.c_double * 9)(*Cov.reshape(-1)), (C.c_double * 9)(*B.reshape(-1)), (C.c_double * 9)(), C.c_double(0.0)
    rows = (C.c_double * 3)()
    assert lib.gpslam_hip_noise_gradient(3, None, b, 5, out) == -1
    assert lib.gpslam_hip_noise_gradient(3, c, None, 5, out) == -1
    assert lib.gpslam_hip_noise_gradient(3, c, b, 5, None) == -1
    assert lib.gpslam_hip_noise_gradient(0, c, b, 5, out) == -1
    assert lib.gpslam_hip_noise_gradient(4, c, b, 5, out) == -1
    assert lib.gpslam_hip_noise_em_update(3, None, 5, out) == -1
    assert lib.gpslam_hip_noise_em_update(3, b, 5, None) == -1
    assert lib.gpslam_hip_noise_em_update(4, b, 5, out) == -1
    assert lib.gpslam_hip_noise_em_scale(3, None, 5, C.byref(th), rows) == -1
    assert lib.gpslam_hip_noise_em_scale(3, b, 5, None, rows) == -1
    assert lib.gpslam_hip_noise_em_scale(0, b, 5, C.byref(th), rows) == -1
    assert lib.gpslam_hip_noise_em_scale(3, b, 5, C.byref(th), None) == 0       # ratio_rows may be NULL
    assert lib.gpslam_hip_noise_gradient(3, c, b, 5, out) == 0


def test_null_handle():
    lib = chain._noise_lib()
    B, n = (C.c_double * 9)(), C.c_int64(0)
    assert lib.gpslam_hip_meas_noise_statistic(None, 3, None, B, B, C.byref(n)) == -1
    assert lib.gpslam_hip_meas_predicted_covariances(None, 3, B) == -1


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(r"\b(gpslam_hip_[a-z0-9_]+)\s*\(", f.read())))


def test_symbols_exist_in_the_library_the_header_and_the_binding():
    lib = gp.load_library()
    assert _declared("gpslam_hip_noise.h") == sorted(chain.NOISE_SYMBOLS)
    assert len(chain.NOISE_SYMBOLS) == 5
    others = chain.ABI_SYMBOLS + chain.DOGLEG_SYMBOLS + chain.EVIDENCE_SYMBOLS + chain.QC_SYMBOLS + chain.SAMPLING_SYMBOLS
    for name in chain.NOISE_SYMBOLS:
        assert hasattr(lib, name), name
        assert name not in others
    assert callable(gp.ChainSolver.meas_noise_statistic) and callable(gp.ChainSolver.meas_predicted_covariances)
    assert callable(gp.noise_gradient) and callable(gp.noise_em_update) and callable(gp.noise_em_scale)
    from gpslam_amd import evidence
    assert callable(evidence.learn_meas_noise)


def test_abi_and_the_other_headers_are_untouched():
    lib = gp.load_library()
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    for header, names in (("gpslam_hip.h", chain.ABI_SYMBOLS), ("gpslam_hip_evidence.h", chain.EVIDENCE_SYMBOLS), ("gpslam_hip_qc.h", chain.QC_SYMBOLS),
                          ("gpslam_hip_dogleg.h", chain.DOGLEG_SYMBOLS), ("gpslam_hip_sampling.h", chain.SAMPLING_SYMBOLS)):
        assert _declared(header) == sorted(names), header
        with open(os.path.join(ROOT, "include", header)) as f:
            text = f.read().lower()
        assert "gpslam_hip_noise" not in text and "gpslam_hip_meas_noise" not in text and "predicted_covariances" not in text, header


# ---------------------------------------------------------------- C++
def _build(tmp_path):
    gp.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "noise_host_tests.cpp")
    exe = str(tmp_path / "noise_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_host_functions_and_null_answers(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=60)      # (no argument: no device call)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "noise_host_tests: all tests passed" in out.stdout


@pytest.mark.gpu
def test_cpp_statistic_equals_the_python_bindings(tmp_path):
    out = subprocess.run([_build(tmp_path), "gpu"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "noise_host_tests: all tests passed" in out.stdout
    nums = re.search(r"measNoiseStatistic at_start (.*)", out.stdout).group(1).split()
    vals = np.array([float(v) for v in nums[1:]])
    n_cpp, B_cpp, Bw_cpp = int(nums[0]), vals[:9].reshape(3, 3), vals[9:].reshape(3, 3)
    N, dt = 12, 0.25
    k = np.arange(N)
    dev = gp.ChainSolver(gp.LINEAR3)
    dev.set_qc(0.5 * np.eye(3))
    dev.set_states(np.stack([0.25 * k + 0.03 * np.sin(0.7 * k), 0.1 * k - 0.02 * np.cos(0.4 * k), 0.05 * k + 0.04 * np.sin(0.3 * k)], axis=1),
                   np.tile([1.0, 0.4, 0.2], (N, 1)))
    dev.add_pose_priors([0], np.zeros((1, 3)), np.full((1, 3), 1e-2))
    left = np.arange(N - 1)
    dev.add_gp_priors(left, np.full(N - 1, dt))
    dev.add_odometry2d(left, np.stack([np.full(N - 1, 0.26), 0.02 * left, np.full(N - 1, 0.05)], axis=1),
                       np.stack([0.05 + 0.01 * left, np.full(N - 1, 0.08), 0.02 + 0.005 * left], axis=1))
    dev.compile()
    dev.marginals()
    B, Bw, n = dev.meas_noise_statistic(gp.chain.MEAS_ODOMETRY2D)
    print("C++ %s\nPython %s" % (B_cpp, B))
    assert n_cpp == n == N - 1
    # the same device arithmetic on the same numbers up to the last place of sin / cos in the states; the marginals answer a
    # relative change eps of H with kappa eps, kappa the condition number the marginals tests cap at 4.5e6: 1e-9
    assert np.abs(B_cpp - B).max() <= 1e-9 * np.abs(B).max() and np.abs(Bw_cpp - Bw).max() <= 1e-9 * np.abs(Bw).max()

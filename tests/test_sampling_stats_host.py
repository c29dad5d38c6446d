"""Statistics of posterior draws, the interface without a device (include/gpslam_hip_sampling_stats.h): the two symbols exist in the
library, the header and the binding's own list and in no other, ABI 2.4, the older headers declare what their lists say, the
NULL-handle and argument answers, gpslam_hip_posterior_moments (host arithmetic) against numpy.mean / numpy.cov, and
samplePosteriorStats of gpslam_amd/host/gpslam_host.hpp (tests/cpp/sampling_stats_host_tests.cpp) compiles with -Wall -Werror, links
and refuses without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import chain
import posterior_stats_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gpslam_hip_posterior_moments", "gpslam_hip_sample_posterior_stats"]


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(r"\b(gpslam_hip_[a-z0-9_]+)\s*\(", f.read())))


def test_symbols_exist_in_the_library_the_header_and_the_binding():
    lib = gp.load_library()
    assert _declared("gpslam_hip_sampling_stats.h") == sorted(chain.SAMPLING_STATS_SYMBOLS) == NAMES
    others = (chain.ABI_SYMBOLS + chain.DOGLEG_SYMBOLS + chain.EVIDENCE_SYMBOLS + chain.QC_SYMBOLS + chain.SAMPLING_SYMBOLS + chain.SAMPLING_AT_SYMBOLS
              + chain.NOISE_SYMBOLS)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name not in others
    for name in ("sample_posterior_stats", "posterior_moments"):
        assert callable(getattr(gp.ChainSolver, name))
    with open(os.path.join(ROOT, "include", "gpslam_hip_sampling_stats.h")) as f:
        assert '#include "gpslam_hip_sampling_at.h"' in f.read()


def test_abi_and_the_older_headers_are_untouched():
    lib = gp.load_library()
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    lists = {"gpslam_hip.h": chain.ABI_SYMBOLS, "gpslam_hip_dogleg.h": chain.DOGLEG_SYMBOLS, "gpslam_hip_evidence.h": chain.EVIDENCE_SYMBOLS,
             "gpslam_hip_qc.h": chain.QC_SYMBOLS, "gpslam_hip_sampling.h": chain.SAMPLING_SYMBOLS, "gpslam_hip_sampling_at.h": chain.SAMPLING_AT_SYMBOLS,
             "gpslam_hip_noise.h": chain.NOISE_SYMBOLS}
    for header, names in lists.items():
        assert _declared(header) == sorted(names), header
        with open(os.path.join(ROOT, "include", header)) as f:
            text = f.read().lower()
        assert "posterior_stats" not in text and "posterior_moments" not in text
    assert len(chain.SAMPLING_SYMBOLS) == 3 and len(chain.SAMPLING_AT_SYMBOLS) == 3 and len(chain.SAMPLING_STATS_SYMBOLS) == 2


def test_null_handle_and_argument_answers():
    lib = chain._sampling_stats_lib()
    n, x, hits = C.c_int64(7), (C.c_double * 8)(), (C.c_int64 * 1)()
    left, dt, tau, ob = (C.c_int32 * 1)(0), (C.c_double * 1)(1.0), (C.c_double * 1)(0.5), (C.c_double * 3)(0.0, 0.0, 1.0)
    call = lib.gpslam_hip_sample_posterior_stats
    assert call(None, 1, 1, 0, None, 1, left, dt, tau, 1, ob, 0.0, 0, C.byref(n), x, x, hits, x, x) == -1 and n.value == 7
    # count <= 0, n_queries <= 0, missing query arrays and all-NULL outputs: refused before the handle is looked at
    for bad in (0, -3):
        assert call(None, bad, 1, 0, None, 1, left, dt, tau, 1, ob, 0.0, 0, C.byref(n), x, x, hits, x, x) == -1
        assert call(None, 1, 1, 0, None, bad, left, dt, tau, 1, ob, 0.0, 0, C.byref(n), x, x, hits, x, x) == -1
    assert call(None, 1, 1, 0, None, 1, None, dt, tau, 1, ob, 0.0, 0, C.byref(n), x, x, hits, x, x) == -1
    assert call(None, 1, 1, 0, None, 1, left, dt, tau, 0, None, 0.0, 0, C.byref(n), None, None, None, None, None) == -1


@pytest.mark.parametrize("d", [2, 3, 6])
@pytest.mark.parametrize("n", [2, 5])
def test_posterior_moments_against_numpy(d, n):
    rng = np.random.default_rng(100 * d + n)
    nq = 4
    e = rng.standard_normal((n, nq, d)) * np.array([1.0, 1e-2, 30.0, 1.0])[None, :, None] + rng.standard_normal((nq, d))[None]
    s1 = e.sum(axis=0)
    s2 = np.array([SM.pack(e[:, q, :].T @ e[:, q, :]) for q in range(nq)])
    mean, cov = gp.ChainSolver.posterior_moments(n, s1, s2)
    want_m = np.mean(e, axis=0)
    want_c = np.array([np.cov(e[:, q, :].T) for q in range(nq)])
    scale = np.abs(want_c).max()      # the largest entry
    print("d %d, n %d: mean %.3g of %.3g, cov %.3g of %.3g" % (d, n, np.abs(mean - want_m).max(), 1e-13 * np.abs(want_m).max(), np.abs(cov - want_c).max(), 1e-13 * scale))
    assert mean.shape == (nq, d) and cov.shape == (nq, d, d)
    assert np.abs(mean - want_m).max() <= 1e-13 * np.abs(want_m).max()
    assert np.abs(cov - want_c).max() <= 1e-13 * scale
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    m2, c2 = SM.moments(n, s1, s2)
    assert np.abs(mean - m2).max() <= 1e-15 * np.abs(m2).max() and np.abs(cov - c2).max() <= 1e-13 * scale


def test_posterior_moments_refuses_too_few_draws():
    s1, s2 = np.ones((2, 3)), np.ones((2, 6))
    mean, cov = gp.ChainSolver.posterior_moments(1, s1, s2, cov=False)
    assert cov is None and np.array_equal(mean, s1)
    for n, cov in ((1, True), (0, False), (0, True), (-2, False)):
        with pytest.raises(gp.GpslamHipError, match=r"\(-1\)"):
            gp.ChainSolver.posterior_moments(n, s1, s2, cov=cov)
    with pytest.raises(gp.GpslamHipError, match="s2 must be"):
        gp.ChainSolver.posterior_moments(3, s1, np.ones((2, 5)))
    lib = chain._sampling_stats_lib()
    dp = C.POINTER(C.c_double)
    out = np.zeros((2, 3))
    assert lib.gpslam_hip_posterior_moments(3, 2, 3, None, s2.ctypes.data_as(dp), out.ctypes.data_as(dp), None) == -1
    assert lib.gpslam_hip_posterior_moments(3, 2, 3, s1.ctypes.data_as(dp), s2.ctypes.data_as(dp), None, None) == -1
    assert lib.gpslam_hip_posterior_moments(0, 2, 3, s1.ctypes.data_as(dp), s2.ctypes.data_as(dp), out.ctypes.data_as(dp), None) == -1


def _build(tmp_path):
    gp.load_library()
    libdir = os.path.join(ROOT, "gpslam_amd", "lib")
    src = os.path.join(ROOT, "tests", "cpp", "sampling_stats_host_tests.cpp")
    exe = str(tmp_path / "sampling_stats_host_tests")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", ROOT, src, "-o", exe, "-L", libdir, "-lgpslam_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_sample_posterior_stats_compiles_links_and_refuses_without_a_device(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=60)      # (no device call)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sampling_stats_host_tests: all tests passed" in out.stdout

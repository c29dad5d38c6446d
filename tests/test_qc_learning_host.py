"""The host arithmetic of Qc learning (include/gpslam_hip_qc.h) on the CPU: gpslam_hip_qc_gradient, gpslam_hip_qc_em_update and
gpslam_hip_qc_em_scale against numpy, their refusals, the NULL-handle answer of gpslam_hip_qc_statistic, and the binding's
bookkeeping (the new symbols exist in the library, the new header and the binding's own list; the other headers and ABI 2.4 are
untouched)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import chain
import qc_learning_model as QM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-11     # the project's bound for scalar host arithmetic


def _spd(d, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((d, d))
    return G @ G.T + 0.5 * np.eye(d)


@pytest.mark.parametrize("d", [1, 2, 3, 6])
@pytest.mark.parametrize("n_f", [1, 39, 10 ** 6, 2 ** 40])
def test_the_three_functions_against_numpy(d, n_f):
    Qc, A = _spd(d, 3 + d), (2.0 * n_f) * _spd(d, 40 + d)
    assert d == 1 or np.count_nonzero(Qc - np.diag(np.diag(Qc))) == d * d - d       # full, not diagonal
    G = gp.qc_gradient(Qc, A, n_f)
    assert np.abs(G - QM.gradient(Qc, A, n_f)).max() <= REL * (n_f * np.abs(Qc).max() + 0.5 * np.abs(A).max())
    Q1 = gp.qc_em_update(A, n_f)
    assert np.array_equal(Q1, Q1.T)
    assert np.abs(Q1 - QM.em_update(A, n_f)).max() <= REL * np.abs(Q1).max()
    assert np.abs(gp.qc_gradient(Q1, A, n_f)).max() <= REL * np.abs(A).max()      # G = 0 at the M-step
    th = gp.qc_em_scale(Qc, A, n_f)
    ref = QM.em_scale(Qc, A, n_f)
    # tr(Qc^-1 A) sums d terms of either sign: relative to sum_j |Qc^-1| |A| (its condition), which is what numpy's own answer carries
    scale = float(np.sum(np.abs(np.linalg.inv(Qc)) @ np.abs(A) * np.eye(d))) / (2.0 * n_f * d)
    assert abs(th - ref) <= REL * scale, (th, ref)
    assert gp.qc_em_scale(Qc, (2.0 * n_f) * 0.37 * Qc, n_f) == pytest.approx(0.37, rel=1e-13)


def test_refusals():
    Qc, A = _spd(3, 1), _spd(3, 2)
    bad = Qc.copy()
    bad[2, 2] = -1.0
    indefinite = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    nan = Qc.copy()
    nan[0, 1] = nan[1, 0] = float("nan")
    for M in (bad, indefinite, np.zeros((3, 3)), nan):
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.qc_gradient(M, A, 5)                 # Qc must be SPD
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.qc_em_update(M, 5)                   # A must be SPD for the answer to be one
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.qc_em_scale(M, A, 5)
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.qc_em_scale(Qc, M, 5)
    with pytest.raises(gp.GpslamHipError, match="-1"):
        gp.qc_gradient(Qc, nan, 5)
    assert np.all(np.isfinite(gp.qc_gradient(Qc, np.zeros((3, 3)), 5)))     # (A = 0 is a statistic: G = n_f Qc)
    for n_f in (0, -3):
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.qc_gradient(Qc, A, n_f)
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.qc_em_update(A, n_f)
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.qc_em_scale(Qc, A, n_f)
    with pytest.raises(gp.GpslamHipError, match="square"):
        gp.qc_em_update(np.zeros((2, 3)), 1)
    with pytest.raises(gp.GpslamHipError, match="differ in size"):
        gp.qc_gradient(_spd(2, 0), A, 1)
    lib = chain._qc_lib()
    q, a, out, th = (C.c_double * 9)(*Qc.reshape(-1)), (C.c_double * 9)(*A.reshape(-1)), (C.c_double * 9)(), C.c_double(0.0)
    assert lib.gpslam_hip_qc_gradient(3, None, a, 5, out) == -1
    assert lib.gpslam_hip_qc_gradient(3, q, None, 5, out) == -1
    assert lib.gpslam_hip_qc_gradient(3, q, a, 5, None) == -1
    assert lib.gpslam_hip_qc_gradient(0, q, a, 5, out) == -1
    assert lib.gpslam_hip_qc_gradient(7, q, a, 5, out) == -1
    assert lib.gpslam_hip_qc_em_update(3, None, 5, out) == -1
    assert lib.gpslam_hip_qc_em_update(3, a, 5, None) == -1
    assert lib.gpslam_hip_qc_em_update(7, a, 5, out) == -1
    assert lib.gpslam_hip_qc_em_scale(3, None, a, 5, C.byref(th)) == -1
    assert lib.gpslam_hip_qc_em_scale(3, q, None, 5, C.byref(th)) == -1
    assert lib.gpslam_hip_qc_em_scale(3, q, a, 5, None) == -1
    assert lib.gpslam_hip_qc_em_scale(0, q, a, 5, C.byref(th)) == -1
    assert lib.gpslam_hip_qc_gradient(3, q, a, 5, out) == 0


def test_null_handle():
    lib = chain._qc_lib()
    A, n = (C.c_double * 36)(), C.c_int64(0)
    assert lib.gpslam_hip_qc_statistic(None, A, C.byref(n)) == -1


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(r"\b(gpslam_hip_[a-z0-9_]+)\s*\(", f.read())))


def test_symbols_exist_in_the_library_the_header_and_the_binding():
    lib = gp.load_library()
    assert _declared("gpslam_hip_qc.h") == sorted(chain.QC_SYMBOLS)
    assert len(chain.QC_SYMBOLS) == 4
    for name in chain.QC_SYMBOLS:
        assert hasattr(lib, name), name
        assert name not in chain.ABI_SYMBOLS and name not in chain.DOGLEG_SYMBOLS and name not in chain.EVIDENCE_SYMBOLS
    assert callable(gp.ChainSolver.qc_statistic)
    assert callable(gp.qc_gradient) and callable(gp.qc_em_update) and callable(gp.qc_em_scale)
    from gpslam_amd import evidence
    assert callable(evidence.learn_qc)


def test_abi_and_the_other_headers_are_untouched():
    lib = gp.load_library()
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    assert _declared("gpslam_hip.h") == sorted(chain.ABI_SYMBOLS)
    assert _declared("gpslam_hip_evidence.h") == sorted(chain.EVIDENCE_SYMBOLS)
    for header in ("gpslam_hip.h", "gpslam_hip_evidence.h", "gpslam_hip_dogleg.h"):
        with open(os.path.join(ROOT, "include", header)) as f:
            assert "gpslam_hip_qc" not in f.read().lower(), header

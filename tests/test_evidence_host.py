"""The host arithmetic of the log-evidence (include/gpslam_hip_evidence.h) on the CPU: gpslam_hip_gp_log_normaliser and
gpslam_hip_evidence_combine against numpy, their refusals, the NULL-handle answers of the three handle entry points, and the binding's
bookkeeping (the new symbols exist in the library, the new header and the binding's own list; gpslam_hip.h and ABI 2.4 are untouched)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gpslam_amd as gp
from gpslam_amd import chain
import evidence_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-11     # the project's bound for scalar host arithmetic (the dogleg's scalars)


def _spd(d, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((d, d))
    return G @ G.T + 0.5 * np.eye(d)


@pytest.mark.parametrize("d", [2, 3, 6])
@pytest.mark.parametrize("dt", [1e-3, 0.1, 7.0])
def test_gp_log_normaliser_against_slogdet_of_Q(d, dt):
    Qc = _spd(d, 10 + d)        # full, not diagonal
    assert np.count_nonzero(Qc) == d * d
    Q = EM.gp_Q(dt, Qc)         # as marginals_model.gp_conditional builds it
    ref = -0.5 * np.linalg.slogdet(Q)[1]
    got = gp.gp_log_normaliser(Qc, dt)
    assert abs(got - ref) <= REL * abs(ref), (got, ref)
    assert abs(got - EM.gp_log_normaliser(Qc, dt)) <= REL * abs(ref)


def test_gp_log_normaliser_refusals():
    Qc = _spd(3, 1)
    for dt in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(gp.GpslamHipError, match="-1"):
            gp.gp_log_normaliser(Qc, dt)
    bad = Qc.copy()
    bad[2, 2] = -1.0
    with pytest.raises(gp.GpslamHipError, match="-1"):
        gp.gp_log_normaliser(bad, 0.1)
    with pytest.raises(gp.GpslamHipError, match="-1"):
        gp.gp_log_normaliser(np.array([[1.0, 2.0], [2.0, 1.0]]), 0.1)      # symmetric, indefinite
    with pytest.raises(gp.GpslamHipError, match="-1"):
        gp.gp_log_normaliser(np.zeros((3, 3)), 0.1)
    lib = chain._evidence_lib()
    out = C.c_double(0.0)
    q = (C.c_double * 9)(*Qc.reshape(-1))
    assert lib.gpslam_hip_gp_log_normaliser(3, None, 0.1, C.byref(out)) == -1
    assert lib.gpslam_hip_gp_log_normaliser(3, q, 0.1, None) == -1
    assert lib.gpslam_hip_gp_log_normaliser(0, q, 0.1, C.byref(out)) == -1
    assert lib.gpslam_hip_gp_log_normaliser(7, q, 0.1, C.byref(out)) == -1


def test_evidence_combine_against_the_formula():
    rng = np.random.default_rng(3)
    for _ in range(50):
        cost, logdet, lognorm = rng.uniform(0, 1e4), rng.uniform(-1e5, 1e5), rng.uniform(-1e5, 1e5)
        rows, nvars = int(rng.integers(0, 10 ** 7)), int(rng.integers(0, 10 ** 7))
        ref = -cost + lognorm - 0.5 * logdet - 0.5 * (rows - nvars) * np.log(2 * np.pi)
        got = gp.evidence_combine(cost, logdet, lognorm, rows, nvars)
        scale = abs(cost) + abs(lognorm) + 0.5 * abs(logdet) + 0.5 * abs(rows - nvars) * np.log(2 * np.pi)
        assert abs(got - ref) <= REL * scale
        assert got == EM.combine(cost, logdet, lognorm, rows, nvars) or abs(got - EM.combine(cost, logdet, lognorm, rows, nvars)) <= REL * scale
    assert gp.evidence_combine(0.0, 0.0, 0.0, 5, 5) == 0.0
    assert gp.evidence_combine(1.5, 4.0, 0.25, 2 ** 40, 2 ** 40 - 2) == pytest.approx(-1.5 + 0.25 - 2.0 - np.log(2 * np.pi), rel=1e-15)   # 64-bit counts
    assert chain._evidence_lib().gpslam_hip_evidence_combine(0.0, 0.0, 0.0, 1, 1, None) == -1


def test_null_handle():
    lib = chain._evidence_lib()
    out, p3, o5 = C.c_double(0.0), (C.c_double * 3)(), (C.c_double * 5)()
    m, n = C.c_int64(0), C.c_int64(0)
    assert lib.gpslam_hip_log_determinant(None, C.byref(out), p3) == -1
    assert lib.gpslam_hip_log_noise_normaliser(None, C.byref(out), C.byref(m), C.byref(n)) == -1
    assert lib.gpslam_hip_log_evidence(None, o5) == -1


def _declared(header):
    with open(os.path.join(ROOT, "include", header)) as f:
        return sorted(set(re.findall(r"\b(gpslam_hip_[a-z0-9_]+)\s*\(", f.read())))


def test_symbols_exist_in_the_library_the_header_and_the_binding():
    lib = gp.load_library()
    assert _declared("gpslam_hip_evidence.h") == sorted(chain.EVIDENCE_SYMBOLS)
    assert len(chain.EVIDENCE_SYMBOLS) == 5
    for name in chain.EVIDENCE_SYMBOLS:
        assert hasattr(lib, name), name
        assert name not in chain.ABI_SYMBOLS and name not in chain.DOGLEG_SYMBOLS
    for name in ("log_determinant", "log_noise_normaliser", "log_evidence"):
        assert callable(getattr(gp.ChainSolver, name))
    assert callable(gp.gp_log_normaliser) and callable(gp.evidence_combine)


def test_abi_and_the_old_header_are_untouched():
    lib = gp.load_library()
    lib.gpslam_hip_abi_version.restype = C.c_uint32
    v = lib.gpslam_hip_abi_version()
    assert (v >> 16, v & 0xffff) == (2, 4)
    assert _declared("gpslam_hip.h") == sorted(chain.ABI_SYMBOLS)
    with open(os.path.join(ROOT, "include", "gpslam_hip.h")) as f:
        text = f.read().lower()
    assert "log_determinant" not in text and "evidence" not in text

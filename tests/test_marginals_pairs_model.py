"""The recursion behind gpslam_hip_get_state_pair_marginals in numpy (tests/marginals_pairs_model.py), against np.linalg.inv:
the chunk-of-16 hierarchy in the kernel's [P^-1 | U | V] storage, A^-1_{a,b} of any pair, and both low-rank forms.  CPU only.
Tolerance 1e-11 in correlation units (|dSigma_rc| <= tol sigma_r sigma_c), the tolerance of the other marginals models."""
import numpy as np
import pytest

import marginals_pairs_model as M

TOL = 1e-11
SIZES = [1, 2, 16, 17, 33, 256, 257, 300]


def pair_list(N, rng):
    """every pair up to N = 33; beyond: same chunk, neighbouring chunks, separators, across levels, first-last, and random ones"""
    if N <= 33:
        return [(a, b) for a in range(N) for b in range(N)]
    fixed = [(0, N - 1), (N - 1, 0), (3, 9), (9, 3), (14, 17), (15, 16), (16, 32), (16, 5), (0, 16), (0, 256 if N > 256 else 240),
             (17, 255), (31, 32), (100, 100), (255, N - 1), (1, 2), (240, 255), (239, 241), (16, 48), (47, 48), (5, N - 2)]
    rnd = [tuple(int(v) for v in rng.integers(0, N, 2)) for _ in range(60)]
    return fixed + rnd


@pytest.mark.parametrize("b", [4, 6, 12])
@pytest.mark.parametrize("N", SIZES)
def test_chain_pairs_against_dense_inverse(N, b):
    rng = np.random.default_rng(1000 * b + N)
    D, O = M.random_chain(N, b, rng)
    S = np.linalg.inv(M.dense(D, O))
    sig = np.sqrt(np.diag(S))
    levels, top = M.factor(D, O)
    worst, most = 0.0, 0
    for a, c in pair_list(N, rng):
        cnt = [0]
        got = M.chain_pair(levels, top, a, c, cnt)
        want = S[a * b:(a + 1) * b, c * b:(c + 1) * b]
        worst = max(worst, M.corr_err(got, want, sig[a * b:(a + 1) * b], sig[c * b:(c + 1) * b]))
        most = max(most, cnt[0])
    print("N=%d b=%d: worst %.2e correlation units, at most %d block products" % (N, b, worst, most))
    assert worst <= TOL
    assert most <= 6 * M.CHUNK * max(len(levels), 1) + 2      # 6 per common interior, at most a chunk of them per level


@pytest.mark.parametrize("b", [4, 6, 12])
@pytest.mark.parametrize("N", [2, 17, 33, 300])
@pytest.mark.parametrize("nl,ncr", [(5, 0), (0, 6), (4, 3), (3, 24)])
def test_lowrank_forms_against_dense_inverse(N, b, nl, ncr):
    rng = np.random.default_rng(7 + 1000 * b + N + 31 * nl + ncr)
    D, O, H, Y, K, W, Si, Zp, Mp = M.border_problem(N, b, nl, ncr, rng)
    S = np.linalg.inv(H)
    sig = np.sqrt(np.diag(S))
    levels, top = M.factor(D, O)
    pairs = pair_list(N, rng)[:: max(1, len(pair_list(N, rng)) // 40)]
    worst = 0.0
    for a, c in pairs:
        chain = M.chain_pair(levels, top, a, c) if N > 1 else top
        want = S[a * b:(a + 1) * b, c * b:(c + 1) * b]
        sa, sc = sig[a * b:(a + 1) * b], sig[c * b:(c + 1) * b]
        worst = max(worst, M.corr_err(chain + M.lowrank_single(Y, K, a, c), want, sa, sc))
        worst = max(worst, M.corr_err(chain + M.lowrank_passes(W, Si, Zp, Mp, a, c, b), want, sa, sc))
    print("N=%d b=%d nl=%d ncr=%d: worst %.2e" % (N, b, nl, ncr, worst))
    assert worst <= TOL


def test_transpose_and_symmetry():
    rng = np.random.default_rng(3)
    D, O = M.random_chain(70, 4, rng)
    levels, top = M.factor(D, O)
    S = np.linalg.inv(M.dense(D, O))
    for a, c in [(3, 60), (16, 17), (0, 69), (20, 20)]:
        x, y = M.chain_pair(levels, top, a, c), M.chain_pair(levels, top, c, a)
        assert np.max(np.abs(x - y.T)) <= 1e-13 * np.max(np.abs(S))

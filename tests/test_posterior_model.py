"""The generator of include/gpslam_hip_sampling.h as tests/posterior_model.py restates it, on the CPU: Random123's known answers for
philox4x32-10, the moments of its normals at four fixed seeds, what a draw depends on, and -- the seed of the GPU statistics test checked
here first -- the whitened second moments of model normals pushed through a random orthonormal map of that test's sizes."""
import numpy as np
import pytest

import posterior_model as PM

# Random123 (tests/kat_vectors): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SEEDS = (1, 2, 3, 2026)
N_MOMENTS = 200000
# tests/test_gpu_posterior.py's statistics case: its seed, its number of draws, and the size its whitened vector has on the se2 graph
# with landmarks (states x 6 + landmark coordinates); the GPU test asserts that size
STAT_SEED, STAT_K, STAT_N = 20260, 2048, 90


@pytest.mark.parametrize("ctr,key,out", KAT, ids=["zeros", "ones", "pi"])
def test_known_answers(ctr, key, out):
    got = tuple(int(w[0]) for w in PM.philox4x32_10(ctr, key))
    assert got == out, ["%08x" % w for w in got]


def test_known_answers_as_one_batch():
    ctr = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    for row, (c, key, out) in enumerate(KAT):      # (one key per call: the batch runs over counters)
        got = PM.philox4x32_10(ctr, key)
        assert tuple(int(w[row]) for w in got) == out


@pytest.mark.parametrize("seed", SEEDS)
def test_moments(seed):
    n = N_MOMENTS
    x = PM.noise(seed, 0, 1, n)[0]
    mean, var = x.mean(), x.var()
    print("seed %d: mean %.3g (%.2f sigma), var - 1 %.3g (%.2f sigma), max |eps| %.3f"
          % (seed, mean, abs(mean) * np.sqrt(n), var - 1.0, abs(var - 1.0) / np.sqrt(2.0 / n), np.abs(x).max()))
    assert np.isfinite(x).all()
    assert abs(mean) <= 5.0 / np.sqrt(n)
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n)


def test_a_draw_depends_on_seed_sample_and_index_alone():
    seed, first = (7 << 40) + 11, 2 ** 32 + 3
    a = PM.noise(seed, first, 5, 37)
    for k in range(5):
        assert np.array_equal(a[k], PM.noise(seed, first + k, 1, 37)[0])
    assert np.array_equal(a[:, :20], PM.noise(seed, first, 5, 20))
    # the high words count: another seed above bit 32, another sample above bit 32, are other numbers
    assert not np.array_equal(a, PM.noise(seed + (1 << 40), first, 5, 37))
    assert not np.array_equal(a, PM.noise(seed, first - 2 ** 32, 5, 37))
    assert not np.array_equal(PM.noise(seed, first, 1, 37), PM.noise(seed & 0xFFFFFFFF, first, 1, 37))
    j = np.uint64(2 ** 32 + 5)
    assert PM.normals(seed, np.uint64(0), j) != PM.normals(seed, np.uint64(0), np.uint64(5))


def test_the_extreme_words_stay_finite():
    """u1 is never 0 (the + 0.5), and the largest u1 rounds to 1: eps = 0"""
    k32 = 2.0 ** -32
    w = float(2 ** 32 - 1)
    assert (0.0 + (0.0 + 0.5) * k32) * k32 > 0.0
    assert (w + (w + 0.5) * k32) * k32 == 1.0
    assert np.sqrt(-2.0 * np.log((0.0 + 0.5 * k32) * k32)) < 10.0      # (the values are below 10: 9.42)


def test_the_statistics_seed_on_the_cpu():
    """What the GPU test asks of w = L^T delta, asked here of model normals through a random orthonormal projection of the same
    sizes: w = Q^T eps with Q (n_noise x n) orthonormal is what L^T delta is when the solver is exact."""
    K, n = STAT_K, STAT_N
    n_noise = 3 * n
    eps = PM.noise(STAT_SEED, 0, K, n_noise)
    Q, _ = np.linalg.qr(np.random.default_rng(1).standard_normal((n_noise, n)))
    w = eps @ Q
    bm, bs = PM.moment_bounds(n, K)
    mean, S = w.mean(axis=0), w.T @ w / K
    dev = np.abs(S - np.eye(n)) / (bs / 6.0)
    print("seed %d: mean at most %.2f sigma, second moments at most %.2f sigma" % (STAT_SEED, np.abs(mean).max() * np.sqrt(K), dev.max()))
    assert np.abs(mean).max() <= bm
    assert (np.abs(S - np.eye(n)) <= bs).all()

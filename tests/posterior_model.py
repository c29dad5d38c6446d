"""Posterior sampling (include/gpslam_hip_sampling.h) in plain numpy: the reference side of
tests/test_posterior_*.py and tests/test_gpu_posterior.py.

  philox4x32_10   the block cipher on arrays of counters, in numpy integer arithmetic (uint64 products, masked to 32 bits)
  normals         the generator of the header: one standard normal per (seed, sample index, noise index)
  noise           (count, n_noise): what gpslam_hip_posterior_noise returns
  own_noise       the graph's own whitened residuals in the noise order: rowE of get_rows(), then (l - prior) / sigma
  moment_bounds   the entry-wise six-sigma bounds of the mean and the second-moment matrix of K whitened draws
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four arrays (or scalars) of 32-bit words, key: two.  Returns the four output words as uint64 arrays below 2^32.
    Ten rounds; the key is bumped by the Weyl constants before every round but the first."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = [np.uint64(int(v) & 0xFFFFFFFF) for v in key]
    for r in range(10):
        if r > 0:
            k0 = (k0 + np.uint64(W0)) & MASK
            k1 = (k1 + np.uint64(W1)) & MASK
        p0 = np.uint64(M0) * c[0]        # (< 2^64: both factors are below 2^32)
        p1 = np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> S32, p0 & MASK, p1 >> S32, p1 & MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return c


def normals(seed, s, j):
    """the standard normals of sample indices s and noise indices j (broadcast against each other), key (seed lo, seed hi),
    counter (j lo, j hi, s lo, s hi); u1 = (w0 + (w1 + 0.5) 2^-32) 2^-32, u2 = (w2 + w3 2^-32) 2^-32, sqrt(-2 ln u1) cos(2 pi u2)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = np.asarray(s, dtype=np.uint64)
    j = np.asarray(j, dtype=np.uint64)
    s, j = np.broadcast_arrays(s, j)
    w = philox4x32_10((j & MASK, j >> S32, s & MASK, s >> S32), (seed & 0xFFFFFFFF, seed >> 32))
    w = [v.astype(np.float64) for v in w]
    k32 = 2.0 ** -32
    u1 = (w[0] + (w[1] + 0.5) * k32) * k32
    u2 = (w[2] + w[3] * k32) * k32
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).reshape(s.shape)


def noise(seed, first, count, n_noise):
    """(count, n_noise): sample first + k in row k"""
    s = (np.uint64(int(first) & 0xFFFFFFFFFFFFFFFF) + np.arange(count, dtype=np.uint64))[:, None]
    return normals(seed, s, np.arange(n_noise, dtype=np.uint64)[None, :])


def own_noise(dev, p):
    """the whitened residuals of the handle's current linearisation in the noise order of the header: the rows of get_rows(), then
    the landmark priors of the description p, (l - prior) / sigma each"""
    e = dev.get_rows()[1]
    if "landmarks" in p and len(p.get("lprior_idx", ())):
        lm = dev.get_landmarks()
        idx = np.asarray(p["lprior_idx"], dtype=np.int64)
        r = (lm[idx] - np.asarray(p["lprior"], dtype=np.float64).reshape(len(idx), -1)) / np.asarray(p["lprior_sig"], dtype=np.float64).reshape(len(idx), -1)
        e = np.concatenate([e, r.reshape(-1)])
    return e


def moment_bounds(n, K, sigmas=6.0):
    """(bound of the mean per coordinate, bound of W^T W / K - I entry by entry) for K draws of n independent standard normals: the
    entries' own standard deviations -- 1 / sqrt(K), sqrt((1 + [i = j]) / K) -- times `sigmas`"""
    return sigmas / np.sqrt(K), sigmas * np.sqrt((1.0 + np.eye(n)) / K)

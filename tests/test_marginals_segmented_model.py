"""The algebra of the marginals on the segmented landmark path (tests/marginals_segmented_model.py) against np.linalg.inv of
random SPD systems of that shape: block sizes 4, 6, 12; 2, 3, 5, 6 and 8 cuts (cyclic reductions with odd and even levels, ends
without a right neighbour); unequal segment lengths, an empty segment (two adjacent cuts); fat blocks of 8, 28 and 64 columns.
Bound: 1e-11 in correlation units, that of tests/test_marginals_passes_model.py.  Runs without a GPU and passes on any code: it pins
the signs and the per-level pair bookkeeping the device kernels implement (tests/test_gpu_marginals_segmented.py holds those to
the oracle)."""
import numpy as np
import pytest

import marginals_segmented_model as M


def _cuts(K, rng, with_empty):
    lens = [int(rng.integers(2, 7)) for _ in range(K - 1)]
    if with_empty and K > 2:
        lens[K // 2] = 1                           # two adjacent cut states: a segment without interior
    return [0] + list(np.cumsum(lens))


def test_levels_follow_the_plan():
    lv, top, nlinks = M.levels(6)
    assert [[e[0] for e in lev] for lev in lv] == [[1, 3, 5], [2], [4]] and top == 0
    assert lv[0][2] == (5, 4, -1, 4, -1, -1) and lv[0][0] == (1, 0, 2, 0, 1, 5) and nlinks == 8
    assert M.levels(1) == ([], 0, 1)


# (a fat block holds its cut state: no 8-column block at block size 12)
_CASES = [(b, K, NB) for b in (4, 6, 12) for K in (2, 3, 5, 6, 8) for NB in (8, 28, 64) if NB >= b]


@pytest.mark.parametrize("b,K,NB", _CASES)
def test_selected_inverse_equals_the_dense_inverse(b, K, NB):
    rng = np.random.default_rng(1000 * b + 10 * K + NB)
    cuts = _cuts(K, rng, with_empty=(K in (5, 8)))
    H, sidx, fidx = M.random_system(rng, b, cuts, NB)
    out = M.segmented_marginals(H, b, cuts, sidx, fidx)
    ref = np.linalg.inv(H)
    dg = np.sqrt(np.diag(ref))
    err = 0.0

    def cmp(S_hat, I, J):
        nonlocal err
        err = max(err, float(np.max(np.abs(S_hat - ref[np.ix_(I, J)]) / np.outer(dg[I], dg[J]))))

    N = cuts[-1] + 1
    for i in range(N):
        cmp(out["Sd"][i], sidx[i], sidx[i])
        if i + 1 < N:
            cmp(out["Sn"][i], sidx[i], sidx[i + 1])
    assert not out["Sn"][N - 1].any()
    for k in range(K):
        cmp(out["fat"][k], fidx[k], fidx[k])
        if k + 1 < K:
            cmp(out["fatpair"][k], fidx[k], fidx[k + 1])
    for s in range(K - 1):
        Bs = np.concatenate([fidx[s], fidx[s + 1]])
        for i in range(cuts[s] + 1, cuts[s + 1]):
            cmp(out["sxF"][i], sidx[i], Bs)
    print("b %d K %d NB %d cuts %s: against inv(H) in correlation units %.2e" % (b, K, NB, cuts, err))
    assert err <= 1e-11

"""The numpy model of Powell's dogleg (tests/dogleg_model.py) on its own, on the CPU: what the GPU tests of tests/test_gpu_dogleg.py
take for granted about their graphs and their reference.

 - from perturbed starts of every family the cost never increases and the loop ends at the Gauss-Newton fixed point;
 - g^T H g of every test graph is a sum the float64 and the np.longdouble twin agree on to 1e-8 relative (the cap of the allowance
   the device's number gets), so every graph is a test graph;
 - some family has a blend branch (|du| < |dn|) at its initial states;
 - the lockstep starts: in every mode the model rejects a trial, and none of the first four iterations is undecidable.  DECIDABLE
   records, per start and mode, the iterations before the first undecidable one: the GPU test runs its lockstep over those."""
import functools

import numpy as np
import pytest

import dogleg_model as DM

# (family, with landmarks) of DM.LOCKSTEP -> per mode, the number of leading decidable iterations of the six
DECIDABLE = {("se2", True): (6, 6, 6), ("r3", True): (6, 6, 6)}


@functools.lru_cache(maxsize=None)
def lockstep_run(start, mode):
    return DM.lockstep(*start, mode)


def leading_decidable(run):
    n = 0
    while n < len(run) and run[n]["decidable"]:
        n += 1
    return n


@pytest.mark.parametrize("name,lm,N", DM.FAMILY)
def test_cost_never_increases_and_ends_at_the_gauss_newton_fixed_point(name, lm, N):
    p = DM.perturbed(DM.graph(name, lm, N), 0.3)
    delta, costs = 1.0, [DM.cost(p)]
    for _ in range(12):
        r = DM.iterate(p, delta)
        p, delta = r["p"], r["delta"]
        costs.append(r["error_after"])
    assert all(b <= a for a, b in zip(costs, costs[1:])), costs
    H, gv, arr = DM.system(p)
    dn = DM.gn_step(H, gv, arr)
    print("%s: cost %.6g -> %.6g, |dn|_inf at the end %.3g" % (name, costs[0], costs[-1], np.abs(dn).max()))
    assert np.abs(dn).max() <= 1e-6, np.abs(dn).max()


@pytest.mark.parametrize("name,lm,N", DM.FAMILY + DM.SIZES)
def test_every_graph_is_a_test_graph(name, lm, N):
    H, gv, arr = DM.system(DM.graph(name, lm, N))
    t = DM.twin_distance(arr)
    print("%s N %s: twin distance of g^T H g %.3g" % (name, N, t))
    assert t <= 1e-8
    s4, _ = DM.scalars(H, gv, arr)
    if H is not None:
        assert abs(s4[1] - gv @ (H @ gv)) <= 1e-12 * s4[1]      # the block form IS g^T H g


def test_the_robust_graph_is_a_test_graph():
    H, gv, arr = DM.system(DM.graph(DM.ROBUST, True, robust=True))
    assert DM.twin_distance(arr) <= 1e-8


def test_some_family_has_a_blend():
    have = []
    for name, lm, N in DM.FAMILY:
        H, gv, arr = DM.system(DM.graph(name, lm, N))
        (gg, gHg, gn, nn), _ = DM.scalars(H, gv, arr)
        if gg / gHg * np.sqrt(gg) < np.sqrt(nn):
            have.append(name)
    assert have


@pytest.mark.parametrize("start", DM.LOCKSTEP, ids=lambda s: s[0])
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_lockstep_starts_reject_and_are_decidable(start, mode):
    run = lockstep_run(start, mode)
    n = leading_decidable(run)
    print(start, mode, [(r["trials"], r["rejected"], r["accepted"], r["branch"], r["decidable"]) for r in run])
    assert n >= 4
    assert any(r["rejected"] for r in run[:n])
    assert DECIDABLE[start[:2]][mode] == n


def test_three_trials_start():
    r = DM.lockstep(*DM.THREE_TRIALS, 1, iterations=1)[0]
    assert r["trials"] >= 3

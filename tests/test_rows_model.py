"""tests/rows_model.py on a hand-made graph: 3 states (d = 2), 2 landmarks, every row set of gpslam_hip_get_rows.  The table is
written out here row by row in the documented order; the model's row map must name the same places, and the blocks it assembles
must be J^T J and -J^T e of the dense Jacobian, which is built factor by factor without the map."""
import numpy as np
import pytest

import rows_model as RM

N, D_, LD, L = 3, 2, 2, 2
B_ = 2 * D_
GP_LEFT, VPRI, PRI, BTW = [0, 1], [0, 2], [0, 2], [0, 1]
IR_LEFT, IR_LM = [1, 0, 1], [0, 1, 1]        # interpolated range (two states, one row)
R_IDX, R_LM = [2, 0], [1, 0]                 # range (one state, one row)
LP_IDX, LP_SIG = [0, 1], np.array([[0.5, 0.25], [2.0, 0.1]])
# the table, in the order of include/gpslam_hip.h: (set, factor) per block of rows
FULL = [("gp", 0), ("vpri", 0), (0, 1), (1, 1), ("gp", 1), (0, 0), (0, 2), ("vpri", 1), (1, 0)]
COMPACT = [("pri", 0), ("btw", 0), ("btw", 1), ("pri", 1)]


def factors(seed=0):
    """per factor: (left state, two_states, landmark or -1, JL, JR, Jm, e), rows drawn at random in each factor's sparsity"""
    rng = np.random.default_rng(seed)
    f = {}

    def put(key, k, left, rows, two, lm=-1, vel=True):
        JL, JR = rng.standard_normal((rows, B_)), rng.standard_normal((rows, B_)) * (1.0 if two else 0.0)
        if not vel:
            JL[:, D_:] = 0.0
            JR[:, D_:] = 0.0
        Jm = rng.standard_normal((rows, LD)) if lm >= 0 else np.zeros((rows, LD))
        f[(key, k)] = (left, two, lm, JL, JR, Jm, rng.standard_normal(rows))
    for k, s in enumerate(GP_LEFT):
        put("gp", k, s, B_, True)
    for k, s in enumerate(VPRI):
        put("vpri", k, s, D_, False)
    for k, s in enumerate(PRI):
        put("pri", k, s, D_, False, vel=False)
    for k, s in enumerate(BTW):
        put("btw", k, s, D_, True, vel=False)
    for k, (s, l) in enumerate(zip(IR_LEFT, IR_LM)):
        put(0, k, s, 1, True, l)
    for k, (s, l) in enumerate(zip(R_IDX, R_LM)):
        put(1, k, s, 1, False, l)
    return f


def table(f, order):
    LR = np.vstack([np.hstack([f[k][3], f[k][4]]) for k in order])
    E = np.concatenate([f[k][6] for k in order])
    Mm = np.vstack([f[k][5] for k in order])
    Lm = np.concatenate([np.full(len(f[k][6]), f[k][2]) for k in order]).astype(np.int32)
    return LR, E, Mm, Lm


def dense_J(f):
    nx = N * B_
    J, e = [], []
    for left, two, lm, JL, JR, Jm, ee in f.values():
        r = np.zeros((len(ee), nx + L * LD))
        r[:, left * B_:(left + 1) * B_] = JL
        if two:
            r[:, (left + 1) * B_:(left + 2) * B_] = JR
        if lm >= 0:
            r[:, nx + lm * LD:nx + (lm + 1) * LD] = Jm
        J.append(r)
        e.append(ee)
    for k, l in enumerate(LP_IDX):          # the landmark priors: I / sigma, no row in the tables
        r = np.zeros((LD, nx + L * LD))
        r[:, nx + l * LD:nx + (l + 1) * LD] = np.diag(1.0 / LP_SIG[k])
        J.append(r)
        e.append(np.zeros(LD))
    return np.vstack(J), np.concatenate(e)


def the_map():
    return RM.row_map(N, D_, GP_LEFT, VPRI, PRI, BTW, {0: IR_LEFT, 1: R_IDX})


def test_row_map_places_every_factor_where_the_header_says():
    m = the_map()
    f = factors()
    at = 0
    for key, k in FULL + COMPACT:
        assert m.row0[key][k] == at, (key, k)
        rows = len(f[(key, k)][6])
        assert rows == m.rows[key]
        assert (m.left[at:at + rows] == f[(key, k)][0]).all(), (key, k)
        at += rows
    assert (m.M, m.Mc, at) == (4 + 2 + 1 + 1 + 4 + 1 + 1 + 2 + 1, 8, 25)
    assert list(m.rows_of(0)) == [m.row0[0][0], m.row0[0][1], m.row0[0][2]] and list(m.rows_of("gp", 1)) == [8, 9, 10, 11]


def test_assembled_blocks_are_jtj_of_the_dense_jacobian():
    f = factors()
    J, e = dense_J(f)
    H, grad = J.T @ J, -J.T @ e
    D, O, g, Bm, HLL, gL = RM.assemble(N, B_, the_map().left, *table(f, FULL + COMPACT), L=L, ld=LD, lprior=(LP_IDX, LP_SIG))
    nx = N * B_
    assert np.abs(RM.dense(D, O, Bm, HLL) - H).max() <= 1e-13 * np.abs(H).max()
    assert np.abs(np.concatenate([g.ravel(), gL]) - grad).max() <= 1e-13 * np.abs(grad).max()
    for i in range(N - 1):
        assert np.abs(O[i] - H[(i + 1) * B_:(i + 2) * B_, i * B_:(i + 1) * B_]).max() <= 1e-13      # O[i] = H[i+1, i]
    assert np.abs(Bm.reshape(nx, -1) - H[:nx, nx:]).max() <= 1e-13 and not O[N - 1].any()


def test_a_misplaced_row_lands_in_the_wrong_block():
    """the check bites: two rows of different left states exchanged, or one landmark id changed, moves the blocks by O(1)"""
    f = factors()
    J, _ = dense_J(f)
    H = J.T @ J
    LR, E, Mm, Lm = table(f, FULL + COMPACT)
    left = the_map().left
    swap = np.arange(len(E))
    swap[[7, 8]] = [8, 7]                    # the last row of state 0 and the first of state 1
    D, O, _, Bm, HLL, _ = RM.assemble(N, B_, left, LR[swap], E[swap], Mm[swap], Lm[swap], L=L, ld=LD, lprior=(LP_IDX, LP_SIG))
    assert np.abs(RM.dense(D, O, Bm, HLL) - H).max() > 0.1
    Lm2 = Lm.copy()
    Lm2[6] = 1 - Lm2[6]
    D, O, _, Bm, HLL, _ = RM.assemble(N, B_, left, LR, E, Mm, Lm2, L=L, ld=LD, lprior=(LP_IDX, LP_SIG))
    assert np.abs(RM.dense(D, O, Bm, HLL) - H).max() > 0.1


def test_factor_lists_record_replay_and_count():
    fl = RM.FactorLists(D_, LD)
    fl.set_states(np.zeros((N, D_)), np.zeros((N, D_)))
    fl.set_landmarks(np.zeros((L, LD)))
    fl.add_gp_priors(GP_LEFT, [0.1, 0.1])
    fl.add_pose_priors(PRI, np.zeros((2, D_)), np.ones((2, D_)))
    fl.add_vel_priors(VPRI, np.zeros((2, D_)), np.ones((2, D_)))
    fl.add_between(BTW, np.zeros((2, D_)), np.ones((2, D_)))
    fl.add_landmark_priors(LP_IDX, np.zeros((L, LD)), LP_SIG)
    fl.add_interp_range(IR_LEFT, IR_LM, np.ones(3), np.ones(3), np.full(3, 0.1), np.full(3, 0.05), None)
    fl.add_range(R_IDX, R_LM, np.ones(2), np.ones(2))
    fl.compile()
    m, ref = fl.row_map(), the_map()
    assert (m.left == ref.left).all() and all((m.row0[k] == ref.row0[k]).all() for k in ref.row0)
    assert fl.n_rows() == 25 == len(m.left)
    got = RM.FactorLists(D_, LD)
    fl.replay(got, edit=lambda name, a: (a[0] + 1.0, a[1]) if name == "set_states" else a)
    assert [n for n, _ in got.calls] == [n for n, _ in fl.calls]
    assert (got.args_of("set_states")[0][0] == 1.0).all() and (fl.args_of("set_states")[0][0] == 0.0).all()
    with pytest.raises(AttributeError):
        fl.iterate_gn


def test_scaled_condition_number_and_tolerance_rule():
    H = np.diag([1.0, 1e8]) + np.array([[0.0, 1e3], [1e3, 0.0]])
    s = RM.jacobi_scale(H)
    assert np.allclose(s, [1.0, 1e4])
    assert abs(RM.scaled_cond(H) - 1.1 / 0.9) < 1e-12          # [[1, .1], [.1, 1]]
    assert RM.step_tol(H) == 1e-10
    with pytest.raises(AssertionError):
        RM.step_tol(np.array([[1.0, 1 - 1e-10], [1 - 1e-10, 1.0]]))

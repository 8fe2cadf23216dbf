"""A grouped Levenberg-Marquardt fit without the integrator, in the pattern of tests/test_lm_fit_analytic.py: the members' fits are computed in numpy, then plh_lsq_group,
plh_lm_step (on the groups) and plh_group_scatter run in a short host loop (wave-emulator build, host pointers).

The model is y = a exp(-b t) with both keys LOG.  A group has two members: member A saw the single datum at t = 0, member B the single datum at t = 1.  Neither identifies
(a, b) -- each member's JtJ has rank 1 --, the group does.  Every group sum is compared bit for bit with the restatement of tests/lsq_group_cases.py, every step is replayed
through lm_cases.step_reference with the inputs the kernel saw and held to lm_cases' bounds, and the number of iterations is that of the restatements' own run."""
import numpy as np

import lm_cases as lm
import lsq_group_cases as gc

NG, M = 8, 2
N = NG * M
MAX_ITER = 30
A_TRUE, B_TRUE = 2.0, 1.3
T_MEMBER = np.tile([0.0, 1.0], NG)                                       # the time of every cell's datum
Y_MEMBER = A_TRUE * np.exp(-B_TRUE * T_MEMBER)
OFF = gc.offsets([M] * NG)
# (as in test_lm_fit_analytic.py: the data are exact, the steps square near the solution, so a step test at 1e-14 is decided far from its threshold; the other two are off)
TIGHT = dict(xtol=1e-14, gtol=0.0, ftol=0.0)


def member_fits(x):
    """x [N, 2] = (a, b) of every cell -> cost [N], grad [N, 2], JtJ [N, 2, 2] of its one datum"""
    cost, grad, JtJ = np.empty(N), np.empty((N, 2)), np.empty((N, 2, 2))
    for c in range(N):
        e = np.exp(-x[c, 1] * T_MEMBER[c])
        r = np.array([x[c, 0] * e - Y_MEMBER[c]])
        J = np.array([[e, -x[c, 0] * T_MEMBER[c] * e]])
        cost[c], grad[c], JtJ[c] = 0.5 * r @ r, J.T @ r, J.T @ J
    return cost, grad, JtJ


def starts(seed):
    r = np.random.default_rng(seed)
    theta = np.ascontiguousarray(r.uniform(0.5, 2.0, size=(N, 4)))
    cols = np.array([3, 1], np.int32)
    theta[:, cols] = np.array([A_TRUE, B_TRUE]) * 2.0 ** r.uniform(-0.5, 0.5, size=(N, 2))      # the members of a group disagree: the first member's values count
    return theta, cols


def test_two_members_with_one_datum_each_identify_both_keys(emu_model):
    theta, cols = starts(11)
    theta0 = theta.copy()
    tf = np.array([lm.LOG, lm.LOG], np.int32)
    # each member alone cannot be fitted: its JtJ has rank 1
    _, _, H = member_fits(theta[:, cols])
    assert all(np.linalg.matrix_rank(H[c]) == 1 for c in range(N))

    # ---- the kernels, every call checked against the restatements
    g_theta = np.ascontiguousarray(theta[OFF[:-1]])
    assert gc.call_scatter(emu_model, OFF, cols, g_theta, theta) == 0
    assert theta.tobytes() == gc.scatter_reference(OFF, cols, g_theta, theta0).tobytes()
    st = lm.State(NG, 2)
    for it in range(MAX_ITER + 1):
        phase = lm.FIRST if it == 0 else lm.LAST if it == MAX_ITER else lm.STEP
        cost, grad, JtJ = member_fits(theta[:, cols])
        out = gc.sum_outputs(NG, 2)
        assert gc.call_sum(emu_model, OFF, cost, grad, JtJ, None, out) == 0, emu_model._lib.plh_last_error()
        ref_sum = gc.sum_reference(OFF, cost, grad, JtJ, None)
        for a, b in zip((out["g_cost"], out["g_grad"], out["g_JtJ"]), ref_sum):
            assert gc.same_bits_nan(a, b), it
        if it == 0:
            assert all(np.linalg.matrix_rank(out["g_JtJ"][g]) == 2 for g in range(NG))
        ref, _ = lm.run(emu_model, g_theta, cols, tf, None, None, out["g_cost"], out["g_grad"], out["g_JtJ"], out["g_status"], st, phase, TIGHT, "grouped decay it %d" % it)
        before = theta.copy()
        assert gc.call_scatter(emu_model, OFF, cols, g_theta, theta) == 0
        assert theta.tobytes() == gc.scatter_reference(OFF, cols, g_theta, before).tobytes()
        if ref[2] == 0:
            break
    iters = it + 1

    # ---- the same loop with the restatements alone
    th_r = gc.scatter_reference(OFF, cols, theta0[OFF[:-1]], theta0)
    g_r, st_r = np.ascontiguousarray(theta0[OFF[:-1]]), lm.State(NG, 2)
    for it in range(MAX_ITER + 1):
        phase = lm.FIRST if it == 0 else lm.LAST if it == MAX_ITER else lm.STEP
        c, g, H, s = gc.sum_reference(OFF, *member_fits(th_r[:, cols]), None)
        g_r, st_r, nrun, _ = lm.step_reference(g_r, cols, tf, None, None, c, g, H, s, st_r, phase, TIGHT)
        th_r = gc.scatter_reference(OFF, cols, g_r, th_r)
        if nrun == 0:
            break
    iters_ref = it + 1

    print("grouped decay: %d iterations (the restatements on their own: %d), states %s, costs %s" % (iters, iters_ref, st.state.tolist(), st.cost_cur.tolist()))
    assert iters == iters_ref <= MAX_ITER and np.array_equal(st.state, st_r.state)
    assert np.isin(st.state, (lm.CONV_F, lm.CONV_X, lm.CONV_G)).all()
    assert (np.abs(theta[:, cols] / np.array([A_TRUE, B_TRUE]) - 1) <= 1e-8).all()
    # the members of a group hold the group's best point, bit for bit; nothing else of theta moved
    assert np.ascontiguousarray(theta[:, cols]).tobytes() == np.repeat(st.theta_cur, M, axis=0).tobytes()
    other = [0, 2]
    assert np.ascontiguousarray(theta[:, other]).tobytes() == np.ascontiguousarray(theta0[:, other]).tobytes()

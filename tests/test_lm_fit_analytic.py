"""The whole Levenberg-Marquardt loop without the integrator: a short host loop calls plh_lm_step (wave-emulator build, host pointers) with cost / grad / JtJ computed in numpy
for problems with known answers.  Every step of every run is replayed through lm_cases.step_reference with the inputs the kernel saw (teacher forcing: rounding cannot make
the two trajectories drift apart) and held to lm_cases' bounds; the number of iterations is compared with a run of the restatement on its own."""
import numpy as np

import lm_cases as lm

N = 8
MAX_ITER = 30


def drive(model, fit, theta, cols, tf, lo=None, hi=None, opts=None, what=""):
    """FIRST, STEPs, LAST at iteration MAX_ITER; returns (state, number of fits consumed).  theta is advanced in place"""
    n, k = theta.shape[0], len(cols)
    st = lm.State(n, k)
    for it in range(MAX_ITER + 1):
        phase = lm.FIRST if it == 0 else lm.LAST if it == MAX_ITER else lm.STEP
        cost, grad, JtJ = fit(theta[:, cols])
        ref, _ = lm.run(model, theta, cols, tf, lo, hi, cost, grad, JtJ, None, st, phase, opts, "%s it %d" % (what, it))
        if ref[2] == 0:
            break
    return st, it + 1


def drive_reference(fit, theta, cols, tf, lo=None, hi=None, opts=None):
    """the same loop with the restatement alone"""
    theta, st = theta.copy(), lm.State(theta.shape[0], len(cols))
    for it in range(MAX_ITER + 1):
        phase = lm.FIRST if it == 0 else lm.LAST if it == MAX_ITER else lm.STEP
        cost, grad, JtJ = fit(theta[:, cols])
        theta, st, nrun, _ = lm.step_reference(theta, cols, tf, lo, hi, cost, grad, JtJ, None, st, phase, opts)
        if nrun == 0:
            break
    return theta, st, it + 1


def from_residuals(res_jac):
    def fit(x):
        n, k = x.shape
        cost, grad, JtJ = np.empty(n), np.empty((n, k)), np.empty((n, k, k))
        for c in range(n):
            r, J = res_jac(x[c])
            cost[c], grad[c], JtJ[c] = 0.5 * r @ r, J.T @ r, J.T @ J
        return cost, grad, JtJ
    return fit


T = np.linspace(0.0, 2.0, 10)
A_TRUE, B_TRUE = 2.0, 1.3
Y = A_TRUE * np.exp(-B_TRUE * T)


def decay(x):
    e = np.exp(-x[1] * T)
    return x[0] * e - Y, np.stack([e, -x[0] * T * e], axis=1)


def starts(seed, centre, spread=0.5, extra=2):
    r = np.random.default_rng(seed)
    theta = np.ascontiguousarray(r.uniform(0.5, 2.0, size=(N, 2 + extra)))
    cols = np.array([3, 1], np.int32)
    theta[:, cols] = np.asarray(centre) * 2.0 ** r.uniform(-spread, spread, size=(N, 2))
    return theta, cols


# (the defaults stop at a step of 1e-8, that is at a cost near 1e-16: this test asks for 1e-20.  Near the solution the steps square from iteration to iteration -- 1e-3, 1e-6,
#  1e-11, then rounding --, so a step test at 1e-14 is decided far from its threshold; the other two tests are off: at a cost of 1e-25 they would be decided by rounding)
TIGHT = dict(xtol=1e-14, gtol=0.0, ftol=0.0)


def test_exponential_decay_exact_data_log_keys(emu_model):
    theta, cols = starts(1, (A_TRUE, B_TRUE))
    tf = np.array([lm.LOG, lm.LOG], np.int32)
    theta0 = theta.copy()
    st, iters = drive(emu_model, from_residuals(decay), theta, cols, tf, opts=TIGHT, what="decay")
    th_ref, st_ref, iters_ref = drive_reference(from_residuals(decay), theta0, cols, tf, opts=TIGHT)
    print("decay: %d iterations (the restatement on its own: %d), states %s, costs %s" % (iters, iters_ref, st.state.tolist(), st.cost_cur.tolist()))
    assert iters == iters_ref <= MAX_ITER and np.array_equal(st.state, st_ref.state)
    assert np.isin(st.state, (lm.CONV_F, lm.CONV_X, lm.CONV_G)).all()
    assert (st.cost_cur < 1e-20).all()
    assert (np.abs(theta[:, cols] / np.array([A_TRUE, B_TRUE]) - 1) <= 1e-8).all()
    assert lm.same_bits(np.ascontiguousarray(theta[:, cols]), st.theta_cur)
    other = [0, 2]
    assert lm.same_bits(np.ascontiguousarray(theta[:, other]), np.ascontiguousarray(theta0[:, other]))


def test_exponential_decay_with_the_truth_outside_a_bound(emu_model):
    from scipy.optimize import least_squares
    hi_b = 1.0
    theta, cols = starts(2, (A_TRUE, 0.8), spread=0.3)
    theta[:, cols[1]] = np.minimum(theta[:, cols[1]], 0.99)
    tf = np.array([lm.LOG, lm.LOG], np.int32)
    lo, hi = np.array([1e-3, 1e-3]), np.array([1e3, hi_b])
    st, iters = drive(emu_model, from_residuals(decay), theta, cols, tf, lo, hi, what="bounded decay")
    sol = least_squares(lambda x: decay(x)[0], [1.0, 0.5], jac=lambda x: decay(x)[1], bounds=([1e-3, 1e-3], [1e3, hi_b]), xtol=1e-15, ftol=1e-15, gtol=1e-15)
    print("bounded decay: %d iterations, states %s, a = %s, scipy %r" % (iters, st.state.tolist(), theta[:, cols[0]].tolist(), sol.x.tolist()))
    assert iters <= MAX_ITER and np.isin(st.state, (lm.CONV_G, lm.CONV_X)).all()
    assert (theta[:, cols[1]] == hi_b).all()
    assert abs(sol.x[1] - hi_b) <= 1e-9
    assert (np.abs(theta[:, cols[0]] / sol.x[0] - 1) <= 1e-6).all()


def rosenbrock(x):
    return np.array([10.0 * (x[1] - x[0] * x[0]), 1.0 - x[0]]), np.array([[-20.0 * x[0], 10.0], [-1.0, 0.0]])


def test_rosenbrock_shows_rejections(emu_model):
    r = np.random.default_rng(3)
    theta = np.ascontiguousarray(r.uniform(0.5, 2.0, size=(N, 4)))
    cols = np.array([2, 0], np.int32)
    theta[:, cols] = np.array([-1.2, 1.0]) + r.uniform(-0.3, 0.3, size=(N, 2))
    tf = np.zeros(2, np.int32)
    theta0 = theta.copy()
    st, iters = drive(emu_model, from_residuals(rosenbrock), theta, cols, tf, what="rosenbrock")
    th_ref, st_ref, iters_ref = drive_reference(from_residuals(rosenbrock), theta0, cols, tf)
    print("rosenbrock: %d iterations, states %s, rejections %s (the restatement: %s)" % (iters, st.state.tolist(), st.n_reject.tolist(), st_ref.n_reject.tolist()))
    assert (st.n_reject > 0).any() and np.array_equal(st.n_reject, st_ref.n_reject) and np.array_equal(st.n_accept, st_ref.n_accept) and iters == iters_ref
    conv = np.isin(st.state, (lm.CONV_F, lm.CONV_X, lm.CONV_G))
    assert conv.any() and (np.abs(theta[conv][:, cols] - 1.0) <= 1e-6).all()

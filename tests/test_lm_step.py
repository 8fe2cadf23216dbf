"""plh_lm_step on the wave-emulator build of the device source (no GPU), host pointers, against the numpy restatement of the header's definition (tests/lm_cases.py: the
restatement, the derivation of the bounds, the near-tie rule).  Every call is made from the same inputs by the kernel and by the restatement; lm_cases.compare holds the
checks every call gets: integers, lambda and the copies exact, the trial and pred within the bounds, cells that were done and theta columns outside cols bitwise untouched."""
import numpy as np
import pytest

import lm_cases as lm

KS = (1, 2, 3, 8)
N = 16                                                                   # less than one wave
N_BIG = 70                                                               # a second block with a partial wave


def start(model, n, k, seed, transform=None, lo=None, hi=None, opts=None, cost_scale=1.0, fit=None):
    """FIRST on good starts: the context the chains go on from"""
    theta, cols = lm.make_theta(n, k, seed)
    tf = np.zeros(k, np.int32) if transform is None else np.asarray(transform, np.int32)
    cost, grad, JtJ = fit or lm.make_fit(n, k, seed + 1, cost_scale=cost_scale)
    st = lm.State(n, k)
    ref, worst = lm.run(model, theta, cols, tf, lo, hi, cost, grad, JtJ, np.zeros(n, np.int32), st, lm.FIRST, opts, "FIRST k=%d" % k)
    return dict(theta=theta, cols=cols, tf=tf, lo=lo, hi=hi, st=st, fit=(cost, grad, JtJ), ref=ref, opts=opts, n=n, k=k, seed=seed)


def step(model, cx, cost, grad, JtJ, status=None, phase=lm.STEP, what="STEP"):
    cx["ref"], worst = lm.run(model, cx["theta"], cx["cols"], cx["tf"], cx["lo"], cx["hi"], cost, grad, JtJ, status, cx["st"], phase, cx["opts"], "%s k=%d" % (what, cx["k"]))
    return cx["ref"]


def judged_fit(cx, kinds, seed):
    """a fit for the trial of every cell: 'accept' (the cost falls by half of pred), 'reject' (it rises by pred), 'failed' (status 1, cost NaN), 'nan_grad'"""
    n, k, st = cx["n"], cx["k"], cx["st"]
    cost, grad, JtJ = lm.make_fit(n, k, seed)
    target = np.where(np.array([x in ("accept", "nan_grad") for x in kinds]), st.cost_cur - 0.5 * st.pred, st.cost_cur + st.pred)
    target = np.where(st.state == lm.RUNNING, target, 1.0)               # (cells that are done: any fit, it is not looked at)
    assert (target > 0).all()
    cost, grad, JtJ = lm.with_cost(cost, grad, JtJ, target)
    status = np.zeros(n, np.int32)
    for c, x in enumerate(kinds):
        if x == "failed":
            status[c], cost[c] = 1, np.nan
        if x == "nan_grad":
            grad[c, k - 1] = np.nan
    return cost, grad, JtJ, status


@pytest.mark.parametrize("k", KS)
def test_first_on_a_good_start_and_the_restatement_share(emu_model, k):
    cx = start(emu_model, N, k, 10 + k)
    theta_ref, st_ref, nrun, infos = cx["ref"]
    assert nrun == N and (cx["st"].state == lm.RUNNING).all() and (cx["st"].lam == lm.OPTS["lambda0"]).all() and (cx["st"].n_accept == 0).all() and (cx["st"].n_reject == 0).all()
    cost, grad, JtJ = cx["fit"]
    assert lm.same_bits(cx["st"].cost_cur, cost) and lm.same_bits(cx["st"].grad_cur, grad) and lm.same_bits(cx["st"].JtJ_cur, JtJ)
    assert all(i["condA"] <= 1e6 for i in infos)
    share = max(lm.restatement_share(i, k) for i in infos)
    print("k = %d: the restatement's solve sits at %.3g of the bound against numpy.longdouble" % (k, share))
    assert share <= lm.RESTATEMENT_SHARE


def test_first_on_bad_starts(emu_model):
    k, n = 3, N
    theta, cols = lm.make_theta(n, k, 21)
    tf = np.array([lm.LINEAR, lm.LOG, lm.LINEAR], np.int32)
    cost, grad, JtJ = lm.make_fit(n, k, 22)
    status = np.zeros(n, np.int32)
    lo, hi = np.full((n, k), 0.1), np.full((n, k), 5.0)
    status[1] = 1
    cost[2] = np.nan
    theta[3, cols[0]] = 7.0                                              # outside [lo, hi]
    theta[4, cols[1]] = -0.5; lo[4, 1] = -1.0                            # <= 0 under LOG, inside its bounds
    lo[5, 2], hi[5, 2] = 3.0, 0.2                                        # per-cell lo > hi
    JtJ[6, 0, 2] = np.inf                                                # (upper triangle)
    theta[7, cols[2]] = np.nan
    bad = [1, 2, 3, 4, 5, 6, 7]
    st, theta0 = lm.State(n, k), theta.copy()
    ref, _ = lm.run(emu_model, theta, cols, tf, lo, hi, cost, grad, JtJ, status, st, lm.FIRST, None, "bad starts")
    assert (st.state[bad] == lm.FAILED_START).all() and (np.delete(st.state, bad) == lm.RUNNING).all() and ref[2] == n - len(bad)
    assert lm.same_bits(theta[bad], theta0[bad])


@pytest.mark.parametrize("k", KS)
def test_step_accept_reject_and_failed_trials(emu_model, k):
    cx = start(emu_model, N, k, 30 + k)
    kinds = [("accept", "reject", "failed", "nan_grad")[c % 4] for c in range(N)]
    before = cx["st"].copy()
    cost, grad, JtJ, status = judged_fit(cx, kinds, 40 + k)
    theta_ref, st_ref, nrun, infos = step(emu_model, cx, cost, grad, JtJ, status)
    st = cx["st"]
    for c, x in enumerate(kinds):
        assert infos[c]["judged"] == ("accept" if x == "accept" else "reject"), (c, x)
        if x == "accept":
            assert st.n_accept[c] == 1 and st.n_reject[c] == 0 and st.cost_cur[c] == cost[c] and st.lam[c] == max(before.lam[c] * lm.OPTS["lambda_down"], lm.OPTS["lambda_min"])
        else:
            assert st.n_accept[c] == 0 and st.n_reject[c] == 1 and st.lam[c] == before.lam[c] * lm.OPTS["lambda_up"]
            for a in ("theta_cur", "cost_cur", "grad_cur", "JtJ_cur"):
                assert lm.same_bits(getattr(st, a)[c], getattr(before, a)[c])
        assert st.state[c] == lm.RUNNING
    # a second rejection everywhere: the theta row among cols returns to cur bitwise when nothing can be proposed (LAST)
    cost, grad, JtJ, status = judged_fit(cx, ["reject"] * N, 50 + k)
    step(emu_model, cx, cost, grad, JtJ, status, phase=lm.LAST, what="LAST, all rejected")
    assert (st.state == lm.MAXIT).all() and lm.same_bits(np.ascontiguousarray(cx["theta"][:, cx["cols"]]), st.theta_cur)


def test_stalled_when_lambda_passes_lambda_max(emu_model):
    k = 2
    opts = dict(lambda_up=10.0, lambda_max=0.3)                          # 1e-3 -> 1e-2, 1e-1, 1: no value within a factor 2 of lambda_max
    cx = start(emu_model, N, k, 61, opts=opts)
    for it in range(3):
        cost, grad, JtJ, status = judged_fit(cx, ["reject"] * N, 62 + it)
        theta_ref, st_ref, nrun, infos = step(emu_model, cx, cost, grad, JtJ, status, what="reject %d" % it)
        assert (cx["st"].state == (lm.STALLED if it == 2 else lm.RUNNING)).all() and nrun == (0 if it == 2 else N)
    assert lm.same_bits(np.ascontiguousarray(cx["theta"][:, cx["cols"]]), cx["st"].theta_cur) and (cx["st"].n_reject == 3).all()


@pytest.mark.parametrize("tf", ([lm.LOG], [lm.LOG, lm.LINEAR, lm.LOG], [lm.LINEAR, lm.LOG, lm.LOG, lm.LINEAR, lm.LOG, lm.LINEAR, lm.LINEAR, lm.LOG]))
def test_transforms(emu_model, tf):
    k = len(tf)
    cx = start(emu_model, N, k, 70 + k, transform=tf, cost_scale=1e-6)   # (small residuals: steps below 1 in ln theta)
    assert all(i["moved"].all() and i["condA"] <= 1e6 for i in cx["ref"][3])
    cost, grad, JtJ, status = judged_fit(cx, ["accept", "reject"] * (N // 2), 75 + k)
    step(emu_model, cx, cost, grad, JtJ, status)


def test_active_set(emu_model):
    k, n = 3, N
    theta, cols = lm.make_theta(n, k, 81)
    tf = np.array([lm.LINEAR, lm.LOG, lm.LINEAR], np.int32)
    cost, grad, JtJ = lm.make_fit(n, k, 82, cost_scale=1e-6)
    st = lm.State(n, k)
    free_ref = lm.step_reference(theta, cols, tf, None, None, cost, grad, JtJ, None, st, lm.FIRST)      # where the unbounded step goes
    lo, hi = np.full((n, k), -np.inf), np.full((n, k), np.inf)
    out = np.arange(n) % 2 == 0                                          # even cells: the gradient pushes key 0 outward at lo; odd cells: inward
    lo[:, 0] = theta[:, cols[0]]
    grad[:, 0] = np.where(out, np.abs(grad[:, 0]), -np.abs(grad[:, 0]))
    for c in range(n):                                                   # key 2 overshoots a bound put half way along its unbounded step
        t0, t1 = theta[c, cols[2]], free_ref[0][c, cols[2]]
        (hi if t1 > t0 else lo)[c, 2] = t0 + 0.5 * (t1 - t0)
    theta0 = theta.copy()
    ref, _ = lm.run(emu_model, theta, cols, tf, lo, hi, cost, grad, JtJ, None, st, lm.FIRST, None, "active set")
    infos = ref[3]
    for c in range(n):
        assert infos[c]["held"][0] == out[c]
        if out[c]:
            assert theta[c, cols[0]] == theta0[c, cols[0]]
        else:
            assert theta[c, cols[0]] > theta0[c, cols[0]]
    hit = [c for c in range(n) if infos[c]["clamped"][2]]
    assert len(hit) >= n // 4                                            # (the reduced / regrouped solve need not overshoot everywhere)
    for c in hit:
        b = hi[c, 2] if np.isfinite(hi[c, 2]) else lo[c, 2]
        assert theta[c, cols[2]] == b


def test_singular_jtj_a_parameter_the_data_do_not_see(emu_model):
    k, n = 3, N
    c2, g2, H2 = lm.make_fit(n, 2, 91)
    grad, JtJ = np.zeros((n, k)), np.zeros((n, k, k))
    grad[:, [0, 2]] = g2
    JtJ[np.ix_(range(n), [0, 2], [0, 2])] = H2
    cx = start(emu_model, n, k, 92, fit=(c2, grad, JtJ))
    for i in cx["ref"][3]:
        assert i["moved"].tolist() == [True, False, True] and i["raises"] == 0
    assert (cx["st"].state == lm.RUNNING).all()


def test_indefinite_h_raises_lambda_inside_the_call(emu_model):
    k, n = 3, N
    cost, grad, JtJ = lm.make_fit(n, k, 101)
    JtJ = JtJ - 1e-3 * np.eye(k)                                         # (eigenvalues 1, 1e-2, 1e-4 - 1e-3)
    cx = start(emu_model, n, k, 102, fit=(cost, grad, JtJ))
    raises = [i["raises"] for i in cx["ref"][3]]
    print("raises of lambda per cell:", raises)
    assert min(raises) >= 1 and max(raises) < lm.MAX_TRIES and (cx["st"].state == lm.RUNNING).all()
    assert np.array_equal(cx["st"].lam, lm.OPTS["lambda0"] * lm.OPTS["lambda_up"] ** np.array(raises, float)) or \
        all(cx["st"].lam[c] == np.prod([lm.OPTS["lambda0"]] + [lm.OPTS["lambda_up"]] * r) for c, r in enumerate(raises))


def test_conv_f_conv_x_conv_g(emu_model):
    k = 3
    # CONV_F: an accepted step that lowers the cost by 1e-3 of it, with ftol = 1e-2
    cx = start(emu_model, N, k, 111, opts=dict(ftol=1e-2))
    cost, grad, JtJ = lm.with_cost(*lm.make_fit(N, k, 112), cx["st"].cost_cur * (1 - 1e-3))
    trial = cx["theta"][:, cx["cols"]].copy()
    ref = step(emu_model, cx, cost, grad, JtJ, what="CONV_F")
    assert (cx["st"].state == lm.CONV_F).all() and ref[2] == 0 and lm.same_bits(cx["st"].theta_cur, trial) and lm.same_bits(np.ascontiguousarray(cx["theta"][:, cx["cols"]]), trial)
    # CONV_X: every step is below xtol = 1e6
    theta0, _ = lm.make_theta(N, k, 113)
    cx = start(emu_model, N, k, 113, opts=dict(xtol=1e6))
    assert (cx["st"].state == lm.CONV_X).all() and lm.same_bits(cx["theta"], theta0) and (cx["st"].pred == 0).all()
    # CONV_G: a gradient 1e-12 of the usual one; and cost_cur == 0
    cost, grad, JtJ = lm.make_fit(N, k, 115)
    grad *= 1e-12
    cost[::2], grad[::2] = 0.0, 0.0
    cx = start(emu_model, N, k, 114, fit=(cost, grad, JtJ))
    assert (cx["st"].state == lm.CONV_G).all() and lm.same_bits(np.ascontiguousarray(cx["theta"][:, cx["cols"]]), cx["st"].theta_cur)


def test_last(emu_model):
    k = 2
    cx = start(emu_model, N, k, 121)
    kinds = ["accept", "reject"] * (N // 2)
    cost, grad, JtJ, status = judged_fit(cx, kinds, 122)
    trial, cur = cx["theta"][:, cx["cols"]].copy(), cx["st"].theta_cur.copy()
    ref = step(emu_model, cx, cost, grad, JtJ, status, phase=lm.LAST, what="LAST")
    assert (cx["st"].state == lm.MAXIT).all() and ref[2] == 0
    now = cx["theta"][:, cx["cols"]]
    assert lm.same_bits(np.ascontiguousarray(now[::2]), np.ascontiguousarray(trial[::2])) and lm.same_bits(np.ascontiguousarray(now[1::2]), np.ascontiguousarray(cur[1::2]))
    assert (cx["st"].n_accept == np.array([1, 0] * (N // 2))).all()


def test_bitwise_isolation_over_a_chain_of_70_cells(emu_model):
    k, n = 8, N_BIG
    theta, cols = lm.make_theta(n, k, 131)
    tf = np.array([lm.LOG, lm.LINEAR] * 4, np.int32)
    cost, grad, JtJ = lm.make_fit(n, k, 132, cost_scale=1e-6)
    status = np.zeros(n, np.int32)
    status[[3, 64, 69]] = 1                                              # bad starts in both blocks
    st = lm.State(n, k)
    cx = dict(theta=theta, cols=cols, tf=tf, lo=np.full(k, 1e-3), hi=np.full(k, 1e3), st=st, opts=dict(ftol=1e-2), n=n, k=k)
    cx["ref"], _ = lm.run(emu_model, theta, cols, tf, cx["lo"], cx["hi"], cost, grad, JtJ, status, st, lm.FIRST, cx["opts"], "70 cells FIRST")
    assert cx["ref"][2] == n - 3
    kinds = [("accept", "reject", "failed", "nan_grad", "conv")[c % 5] for c in range(n)]
    for it in range(2):                                                  # (compare checks every done cell and every other column against the copy taken before the call)
        c2, g2, H2, s2 = judged_fit(cx, kinds, 133 + it)
        conv = np.array([x == "conv" for x in kinds]) & (st.state == lm.RUNNING)
        tgt = np.where(conv, st.cost_cur * (1 - 1e-3), c2)
        ok = np.isfinite(c2)
        c2[ok], g2[ok], _ = lm.with_cost(c2[ok], g2[ok], H2[ok], tgt[ok])
        ref = step(emu_model, cx, c2, g2, H2, s2, what="70 cells STEP %d" % it)
        done = (st.state != lm.RUNNING).sum()
        assert ref[2] == n - done
    assert (st.state[[3, 64, 69]] == lm.FAILED_START).all() and (st.state == lm.CONV_F).sum() >= 10 and (st.state == lm.RUNNING).sum() >= 30


def test_shared_and_per_cell_bounds_give_the_same_bits(emu_model):
    k, n = 3, N
    tf = np.array([lm.LOG, lm.LINEAR, lm.LOG], np.int32)
    lo, hi = np.array([0.4, 0.3, 0.45]), np.array([2.5, 2.2, np.inf])
    outs = []
    for per_cell in (False, True):
        theta, cols = lm.make_theta(n, k, 141)
        st = lm.State(n, k)
        cost, grad, JtJ = lm.make_fit(n, k, 142, cost_scale=1e-6)
        b = (lambda x: np.ascontiguousarray(np.broadcast_to(x, (n, k)))) if per_cell else (lambda x: x)
        rc, nrun = lm.call(emu_model, theta, cols, tf, b(lo), b(hi), cost, grad, JtJ, None, st, lm.FIRST)
        assert rc == 0
        outs.append((theta, st, nrun))
    assert outs[0][2] == outs[1][2] and lm.same_bits(outs[0][0], outs[1][0]) and all(lm.same_bits(getattr(outs[0][1], a), getattr(outs[1][1], a)) for a in lm.STATE_ARRAYS)
    assert (outs[0][0][:, cols] != lm.make_theta(n, k, 141)[0][:, cols]).any()


def test_every_e_arg_case_writes_nothing(emu_model):
    k, n = 3, N
    theta, cols = lm.make_theta(n, k, 151)
    tf = np.zeros(k, np.int32)
    cost, grad, JtJ = lm.make_fit(n, k, 152)
    st = lm.State(n, k)
    theta0, st0 = theta.copy(), st.copy()
    base = dict(cols=cols, transform=tf, lo=None, hi=None, phase=lm.FIRST, opts=None, n_keys=None, n_cells=None, null=())
    twice = cols.copy(); twice[2] = twice[0]
    outside = cols.copy(); outside[1] = theta.shape[1]
    negative = cols.copy(); negative[1] = -1
    cases = [dict(n_cells=0), dict(n_keys=0), dict(n_keys=9), dict(cols=outside), dict(cols=negative), dict(cols=twice), dict(transform=np.array([0, 2, 0], np.int32)),
             dict(phase=3), dict(phase=-1), dict(lo=np.array([0.1, 3.0, 0.1]), hi=np.array([5.0, 2.0, 5.0])),
             dict(opts=dict(lambda_up=1.0)), dict(opts=dict(lambda_down=0.0)), dict(opts=dict(lambda_down=1.0)), dict(opts=dict(lambda0=0.0)),
             dict(opts=dict(ftol=-1.0)), dict(opts=dict(xtol=-1.0)), dict(opts=dict(gtol=-1.0)), dict(opts=dict(diag_floor=-1.0))]
    cases += [dict(null=(a,)) for a in ("theta", "cols", "transform", "cost", "grad", "JtJ", "n_running") + lm.STATE_ARRAYS]
    for case in cases:
        a = dict(base, **case)
        rc, nrun = lm.call(emu_model, theta, a["cols"], a["transform"], a["lo"], a["hi"], cost, grad, JtJ, None, st, a["phase"], a["opts"], a["n_keys"], a["n_cells"], a["null"])
        assert rc == lm.E_ARG, case
        assert nrun == -12345 and lm.same_bits(theta, theta0) and all(lm.same_bits(getattr(st, x), getattr(st0, x)) for x in lm.STATE_ARRAYS), case
    rc, nrun = lm.call(emu_model, theta, cols, tf, None, None, cost, grad, JtJ, None, st, lm.FIRST)      # (and the call itself is a good one)
    assert rc == 0 and nrun == n

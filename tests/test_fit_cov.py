"""plh_fit_cov -- parameter covariances and identifiability of device fits -- on the wave-emulator build of the device source (no GPU) and on the GPU, against the numpy
restatement of the header's definition (tests/cov_cases.py: the restatement, the derivation of the bounds).  cov.compare holds the checks every call gets: sigma2, free_mask,
status and every 0 / 1 / NaN / inf exact; corr, cov, stderr, the eigenvalues, the eigenvectors' residual and orthogonality within the bounds; the sign rule."""
import numpy as np
import pytest

import cov_cases as cov
import lm_cases as lm
import parity

KS = (1, 2, 3, 8)
N = 16                                                                   # less than one wave
N_BIG = 70                                                               # a second block with 6 live lanes
KEYS = ["D_sp", "k_p"]


def run(model, pr, what, **kw):
    ref, infos = cov.reference(**pr)
    rc, got = cov.call(model, **pr)
    assert rc == 0, model._lib.plh_last_error()
    return got, ref, infos, cov.compare(got, ref, infos, what, **kw)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,per_cell", ((N, True), (N, False), (N_BIG, True)))
def test_random_fits_against_the_restatement(emu_model, k, n, per_cell):
    pr = cov.make_problem(n, k, 100 + 10 * k + n, per_cell_bounds=per_cell)
    got, ref, infos, worst = run(emu_model, pr, "random fits k=%d n=%d %s bounds" % (k, n, "per-cell" if per_cell else "shared"))
    assert (ref["status"] & ~cov.NO_FREE == 0).all()                     # (k = 1 with its key held: no analysed key)
    assert all(i["cond"] is None or i["cond"] <= 1e6 for i in infos)
    held = np.array([i["held"] for i in infos])
    assert held[:, 0].any() and not held[:, 0].all()                     # a key on its bound is held with the gradient outward and free with it inward
    shares = np.array([cov.restatement_shares(i) for i in infos]).max(axis=0)
    print("k = %d: the restatement sits at %s of the bounds (eigenvalues, residual, orthogonality, inverse), at most %d sweeps" % (k, shares, max(i["sweeps"] for i in infos)))
    assert (shares <= cov.RESTATEMENT_SHARE).all() and max(i["sweeps"] for i in infos) <= 8


@pytest.mark.parametrize("k", (2, 3, 8))
def test_near_collinear_columns(emu_model, k):
    n = N
    r = np.random.default_rng(300 + k)
    cost, grad, JtJ = np.empty(n), np.empty((n, k)), np.empty((n, k, k))
    for c in range(n):
        J = r.normal(size=(lm.M_ROWS, k))
        J[:, k - 1] = r.uniform(0.5, 2.0) * J[:, 0] + 1e-6 * r.normal(size=lm.M_ROWS)
        res = r.normal(size=lm.M_ROWS)
        cost[c], grad[c], JtJ[c] = 0.5 * res @ res, J.T @ res, J.T @ J
    pr = dict(theta_k=r.uniform(0.5, 2.0, size=(n, k)), transform=np.zeros(k, np.int32), lo=None, hi=None, cost=cost, grad=grad, JtJ=JtJ, n_data=np.full(n, lm.M_ROWS, np.int32))
    got, ref, infos, worst = run(emu_model, pr, "near-collinear k=%d" % k, eig_only=True)
    assert (got["status"] & ~cov.SINGULAR == 0).all()
    assert (got["collinearity"] >= 1e5).all(), got["collinearity"]
    for c in range(n):
        two = np.sort(np.argsort(-np.abs(got["evec"][c, 0]))[:2])
        assert two.tolist() == [0, k - 1], (c, got["evec"][c, 0])


def test_every_status_one_problem_each(emu_model):
    k, n = 3, N
    pr = cov.make_problem(n, k, 400, per_cell_bounds=True, bounded=False)
    ix = cov.status_problems(pr, (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14))
    clean = cov.make_problem(n, k, 400, per_cell_bounds=True, bounded=False)
    got, ref, infos, _ = run(emu_model, pr, "every status")
    bad = [ix[a] for a in ("nan_cost", "inf_grad", "nan_jtj_upper", "nan_theta", "outside_bounds", "log_nonpositive", "scaled_overflow", "negative_diagonal")]
    assert (got["status"][bad] == cov.BAD_INPUT).all() and (got["free"][bad] == 0).all()
    for a in cov.DOUBLE_OUT:
        assert np.isnan(got[a][bad]).all(), a
    c = ix["all_held"]
    assert got["status"][c] == cov.NO_FREE and got["free"][c] == 0 and np.isnan(got["collinearity"][c]) and np.isnan(got["eval"][c]).all() and np.isnan(got["evec"][c]).all()
    assert (got["cov"][c] == 0).all() and (got["corr"][c] == 0).all() and (got["stderr"][c] == 0).all() and got["sigma2"][c] == 2 * pr["cost"][c] / lm.M_ROWS
    c = ix["unseen"]
    assert got["status"][c] == (cov.UNSEEN | (0b010 << 8)) and got["free"][c] == 0b111
    assert got["stderr"][c, 1] == np.inf and np.isfinite(got["stderr"][c, [0, 2]]).all()
    assert np.isnan(got["cov"][c, 1, :]).all() and np.isnan(got["cov"][c, :, 1]).all() and np.isnan(got["corr"][c, 1, :]).all() and np.isfinite(got["cov"][c][np.ix_([0, 2], [0, 2])]).all()
    assert np.isfinite(got["eval"][c, :2]).all() and np.isnan(got["eval"][c, 2]) and (got["evec"][c, :2, 1] == 0).all() and np.isnan(got["evec"][c, 2]).all()
    assert got["sigma2"][c] == 2 * pr["cost"][c] / (lm.M_ROWS - 3)      # (an unseen key stays among the free ones)
    c = ix["no_dof"]
    assert got["status"][c] == cov.NO_DOF and np.isnan(got["sigma2"][c]) and np.isnan(got["cov"][c]).all() and np.isnan(got["stderr"][c]).all()
    assert np.isfinite(got["corr"][c]).all() and np.isfinite(got["eval"][c]).all() and np.isfinite(got["evec"][c]).all() and np.isfinite(got["collinearity"][c])
    # the neighbours: every other problem has the bits of the call without the special cases
    rc, plain = cov.call(emu_model, **clean)
    assert rc == 0
    others = np.setdiff1d(np.arange(n), list(ix.values()))
    for a in cov.OUT:
        assert lm.same_bits(np.ascontiguousarray(got[a][others]), np.ascontiguousarray(plain[a][others])), a
    assert (plain["status"] == 0).all()


def test_every_status_in_one_call_of_two_keys(emu_model):
    """the same special cases with k = 2, where the singular problem fits in as well: twelve of the sixteen problems of ONE call are special, the other four keep their bits"""
    k, n = 2, N
    make = lambda: cov.make_problem(n, k, 450, transform=[lm.LOG, lm.LINEAR], per_cell_bounds=True, bounded=False)
    pr = make()
    ix = cov.status_problems(pr, (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13))
    c = ix["singular"] = 14
    pr["theta_k"][c, 0], pr["JtJ"][c] = 1.0, 4.0                          # (s = 1: C = [[1, 1], [1, 1]] exactly)
    got, ref, infos, _ = run(emu_model, pr, "every status, k = 2")
    want = dict(all_held=cov.NO_FREE, unseen=cov.UNSEEN | (0b10 << 8), no_dof=cov.NO_DOF, singular=cov.SINGULAR)
    for name, i in ix.items():
        assert got["status"][i] == want.get(name, cov.BAD_INPUT), (name, got["status"][i])
    c = ix["singular"]
    assert np.isnan(got["cov"][c]).all() and np.isnan(got["corr"][c]).all() and np.isnan(got["stderr"][c]).all() and got["eval"][c].tolist() == [0.0, 2.0] and got["collinearity"][c] == np.inf
    c = ix["unseen"]
    assert got["stderr"][c, 1] == np.inf and got["stderr"][c, 0] > 0 and got["corr"][c, 0, 0] == 1.0 and np.isnan(got["corr"][c, 0, 1]) and np.isnan(got["eval"][c, 1]) and got["eval"][c, 0] == 1.0
    rc, plain = cov.call(emu_model, **make())
    others = np.setdiff1d(np.arange(n), list(ix.values()))
    assert rc == 0 and len(others) == 4 and (plain["status"] == 0).all()
    for a in cov.OUT:
        assert lm.same_bits(np.ascontiguousarray(got[a][others]), np.ascontiguousarray(plain[a][others])), a


def test_singular_exact_duplicate_column(emu_model):
    k, n = 2, N
    pr = cov.make_problem(n, k, 500, transform=[lm.LINEAR, lm.LINEAR], per_cell_bounds=True, bounded=False)
    clean = {a: (v.copy() if isinstance(v, np.ndarray) else v) for a, v in pr.items()}
    c = 5
    pr["JtJ"][c] = 4.0                                                   # J = [a, a]: C = [[1, 1], [1, 1]], the second pivot is exactly 0
    got, ref, infos, _ = run(emu_model, pr, "singular")
    assert got["status"][c] == cov.SINGULAR and got["free"][c] == 0b11
    assert np.isnan(got["cov"][c]).all() and np.isnan(got["corr"][c]).all() and np.isnan(got["stderr"][c]).all() and np.isfinite(got["sigma2"][c])
    assert got["eval"][c, 0] == 0.0 and got["eval"][c, 1] == 2.0 and got["collinearity"][c] == np.inf
    assert np.allclose(np.abs(got["evec"][c]), np.sqrt(0.5), rtol=16 * cov.EPS, atol=0)      # (a handful of rounded operations, one subtraction 1 - 0.29)
    rc, plain = cov.call(emu_model, **clean)
    others = np.setdiff1d(np.arange(n), [c])
    for a in cov.OUT:
        assert lm.same_bits(np.ascontiguousarray(got[a][others]), np.ascontiguousarray(plain[a][others])), a


def test_straight_line_closed_form_and_units(emu_model):
    n, m = N, 20
    r = np.random.default_rng(600)
    t = np.linspace(1.0, 3.0, m)
    X = np.stack([np.ones(m), t], axis=1)
    cost, grad, JtJ, theta = np.empty(n), np.empty((n, 2)), np.empty((n, 2, 2)), r.uniform(0.5, 2.0, size=(n, 2))
    for c in range(n):
        res = 0.1 * r.normal(size=m)
        cost[c], grad[c], JtJ[c] = 0.5 * res @ res, X.T @ res, X.T @ X
    pr = dict(theta_k=theta, transform=np.zeros(2, np.int32), lo=None, hi=None, cost=cost, grad=grad, JtJ=JtJ, n_data=np.full(n, m, np.int32))
    got, ref, infos, _ = run(emu_model, pr, "straight line")
    assert (got["status"] == 0).all()
    P = infos[0]["P"]
    B = cov.STEP_C * 2 * cov.EPS * infos[0]["cond"] * np.abs(P).max()
    r0, r1 = np.sqrt(m), np.sqrt((t * t).sum())
    XtXi = np.linalg.inv(X.T @ X)
    for c in range(n):
        sg2 = 2 * cost[c] / (m - 2)
        assert got["sigma2"][c] == sg2
        assert (np.abs(got["cov"][c] - sg2 * XtXi) <= B * sg2 / np.outer([r0, r1], [r0, r1]) + 4 * cov.EPS * np.abs(sg2 * XtXi)).all()      # (numpy's own inverse: a few eps)
        assert abs(got["corr"][c, 0, 1] - (-t.sum() / np.sqrt(m * (t * t).sum()))) <= B
    # the LINEAR key b in other units: b' = 1e6 b, so the column of J is divided by 1e6
    f = np.array([1.0, 1e-6])
    pr2 = dict(pr, theta_k=theta * np.array([1.0, 1e6]), grad=grad * f, JtJ=JtJ * np.outer(f, f))
    rc, got2 = cov.call(emu_model, **pr2)
    assert rc == 0 and (got2["status"] == 0).all()
    E = cov.STEP_C * 2 * cov.EPS * float(np.linalg.norm(infos[0]["C"], 2))
    assert (np.abs(got2["corr"] - got["corr"]) <= 2 * B).all() and (np.abs(got2["eval"] - got["eval"]) <= 2 * E).all()
    assert (np.abs(got2["collinearity"] / got["collinearity"] - 1) <= 2 * E / got["eval"][:, 0]).all()      # (1 / sqrt(eval[0]): half the relative change of eval[0])
    assert np.allclose(got2["stderr"][:, 1], 1e6 * got["stderr"][:, 1], rtol=1e-9)


def test_every_e_arg_case_writes_nothing(emu_model):
    k, n = 3, N
    pr = cov.make_problem(n, k, 700, per_cell_bounds=False, bounded=False)
    out = cov.outputs(n, k)
    cases = [dict(n=0), dict(n=-1), dict(n_keys=0), dict(n_keys=9), dict(transform=np.array([0, 2, 0], np.int32)), dict(per_cell=2), dict(per_cell=-1),
             dict(lo=np.array([0.1, 3.0, 0.1]), hi=np.array([5.0, 2.0, 5.0])), dict(lo=np.array([0.1, np.nan, 0.1]))]
    cases += [dict(null=(a,)) for a in ("transform", "theta_k", "cost", "grad", "JtJ") + cov.OUT]
    for case in cases:
        rc, _ = cov.call(emu_model, **dict(pr, **case), out=out)
        assert rc == cov.E_ARG, case
        assert cov.untouched(out), case
    rc, got = cov.call(emu_model, **pr, out=out)                           # (and the call itself is a good one; n_data, lo and hi may be NULL)
    assert rc == 0 and (got["status"] == 0).all()
    rc, got = cov.call(emu_model, **dict(pr, n_data=None, lo=None, hi=None))
    assert rc == 0 and (got["sigma2"] == 1.0).all()


def check_result_covariance(pkg, p, res, n_data_expected, rows):
    """res.covariance() against the restatement on the result's own arrays"""
    cv = res.covariance()
    def host(a):
        if not hasattr(a, "cpu"):
            return np.asarray(a)
        import torch
        torch.cuda.synchronize()                                         # (the call is queued on the fit's launch stream)
        return a.cpu().numpy()
    assert np.array_equal(host(res.n_data), np.full(rows, n_data_expected)) and host(res.n_data).dtype == np.int32
    pr = dict(theta_k=host(res.theta_cur), transform=[lm.LOG, lm.LOG], lo=None, hi=None, cost=host(res.cost), grad=host(res.grad), JtJ=host(res.JtJ), n_data=host(res.n_data))
    ref, infos = cov.reference(**pr)
    got = {a: host(getattr(cv, a)) for a in cov.OUT}
    assert cv.keys == KEYS and got["cov"].shape == (rows, 2, 2)
    worst = cov.compare(got, ref, infos, "fit_ensemble(...).covariance(), %d rows" % rows)
    ca = res.covariance(absolute_sigma=True)
    assert (host(ca.sigma2) == 1.0).all() and lm.same_bits(host(ca.corr), got["corr"]) and lm.same_bits(host(ca.eval), got["eval"])
    return cv, got, pr


def test_fit_ensemble_covariance_on_the_emulator(emu_model, pkg):
    p, n = emu_model, 4
    cols = [p.θ_keys.index(k) for k in KEYS]
    proto = [{"I": np.array([-0.5, -1.0, -0.5, -1.0]), "tf": 60.0}]
    t = np.linspace(2.0, 58.0, 12)
    V_data = np.ascontiguousarray(pkg.simulate_ensemble(p, pkg.theta_matrix(p, n), proto, SOC=0.9)(t, fields="V").V)
    Theta0 = pkg.theta_matrix(p, n)
    Theta0[:, cols] *= np.array([[1.3, 0.8], [0.7, 1.1], [0.8, 1.25], [1.2, 0.9]])
    tf = {k: "log" for k in KEYS}
    grouped = pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data, SOC=0.9, transform=tf, max_iter=1, groups=np.array([0, 0, 1, 1]))      # (the first point and the last judgement)
    check_result_covariance(pkg, p, grouped, 24, 2)
    single = pkg.fit_ensemble(p, Theta0, proto, KEYS, t, V_data, SOC=0.9, transform=tf, max_iter=1)
    cv, got, pr = check_result_covariance(pkg, p, single, 12, 4)
    # weights: a point with weight 0 is not a datum (two cells, a short run: only the count is looked at)
    w = np.ones((2, 4)); w[1, :3] = 0.0
    short = [{"I": -1.0, "tf": 10.0}]
    wres = pkg.fit_ensemble(p, Theta0[:2], short, KEYS, t[:4], V_data[:2, :4], w, I_data=np.full(4, -1.0), I_weights=np.array([1.0, 0.0, 2.0, 1.0]), SOC=0.9, transform=tf, max_iter=1)
    assert wres.n_data.tolist() == [4 + 3, 1 + 3] and wres.n_data.dtype == np.int32
    # fit_covariance on ens.lsq's arrays: the same bits as the method on identical inputs
    ens = pkg.simulate_ensemble(p, single.theta, proto, SOC=0.9, sens=KEYS)
    fit = ens.lsq(t, V_data)
    th_k = np.ascontiguousarray(single.theta[:, cols])
    a = pkg.fit_covariance(p, th_k, fit.cost, fit.grad, fit.JtJ, n_data=single.n_data, transform=["log", "log"], keys=KEYS)
    single.theta_cur, single.cost, single.grad, single.JtJ = th_k, fit.cost, fit.grad, fit.JtJ
    b = single.covariance()
    for name in ("sigma2", "cov", "stderr", "corr", "eval", "evec", "collinearity", "free", "status"):
        assert lm.same_bits(getattr(a, name), getattr(b, name)), name
    assert isinstance(a.cov, np.ndarray) and (a.status == 0).all()


# ---- GPU
def mixed_problem(n, k, seed):
    pr = cov.make_problem(n, k, seed, per_cell_bounds=True)
    if k >= 3:
        cov.status_problems(pr, (1, 9, 17, 63, 64, 65, 66, 100, 127, 128, 129))      # in every block, on both sides of the block boundaries, in the partial block
    else:
        pr["cost"][[1, 64, 129]] = np.nan
        pr["n_data"][[2, 65, 128]] = 0
    return pr


@pytest.mark.gpu
@pytest.mark.parametrize("k", (1, 5, 8))
def test_host_and_device_pointers_give_the_same_bits(hip_model, k):
    import torch
    n = 130                                                              # three blocks, the last one partial
    pr = mixed_problem(n, k, 800 + k)
    ref, infos = cov.reference(**pr)
    rc, got = cov.call(hip_model, **pr)
    assert rc == 0, hip_model._lib.plh_last_error()
    stream = torch.cuda.Stream()
    rc, dgot = cov.call_device(hip_model, pr["theta_k"], pr["transform"], pr["lo"], pr["hi"], pr["cost"], pr["grad"], pr["JtJ"], pr["n_data"], stream)
    assert rc == 0, hip_model._lib.plh_last_error()
    for a in cov.OUT:
        assert lm.same_bits(got[a], dgot[a]), a
    cov.compare(got, ref, infos, "GPU k=%d n=%d" % (k, n))
    assert (ref["status"] != 0).sum() >= 3


@pytest.mark.gpu
def test_covariance_of_a_grouped_fit_in_hbm(hip_model, pkg):
    import torch
    p, ng, m = hip_model, 8, 3
    n = ng * m
    cols = [p.θ_keys.index(k) for k in KEYS]
    groups = np.repeat(np.arange(ng), m)
    proto = [{"I": np.tile([-0.5, -1.0, -2.0], ng), "tf": 300.0}]
    o = pkg.Opts(); o.reltol, o.abstol, o.maxiters = parity.TIGHT["reltol"], parity.TIGHT["abstol"], 200000
    t = np.linspace(15.0, 285.0, 16)
    truth = pkg.theta_matrix(p, n)
    sV = 1e-3
    rng = np.random.default_rng(6)
    V_true = pkg.simulate_ensemble(p, truth, proto, SOC=0.9, opts=o)(t, fields="V").V
    V_data = np.ascontiguousarray(np.asarray(V_true) + sV * rng.standard_normal((n, len(t))))
    wV = np.full(len(t), 1.0 / sV)
    Theta0 = truth.copy()
    Theta0[:, cols] *= np.repeat(2.0 ** rng.uniform(-0.5, 0.5, size=(ng, 2)), m, axis=0)
    stream = torch.cuda.Stream()
    res = pkg.fit_ensemble(p, torch.from_numpy(Theta0).cuda(), proto, KEYS, t, V_data, wV, SOC=0.9, opts=o, transform={k: "log" for k in KEYS}, max_iter=20, device=True,
                           stream=stream.cuda_stream, lm=dict(ftol=1e-10), groups=groups)
    cv, got, pr = check_result_covariance(pkg, p, res, m * len(t), ng)
    stream.synchronize()
    for a in (cv.sigma2, cv.cov, cv.stderr, cv.corr, cv.eval, cv.evec, cv.collinearity, cv.free, cv.status):
        assert isinstance(a, torch.Tensor) and a.is_cuda and a.shape[0] == ng
    assert (got["status"] == 0).all()
    th = pr["theta_k"]
    assert ((got["stderr"] > 0) & (got["stderr"] < th)).all(), (got["stderr"], th)
    z = np.log(th / truth[::m][:, cols]) / (got["stderr"] / th)
    print("covariance of the grouped fit in HBM: z-scores %s, sigma2 %s, collinearity %s" % (np.round(z, 2).tolist(), np.round(got["sigma2"], 3).tolist(), np.round(got["collinearity"], 2).tolist()))

"""plh_lm_step: inputs, the numpy restatement of the definition in include/petlion_hip.h, the bounds and the comparison (tests/test_lm_step.py, test_lm_fit_analytic.py,
test_lm_fit.py, test_gpu_lm.py).  Nothing here calls the library except `call`.

The bound on the step.  The kernel solves A d = -gs by a Cholesky factorisation in fp64; backward-stable, so |d - d_exact| <= c k eps cond(A) |d_exact| with a modest c.  The
tests take c = 64:   |d - d_ref|_inf <= STEP_C k eps cond(A) |d_ref|_inf   in u (u = theta, or ln theta for a LOG key), cond(A) computed for the system the restatement solved
last.  The restatement itself (numpy.linalg.cholesky / solve) must sit at <= 1/10 of it against the same solve in numpy.longdouble (restatement_share).
The step is only visible through the theta row the kernel stores, so the comparison is made on theta and carries the rounding of that store and of exp / ln on both sides:
  LINEAR   |theta - theta_ref| <= B + 2 eps max(|theta_cur|, |theta_ref|)             (theta_cur + d rounded once on each side)
  LOG      |theta - theta_ref| <= |theta_ref| (B + 4 eps)                              (exp to an ulp and the product, on each side)
with B the bound above.  A key the restatement clamps to a bound, holds, or leaves at cur is compared exactly.  pred: |pred - pred_ref| <= STEP_C k eps cond(A) |pred_ref|
(pred = 1/2 d.A d + 1/2 lambda d.D d >= 0: no cancellation).  lambda, state, the counters, n_running and which keys moved are exact.

Near ties.  Every decision of the restatement reports how far it is from its threshold (`tie`): actual / pred within 1e-6 of eta, a convergence test or lambda_max within a
factor 2, a pivot or a clamp within 1e-9.  The case builders and the analytic loops assert that no cell is near a tie.  The replay of a fit of integrated curves cannot choose
its inputs: there the convergence tests and lambda_max are held to the rounding margin (`tie_rounding`: within 1e-6 of the threshold), the other three as above; no cell is
excluded in either."""
import ctypes as C

import numpy as np

LINEAR, LOG = 0, 1
FIRST, STEP, LAST = 0, 1, 2
RUNNING, CONV_F, CONV_X, CONV_G, MAXIT, STALLED, FAILED_START = range(7)
MAX_TRIES = 16
E_ARG = -1
EPS = float(np.finfo(np.float64).eps)
STEP_C = 64.0
RESTATEMENT_SHARE = 0.1
OPTS = dict(lambda0=1e-3, lambda_up=3.0, lambda_down=1.0 / 3.0, lambda_min=1e-12, lambda_max=1e12, eta=1e-4, ftol=1e-10, xtol=1e-8, gtol=1e-8, diag_floor=1e-12)
STATE_ARRAYS = ("theta_cur", "cost_cur", "grad_cur", "JtJ_cur", "lam", "pred", "state", "n_accept", "n_reject")


class State:
    """the caller-owned per-cell state of a fit"""

    def __init__(self, n, k, seed=99):
        r = np.random.default_rng(seed)                                  # (what FIRST must overwrite, and what a bad start must leave alone)
        self.theta_cur, self.cost_cur, self.grad_cur, self.JtJ_cur = r.normal(size=(n, k)), r.normal(size=n), r.normal(size=(n, k)), r.normal(size=(n, k, k))
        self.lam, self.pred = r.normal(size=n), r.normal(size=n)
        self.state, self.n_accept, self.n_reject = (r.integers(0, 7, n).astype(np.int32) for _ in range(3))

    def copy(self):
        c = State.__new__(State)
        for a in STATE_ARRAYS:
            setattr(c, a, getattr(self, a).copy())
        return c


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _finite(*xs):
    return all(np.isfinite(x).all() for x in xs)


def _far(x, thr, factor=2.0):
    """x is not within `factor` of the threshold thr (both >= 0)"""
    return x <= thr / factor or x >= thr * factor


def _mark(info, x, thr):
    """a comparison of x with the threshold thr (both >= 0): a tie for the case builders when within a factor 2, a tie at the rounding margin when within 1e-6 of it"""
    info["tie"] |= not _far(x, thr)
    info["tie_rounding"] |= bool(abs(x - thr) <= 1e-6 * thr)


def chol_solve(A, b, dtype):
    """A^-1 b by Cholesky in `dtype` (numpy.linalg has no longdouble)"""
    A, b = np.asarray(A, dtype), np.asarray(b, dtype)
    n = len(b)
    L = np.zeros((n, n), dtype)
    for i in range(n):
        for j in range(i):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
        L[i, i] = np.sqrt(A[i, i] - (L[i, :i] * L[i, :i]).sum())
    y = np.zeros(n, dtype)
    for i in range(n):
        y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    x = np.zeros(n, dtype)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x


def _propose(th, g, H, cc, lam, lo, hi, tf, o, info):
    """Propose of the header, one cell: (state, trial theta, lambda, pred or None)"""
    k = len(th)
    lg = tf == LOG
    s = np.where(lg, th, 1.0)
    gs = s * g
    Hs = (s[:, None] * s[None, :]) * H
    if not _finite(gs, Hs):
        return STALLED, th.copy(), lam, None
    held = ((th <= lo) & (gs > 0)) | ((th >= hi) & (gs < 0))
    free = ~held
    info["held"] = held
    dg = np.diag(Hs).copy()
    with np.errstate(invalid="ignore"):
        thr = o["gtol"] * np.sqrt(dg * (2.0 * cc))
    small = np.array([bool(abs(gs[i]) <= thr[i]) for i in range(k)])
    if free.any() and cc != 0:
        rat = [abs(gs[i]) / thr[i] if thr[i] > 0 else (0.0 if gs[i] == 0 else np.inf) for i in range(k) if free[i]]
        _mark(info, max(rat), 1.0)
    if not free.any() or cc == 0 or small[free].all():
        return CONV_G, th.copy(), lam, None
    D = np.maximum(dg, o["diag_floor"] * dg.max())
    for _ in range(MAX_TRIES):
        A = Hs[np.ix_(free, free)] + lam * np.diag(D[free])
        # the coupled part: a free key with a zero row, column and gradient (a parameter the data do not see) is a 1 x 1 block of its own, with the pivot lambda D_i (no
        # subtraction: its sign is not a matter of rounding) and the solution exactly 0 -- it enters neither the other keys' solve nor their error
        cpl = free & ~((gs == 0) & ((Hs - np.diag(dg)) == 0).all(axis=1))
        Ac = Hs[np.ix_(cpl, cpl)] + lam * np.diag(D[cpl])
        ev = np.linalg.eigvalsh(A)
        evc = np.linalg.eigvalsh(Ac) if cpl.any() else np.ones(1)
        near = bool(abs(evc[0]) <= 1e-9 * max(abs(evc[-1]), np.finfo(float).tiny))
        info["tie"] |= near
        info["tie_rounding"] |= near
        fail, d, trial, pred = False, np.zeros(k), th.copy(), None
        try:
            np.linalg.cholesky(A)
            fail = not ev[0] > 0
        except np.linalg.LinAlgError:
            fail = True
        if not fail:
            d[free] = np.linalg.solve(A, -gs[free])
            info.update(A=A, rhs=-gs[free], d_ref=d.copy(), free=free, condA=float(np.linalg.cond(Ac)) if cpl.any() else 1.0)      # (cond of the coupled part)
            with np.errstate(over="ignore", invalid="ignore"):
                trial = np.where(lg, th * np.exp(d), th + d)
            trial[held] = th[held]
            for b in (lo, hi):
                fb = np.isfinite(b) & free
                near = bool((np.abs(trial[fb] - b[fb]) <= 1e-9 * np.abs(b[fb])).any() and not (trial[fb] == b[fb]).all())
                info["tie"] |= near
                info["tie_rounding"] |= near
            cl = (trial < lo) | (trial > hi)
            trial = np.where(trial < lo, lo, np.where(trial > hi, hi, trial))
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.where(cl, np.where(lg, np.log(trial / th), trial - th), d)
            info["clamped"] = cl
            pred = -(gs @ d + 0.5 * d @ (Hs @ d))
            fail = not _finite(trial, d) or not pred > 0 or not np.isfinite(pred)
        if fail:
            lam = lam * o["lambda_up"]
            info["raises"] += 1
            _mark(info, lam, o["lambda_max"])
            if lam > o["lambda_max"]:
                return STALLED, th.copy(), lam, None
            continue
        meas = np.where(lg, np.abs(d), np.abs(d) / np.maximum(np.abs(th), np.finfo(float).tiny))
        if o["xtol"] > 0:
            _mark(info, meas.max(), o["xtol"])
        if (meas <= o["xtol"]).all():
            return CONV_X, th.copy(), lam, None
        info["moved"] = trial != th
        return RUNNING, trial, lam, pred
    return STALLED, th.copy(), lam, None


def step_reference(theta, cols, transform, lo, hi, cost, grad, JtJ, status, st, phase, opts=None):
    """the header's definition, cell by cell.  theta and st (a State) are not modified: returns (theta', State', n_running, [info per cell]).  lo / hi: None, [k] or [n, k]"""
    o = dict(OPTS, **(opts or {}))
    n, k = grad.shape
    cols, tf = np.asarray(cols), np.asarray(transform)
    bnd = lambda b, dflt: np.full((n, k), dflt) if b is None else np.broadcast_to(np.asarray(b, float), (n, k))
    lo, hi = bnd(lo, -np.inf), bnd(hi, np.inf)
    th_out, new, infos = theta.copy(), st.copy(), []
    for c in range(n):
        info = dict(tie=False, tie_rounding=False, raises=0, touched=False, held=np.zeros(k, bool), moved=np.zeros(k, bool), clamped=np.zeros(k, bool), d_ref=None, condA=None, judged=None)
        infos.append(info)
        if phase != FIRST and st.state[c] != RUNNING:
            continue
        Hu = np.triu(JtJ[c]) + np.triu(JtJ[c], 1).T
        ok = (status is None or status[c] == 0) and _finite(cost[c], grad[c], Hu)
        tin = theta[c, cols]
        if phase == FIRST:
            with np.errstate(invalid="ignore"):
                good = ok and _finite(tin) and bool(((lo[c] <= tin) & (tin <= hi[c])).all()) and not bool(((tf == LOG) & (tin <= 0)).any())
            if not good:
                new.state[c] = FAILED_START
                continue
            take, lam, prd, state = True, o["lambda0"], 0.0, RUNNING
            new.n_accept[c] = new.n_reject[c] = 0
        else:
            state, lam, prd = RUNNING, st.lam[c], st.pred[c]
            actual = st.cost_cur[c] - cost[c]
            take = bool(ok and actual >= o["eta"] * prd)
            info["judged"] = "accept" if take else "reject"
            if ok:
                near = bool(abs(actual / prd - o["eta"]) <= 1e-6)
                info["tie"] |= near
                info["tie_rounding"] |= near
            if take:
                lam = max(lam * o["lambda_down"], o["lambda_min"])
                new.n_accept[c] += 1
                if o["ftol"] > 0 and st.cost_cur[c] != 0:
                    _mark(info, abs(actual), o["ftol"] * abs(st.cost_cur[c]))
                if actual <= o["ftol"] * st.cost_cur[c]:
                    state = CONV_F
            else:
                lam = lam * o["lambda_up"]
                new.n_reject[c] += 1
                _mark(info, lam, o["lambda_max"])
                if lam > o["lambda_max"]:
                    state = STALLED
            if phase == LAST and state == RUNNING:
                state = MAXIT
        info["touched"] = True
        if take:
            new.theta_cur[c], new.cost_cur[c], new.grad_cur[c], new.JtJ_cur[c] = tin, cost[c], grad[c], JtJ[c]
        th, trial = new.theta_cur[c].copy(), new.theta_cur[c].copy()
        if state == RUNNING:
            Hc = np.triu(new.JtJ_cur[c]) + np.triu(new.JtJ_cur[c], 1).T
            state, trial, lam, p = _propose(th, new.grad_cur[c].copy(), Hc, new.cost_cur[c], lam, lo[c], hi[c], tf, o, info)
            if p is not None:
                prd = p
        th_out[c, cols] = trial
        new.lam[c], new.pred[c], new.state[c] = lam, prd, state
    return th_out, new, int((new.state == RUNNING).sum()), infos


def restatement_share(info, k):
    """the restatement's own solve against the same solve in numpy.longdouble, as a share of the bound (no code under test)"""
    if info["d_ref"] is None:
        return 0.0
    x = chol_solve(info["A"], info["rhs"], np.longdouble)
    ref = np.abs(x).max()
    bound = STEP_C * k * EPS * info["condA"] * float(ref)
    return float(np.abs(info["d_ref"][info["free"]] - x).max() / bound) if bound > 0 else 0.0


def call(model, theta, cols, transform, lo, hi, cost, grad, JtJ, status, st, phase, opts=None, n_keys=None, n_cells=None, null=()):
    """plh_lm_step on host pointers, in place on theta and st.  Returns (return code, n_running).  null: names of arguments passed as NULL"""
    lib, h = model._lib, model._h
    import pkgload
    cap = pkgload.load()._capi
    n, k = grad.shape
    ci, ti = np.ascontiguousarray(cols, dtype=np.int32), np.ascontiguousarray(transform, dtype=np.int32)
    per_cell = int(any(b is not None and np.ndim(b) == 2 for b in (lo, hi)))
    fb = lambda b: None if b is None else np.ascontiguousarray(np.broadcast_to(np.asarray(b, float), (n, k)) if per_cell else b, dtype=np.float64)
    lo_, hi_ = fb(lo), fb(hi)
    so = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
    for a in (theta, cost, grad, JtJ) + tuple(getattr(st, x) for x in STATE_ARRAYS):
        assert a.flags.c_contiguous
    nrun = np.array([-12345], np.int32)
    args = dict(theta=theta, cols=ci, transform=ti, lo=lo_, hi=hi_, cost=cost, grad=grad, JtJ=JtJ, status=so, n_running=nrun, **{x: getattr(st, x) for x in STATE_ARRAYS})
    p = {x: (None if x in null else cap.ptr(a)) for x, a in args.items()}
    rc = lib.plh_lm_step(h, n if n_cells is None else n_cells, theta.shape[1], p["theta"], k if n_keys is None else n_keys, p["cols"], p["transform"], p["lo"], p["hi"], per_cell,
                         p["cost"], p["grad"], p["JtJ"], p["status"], p["theta_cur"], p["cost_cur"], p["grad_cur"], p["JtJ_cur"], p["lam"], p["pred"],
                         p["state"], p["n_accept"], p["n_reject"], None if opts is None else C.byref(cap.LMOpts(**opts)), phase, p["n_running"], cap.PLH_HOST, None)
    return rc, int(nrun[0])


def compare(theta0, st0, got_theta, got_st, got_nrun, ref, cols, transform, what="", tie="tie"):
    """the kernel's outputs (from theta0 / st0) against the restatement's (ref = step_reference's return value).  Returns the worst shares of the bounds.
    tie: "tie" -- the case builders' margins (synthetic inputs are chosen to keep them); "tie_rounding" -- the replay of a fit of real curves, where a test may come within a
    factor 2 of its tolerance honestly and only the rounding margin (1e-6 of the threshold) would make the two sides disagree"""
    ref_theta, ref_st, ref_nrun, infos = ref
    n, k = st0.theta_cur.shape
    cols, tf = np.asarray(cols), np.asarray(transform)
    assert not any(i[tie] for i in infos), "%s: cells %s sit near a tie" % (what, [c for c, i in enumerate(infos) if i[tie]])
    assert got_nrun == ref_nrun, (what, got_nrun, ref_nrun)
    for a in ("state", "n_accept", "n_reject", "lam"):
        assert same_bits(getattr(got_st, a), getattr(ref_st, a)), (what, a, getattr(got_st, a), getattr(ref_st, a))
    for a in ("theta_cur", "cost_cur", "grad_cur", "JtJ_cur"):                       # (copies of inputs: exact)
        assert same_bits(getattr(got_st, a), getattr(ref_st, a)), (what, a)
    other = np.setdiff1d(np.arange(theta0.shape[1]), cols)
    assert same_bits(got_theta[:, other], theta0[:, other]), what + ": a theta column outside cols was written"
    worst = dict(step=0.0, pred=0.0)
    for c, info in enumerate(infos):
        if not info["touched"]:
            assert same_bits(got_theta[c], theta0[c]), (what, c)
            for a in STATE_ARRAYS:
                if not (a == "state" and ref_st.state[c] == FAILED_START):
                    assert same_bits(getattr(got_st, a)[c:c + 1], getattr(st0, a)[c:c + 1]), (what, c, a)
            continue
        g, r, cur = got_theta[c, cols], ref_theta[c, cols], ref_st.theta_cur[c]
        stepped = ref_st.state[c] == RUNNING and info["d_ref"] is not None
        if not stepped:
            assert same_bits(g, cur) and got_st.pred[c] == ref_st.pred[c], (what, c, "theta must be cur")
            continue
        B = STEP_C * k * EPS * info["condA"] * np.abs(info["d_ref"]).max()
        assert np.array_equal(g != cur, info["moved"]), (what, c, "which keys moved", g != cur, info["moved"])
        for i in range(k):
            if info["held"][i] or info["clamped"][i] or not info["moved"][i]:
                assert g[i] == r[i], (what, c, i, g[i], r[i])
                continue
            tol = abs(r[i]) * (B + 4 * EPS) if tf[i] == LOG else B + 2 * EPS * max(abs(cur[i]), abs(r[i]))
            worst["step"] = max(worst["step"], abs(g[i] - r[i]) / tol)
        pb = STEP_C * k * EPS * info["condA"] * abs(ref_st.pred[c])
        worst["pred"] = max(worst["pred"], abs(got_st.pred[c] - ref_st.pred[c]) / pb)
    print("%s: step at %.3g, pred at %.3g of the bounds" % (what, worst["step"], worst["pred"]))
    assert worst["step"] <= 1.0 and worst["pred"] <= 1.0, (what, worst)
    return worst


def run(model, theta, cols, transform, lo, hi, cost, grad, JtJ, status, st, phase, opts=None, what=""):
    """one call of the kernel and of the restatement from the same inputs (teacher forcing); theta and st are advanced in place to the KERNEL's outputs.  Returns
    (restatement's return value, worst shares)"""
    theta0, st0 = theta.copy(), st.copy()
    ref = step_reference(theta0, cols, transform, lo, hi, cost, grad, JtJ, status, st0, phase, opts)
    rc, nrun = call(model, theta, cols, transform, lo, hi, cost, grad, JtJ, status, st, phase, opts)
    assert rc == 0, model._lib.plh_last_error()
    return ref, compare(theta0, st0, theta, st, nrun, ref, cols, transform, what)


# ---- synthetic fits: JtJ = J'J and grad = J'r from J [m, k] with prescribed singular values
M_ROWS = 12


def make_fit(n, k, seed, cond_H=1e4, cost_scale=1.0):
    r = np.random.default_rng(seed)
    cost, grad, JtJ = np.empty(n), np.empty((n, k)), np.empty((n, k, k))
    for c in range(n):
        U, _ = np.linalg.qr(r.normal(size=(M_ROWS, k)))
        V, _ = np.linalg.qr(r.normal(size=(k, k)))
        sv = np.logspace(0, -0.5 * np.log10(cond_H), k) if k > 1 else np.ones(1)
        J = (U * sv) @ V.T
        res = r.normal(size=M_ROWS) * np.sqrt(cost_scale)
        cost[c], grad[c], JtJ[c] = 0.5 * res @ res, J.T @ res, J.T @ J
        JtJ[c] = 0.5 * (JtJ[c] + JtJ[c].T)
    return cost, grad, JtJ


def make_theta(n, k, seed, extra=3):
    """theta [n, k + extra] in [0.5, 2], and k columns in an order that is neither sorted nor contiguous"""
    r = np.random.default_rng(seed)
    nt = k + extra
    cols = r.permutation(nt)[:k]
    return np.ascontiguousarray(r.uniform(0.5, 2.0, size=(n, nt))), cols.astype(np.int32)


def with_cost(cost, grad, JtJ, target):
    """the same fit with its cost set to target [n] (the residual rescaled: grad follows)"""
    f = np.sqrt(target / cost)
    return target.copy(), grad * f[:, None], JtJ.copy()


def replay(history, cols, transform, lo, hi, opts=None, what="fit"):
    """every recorded iteration of fit_ensemble(history=True) through the restatement, from the inputs the kernel saw"""
    worst = dict(step=0.0, pred=0.0)
    for it, rec in enumerate(history):
        st0, got = State.__new__(State), State.__new__(State)
        for a in STATE_ARRAYS:
            setattr(st0, a, rec["before"][a])
            setattr(got, a, rec["after"][a])
        status = rec["status"]
        ref = step_reference(rec["theta_before"], cols, transform, lo, hi, rec["cost"], rec["grad"], rec["JtJ"], status, st0, rec["phase"], opts)
        w = compare(rec["theta_before"], st0, rec["theta_after"], got, rec["n_running"], ref, cols, transform, "%s iteration %d" % (what, it), tie="tie_rounding")
        worst = {k: max(worst[k], w[k]) for k in worst}
    return worst

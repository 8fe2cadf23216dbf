"""plh_fit_cov: inputs, the numpy restatement of the definition in include/petlion_hip.h, the bounds and the comparison (tests/test_fit_cov.py).  Nothing here calls the
library except `call` (and `call_device` on the GPU).

The bounds, in the form lm_cases uses for plh_lm_step (STEP_C = 64).  C is the normalised information matrix over the analysed keys (unit diagonal), P = C^-1 from a Cholesky
factorisation in fp64: backward stable, so |P - P_exact| <= c k eps cond2(C) max|P| with a modest c; the tests take c = 64.
  corr     |corr - corr_ref| <= B,  B = STEP_C k eps cond2(C) max|P|        (|corr| <= 1 <= P_ii: the bound on P covers its normalisation)
  cov      |cov_ij - ref| <= B |sigma2 s_i s_j| / (r_i r_j)                 (cov_ij is P_ij times that factor)
  stderr   |stderr_i - ref| / ref <= (B / P_ii) / 2                         (the square root halves the relative error of cov_ii)
  eval     |eval - numpy.linalg.eigvalsh(C)| <= E,  E = STEP_C k eps ||C||_2        (Jacobi is backward stable in the norm of the matrix)
  evec     max|C V - V diag(eval)| <= E  and  max|V^T V - I| <= STEP_C k eps, over the analysed keys; the sign rule and the zeros exactly.  Eigenvectors are not compared with
           another solver's: near-degenerate pairs make that meaningless.
  collinearity   against 1 / sqrt of the eval[0] it was computed from, 4 eps relative (a square root and a division, each correctly rounded)
  sigma2 ((2 cost) / dof: two correctly rounded operations, the same on both sides), free_mask, status and every exact 0 / 1 / NaN / inf: exact.
The restatement itself must sit at <= RESTATEMENT_SHARE (lm_cases') of each bound: its eigenvalues against eigvalsh, its residual and orthogonality, and its inverse against
a Gauss-Jordan elimination in numpy.longdouble."""
import numpy as np

import lm_cases as lm

LINEAR, LOG = lm.LINEAR, lm.LOG
BAD_INPUT, NO_FREE, UNSEEN, NO_DOF, SINGULAR, SWEEPS = 1, 2, 4, 8, 16, 32
MAX_SWEEPS = 16
E_ARG = -1
EPS = lm.EPS
STEP_C = lm.STEP_C
RESTATEMENT_SHARE = lm.RESTATEMENT_SHARE
DOUBLE_OUT = ("sigma2", "cov", "stderr", "corr", "eval", "evec", "collinearity")
INT_OUT = ("free", "status")
OUT = DOUBLE_OUT + INT_OUT
SENTINEL, ISENTINEL = -777.25, -12345


def jacobi(C):
    """the header's cyclic Jacobi on the upper triangle of C: (diagonal, V, sweeps made, still rotating after MAX_SWEEPS)"""
    k = len(C)
    a, V = np.triu(np.asarray(C, float)).copy(), np.eye(k)
    at = lambda x, y: (x, y) if x < y else (y, x)
    sweeps, rot = 0, True
    with np.errstate(over="ignore"):
        while sweeps < MAX_SWEEPS and rot:
            rot, sweeps = False, sweeps + 1
            for p in range(k):
                for q in range(p + 1, k):
                    apq, app, aqq = a[p, q], a[p, p], a[q, q]
                    if abs(apq) <= EPS * np.sqrt(abs(app * aqq)):
                        a[p, q] = 0.0
                        continue
                    rot = True
                    th = (aqq - app) / (2.0 * apq)
                    t = (1.0 if th >= 0 else -1.0) / (abs(th) + np.sqrt(th * th + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    tau = s / (1.0 + c)
                    a[p, p], a[q, q], a[p, q] = app - t * apq, aqq + t * apq, 0.0
                    for x in range(k):
                        if x != p and x != q:
                            ip, iq = at(x, p), at(x, q)
                            g, h = a[ip], a[iq]
                            a[ip], a[iq] = g - s * (h + tau * g), h + s * (g - tau * h)
                    for x in range(k):
                        g, h = V[x, p], V[x, q]
                        V[x, p], V[x, q] = g - s * (h + tau * g), h + s * (g - tau * h)
    return np.diag(a).copy(), V, sweeps, rot


def chol_inverse(C, dtype=np.float64):
    """the header's P = C^-1: Cholesky row by row, X = L^-1 column by column, P = X^T X.  Returns (P, failed)"""
    C = np.asarray(C, dtype)
    k = len(C)
    L, fail = np.zeros((k, k), dtype), False
    for i in range(k):
        for j in range(i):
            L[i, j] = (C[j, i] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
        v = C[i, i] - (L[i, :i] * L[i, :i]).sum()
        if not v > 0 or not np.isfinite(v):
            fail, v = True, dtype(1.0)
        L[i, i] = np.sqrt(v)
    X = np.zeros((k, k), dtype)
    for j in range(k):
        X[j, j] = 1.0 / L[j, j]
        for i in range(j + 1, k):
            X[i, j] = -((L[i, j:i] * X[j:i, j]).sum() / L[i, i])
    return X.T @ X, fail


def gauss_jordan(C):
    """C^-1 in numpy.longdouble with partial pivoting (the reference of the restatement's own inverse)"""
    k = len(C)
    M = np.concatenate([np.asarray(C, np.longdouble), np.eye(k, dtype=np.longdouble)], axis=1)
    for c in range(k):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        M[[c, p]] = M[[p, c]]
        M[c] = M[c] / M[c, c]
        for r in range(k):
            if r != c:
                M[r] = M[r] - M[r, c] * M[c]
    return M[:, k:]


def reference(theta_k, transform, lo, hi, cost, grad, JtJ, n_data):
    """the header's definition, problem by problem.  lo / hi: None, [k] or [n, k]; n_data: None or [n].  Returns (dict of the outputs, [info per problem])"""
    n, k = grad.shape
    tf = np.asarray(transform)
    bnd = lambda b, dflt: np.full((n, k), dflt) if b is None else np.broadcast_to(np.asarray(b, float), (n, k))
    lo, hi = bnd(lo, -np.inf), bnd(hi, np.inf)
    out = dict(sigma2=np.full(n, np.nan), cov=np.full((n, k, k), np.nan), stderr=np.full((n, k), np.nan), corr=np.full((n, k, k), np.nan), eval=np.full((n, k), np.nan),
               evec=np.full((n, k, k), np.nan), collinearity=np.full(n, np.nan), free=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
    infos = []
    for c in range(n):
        info = dict(bad=True, an=np.zeros(k, bool), held=np.zeros(k, bool), unseen=np.zeros(k, bool), C=None, P=None, cond=None, sing=False, sweeps=0, scale=None)
        infos.append(info)
        th, g = theta_k[c], grad[c]
        H = np.triu(JtJ[c]) + np.triu(JtJ[c], 1).T
        lg = tf == LOG
        with np.errstate(invalid="ignore", over="ignore"):
            good = np.isfinite(cost[c]) and np.isfinite(g).all() and np.isfinite(H).all() and np.isfinite(th).all() and bool(((lo[c] <= th) & (th <= hi[c])).all()) \
                and not bool((lg & (th <= 0)).any())
            s = np.where(lg, th, 1.0)
            gs, Hs = s * g, (s[:, None] * s[None, :]) * H
            good = good and np.isfinite(gs).all() and np.isfinite(Hs).all() and not (np.diag(Hs) < 0).any()
        if not good:
            out["status"][c] = BAD_INPUT
            continue
        info["bad"] = False
        dg = np.diag(Hs).copy()
        held = ((th <= lo[c]) & (gs > 0)) | ((th >= hi[c]) & (gs < 0))
        unseen = ~held & (dg == 0)
        an = ~held & ~unseen
        info.update(held=held, unseen=unseen, an=an)
        st = 0
        out["free"][c] = int(sum(1 << i for i in range(k) if not held[i]))
        n_free, n_an = int((~held).sum()), int(an.sum())
        if unseen.any():
            st |= UNSEEN | (int(sum(1 << i for i in range(k) if unseen[i])) << 8)
        if n_an == 0:
            st |= NO_FREE
        sg2 = 1.0
        if n_data is not None:
            dof = int(n_data[c]) - n_free
            if dof <= 0:
                sg2, st = np.nan, st | NO_DOF
            else:
                sg2 = (2.0 * cost[c]) / float(dof)
        out["sigma2"][c] = sg2
        r = np.where(an, np.sqrt(np.where(an, dg, 1.0)), 1.0)
        C = np.eye(k)
        for i in range(k):
            for j in range(i + 1, k):
                if an[i] and an[j]:
                    C[i, j] = C[j, i] = Hs[i, j] / (r[i] * r[j])
        P, sing = chol_inverse(C)
        if sing:
            st |= SINGULAR
        ia = np.flatnonzero(an)
        Ca = C[np.ix_(ia, ia)]
        info.update(C=Ca, sing=sing, scale=np.abs(sg2 * s[:, None] * s[None, :]) / (r[:, None] * r[None, :]))
        if n_an and not sing:
            info.update(P=P[np.ix_(ia, ia)], cond=float(np.linalg.cond(Ca)))
        for i in range(k):
            for j in range(k):
                if held[i] or held[j]:
                    out["cov"][c, i, j] = out["corr"][c, i, j] = 0.0
                elif unseen[i] or unseen[j] or sing:
                    pass                                                 # (NaN)
                else:
                    out["cov"][c, i, j] = (s[i] * s[j]) * ((P[i, j] * sg2) / (r[i] * r[j]))
                    out["corr"][c, i, j] = 1.0 if i == j else P[i, j] / np.sqrt(P[i, i] * P[j, j])
            out["stderr"][c, i] = 0.0 if held[i] else np.inf if unseen[i] else np.sqrt(out["cov"][c, i, i])
        d, V, info["sweeps"], still = jacobi(C)
        if still:
            st |= SWEEPS
        order = np.argsort(np.where(an, d, np.inf), kind="stable")
        for j in range(n_an):
            v = V[:, order[j]].copy()
            if v[int(np.argmax(np.abs(v)))] < 0:
                v = -v
            out["eval"][c, j], out["evec"][c, j] = d[order[j]], v
        if n_an:
            e0 = out["eval"][c, 0]
            out["collinearity"][c] = np.inf if e0 <= 0 else 1.0 / np.sqrt(e0)
        out["status"][c] = st
    return out, infos


def restatement_shares(info):
    """the restatement's own arithmetic as shares of the bounds: (eigenvalues against eigvalsh, residual, orthogonality, inverse against longdouble Gauss-Jordan)"""
    C = info["C"]
    if C is None or len(C) == 0:
        return 0.0, 0.0, 0.0, 0.0
    k = len(C)
    d, V, _, _ = jacobi(C)
    nrm = float(np.linalg.norm(C, 2))
    E = STEP_C * k * EPS * nrm
    sh_e = float(np.abs(np.sort(d) - np.linalg.eigvalsh(C)).max() / E)
    sh_r = float(np.abs(C @ V - V * d).max() / E)
    sh_o = float(np.abs(V.T @ V - np.eye(k)).max() / (STEP_C * k * EPS))
    sh_p = 0.0
    if info["P"] is not None:
        Px = gauss_jordan(C)
        sh_p = float(np.abs(info["P"] - Px).max() / (STEP_C * k * EPS * info["cond"] * float(np.abs(Px).max())))
    return sh_e, sh_r, sh_o, sh_p


def _same(a, b):
    """exact agreement, NaN with NaN"""
    return bool(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True))


def compare(got, ref, infos, what="", eig_only=False):
    """the kernel's outputs (dict) against the restatement's.  eig_only: a problem whose C is singular to rounding -- the inverse has no bound worth the name; status, the
    patterns and the eigen outputs are still checked.  Returns the worst shares of the bounds."""
    n, k = ref["eval"].shape
    worst = dict(corr=0.0, cov=0.0, stderr=0.0, eval=0.0, resid=0.0, orth=0.0, coll=0.0)
    assert _same(got["status"], ref["status"]), (what, "status", got["status"], ref["status"])
    assert _same(got["free"], ref["free"]), (what, "free", got["free"], ref["free"])
    assert lm.same_bits(np.nan_to_num(got["sigma2"], nan=-1.0), np.nan_to_num(ref["sigma2"], nan=-1.0)) and _same(np.isnan(got["sigma2"]), np.isnan(ref["sigma2"])), (what, "sigma2")
    for c, info in enumerate(infos):
        if info["bad"]:
            assert all(np.isnan(got[a][c]).all() for a in DOUBLE_OUT) and got["free"][c] == 0 and got["status"][c] == BAD_INPUT, (what, c, "bad input")
            continue
        an = info["an"]
        ia = np.flatnonzero(an)
        na = len(ia)
        # every entry the definition fixes exactly: 0, 1, NaN, inf
        for a in ("cov", "corr", "stderr", "eval", "evec"):
            g, r = got[a][c], ref[a][c]
            fixed = ~np.isfinite(r) | (r == 0) if a != "corr" else ~np.isfinite(r) | (r == 0) | (r == 1)
            if a == "evec":
                fixed = np.isnan(r) | np.broadcast_to(~an, r.shape)      # (rows >= n_an; the components of the keys that are not analysed)
            assert _same(g[fixed], r[fixed]), (what, c, a, g, r)
            assert np.isfinite(g[~fixed]).all() or (eig_only and a in ("cov", "corr", "stderr")), (what, c, a, g)
        if na == 0:
            assert np.isnan(got["collinearity"][c]), (what, c)
            continue
        C = info["C"]
        nrm = float(np.linalg.norm(C, 2))
        E = STEP_C * k * EPS * nrm
        ev, V = got["eval"][c, :na], got["evec"][c, :na][:, ia].T      # V[:, j]: eigenvector j over the analysed keys
        worst["eval"] = max(worst["eval"], float(np.abs(ev - np.linalg.eigvalsh(C)).max() / E))
        assert (np.diff(ev) >= 0).all(), (what, c, "eval must ascend", ev)
        worst["resid"] = max(worst["resid"], float(np.abs(C @ V - V * ev).max() / E))
        worst["orth"] = max(worst["orth"], float(np.abs(V.T @ V - np.eye(na)).max() / (STEP_C * k * EPS)))
        for j in range(na):
            v = got["evec"][c, j]
            assert v[int(np.argmax(np.abs(v)))] > 0, (what, c, j, "sign rule", v)
        e0 = got["eval"][c, 0]
        if e0 <= 0:
            assert got["collinearity"][c] == np.inf, (what, c)
        else:
            worst["coll"] = max(worst["coll"], abs(got["collinearity"][c] * np.sqrt(e0) - 1.0) / (4 * EPS))
        if info["sing"] or eig_only:
            continue
        B = STEP_C * k * EPS * info["cond"] * float(np.abs(info["P"]).max())
        sub = np.ix_(ia, ia)
        worst["corr"] = max(worst["corr"], float(np.abs(got["corr"][c][sub] - ref["corr"][c][sub]).max() / B))
        if np.isfinite(ref["sigma2"][c]):
            tol = B * info["scale"][sub]
            nz = tol > 0
            if nz.any():
                worst["cov"] = max(worst["cov"], float((np.abs(got["cov"][c][sub] - ref["cov"][c][sub])[nz] / tol[nz]).max()))
            assert _same(got["cov"][c][sub][~nz], ref["cov"][c][sub][~nz]), (what, c, "cov where sigma2 = 0")
            se_g, se_r = got["stderr"][c, ia], ref["stderr"][c, ia]
            pos = se_r > 0
            if pos.any():
                worst["stderr"] = max(worst["stderr"], float((np.abs(se_g - se_r)[pos] / se_r[pos] / (0.5 * B / np.diag(info["P"])[pos])).max()))
    print("%s: shares of the bounds %s" % (what, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values()), (what, worst)
    return worst


def outputs(n, k, xp=np, device=None):
    """the output arrays, pre-filled with a sentinel (a refused call must leave it)"""
    if xp is np:
        shp = dict(sigma2=(n,), cov=(n, k, k), stderr=(n, k), corr=(n, k, k), eval=(n, k), evec=(n, k, k), collinearity=(n,))
        o = {a: np.full(s, SENTINEL) for a, s in shp.items()}
        o.update(free=np.full(n, ISENTINEL, np.int32), status=np.full(n, ISENTINEL, np.int32))
        return o
    o = {a: xp.as_tensor(v).to(device) for a, v in outputs(n, k).items()}
    return o


def untouched(o):
    return all((o[a] == SENTINEL).all() for a in DOUBLE_OUT) and all((o[a] == ISENTINEL).all() for a in INT_OUT)


def call(model, theta_k, transform, lo, hi, cost, grad, JtJ, n_data, n=None, n_keys=None, null=(), per_cell=None, out=None):
    """plh_fit_cov on host pointers.  Returns (return code, dict of the outputs).  null: names of arguments passed as NULL"""
    import pkgload
    cap = pkgload.load()._capi
    nn, k = grad.shape
    tf = np.ascontiguousarray(transform, dtype=np.int32)
    if per_cell is None:
        per_cell = int(any(b is not None and np.ndim(b) == 2 for b in (lo, hi)))
    fb = lambda b: None if b is None else np.ascontiguousarray(np.broadcast_to(np.asarray(b, float), (nn, k)) if per_cell == 1 else b, dtype=np.float64)
    nd = None if n_data is None else np.ascontiguousarray(n_data, dtype=np.int32)
    o = outputs(nn, k) if out is None else out
    args = dict(transform=tf, theta_k=np.ascontiguousarray(theta_k), lo=fb(lo), hi=fb(hi), cost=np.ascontiguousarray(cost), grad=np.ascontiguousarray(grad), JtJ=np.ascontiguousarray(JtJ),
                n_data=nd, **o)
    p = {x: (None if x in null else cap.ptr(a)) for x, a in args.items()}
    rc = model._lib.plh_fit_cov(model._h, nn if n is None else n, k if n_keys is None else n_keys, p["transform"], p["theta_k"], p["lo"], p["hi"], per_cell,
                                p["cost"], p["grad"], p["JtJ"], p["n_data"], *[p[a] for a in OUT], cap.PLH_HOST, None)
    return rc, o


def call_device(model, theta_k, transform, lo, hi, cost, grad, JtJ, n_data, stream):
    """the same call on tensors in HBM, queued on `stream` (a torch stream of the caller's).  Returns (return code, dict of host copies)"""
    import torch
    import pkgload
    cap = pkgload.load()._capi
    nn, k = grad.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    per_cell = int(any(b is not None and np.ndim(b) == 2 for b in (lo, hi)))
    tf = np.ascontiguousarray(transform, dtype=np.int32)
    with torch.cuda.stream(stream):
        up = lambda a, dt=np.float64: None if a is None else torch.from_numpy(np.array(a, dtype=dt, order="C")).to(dev)
        fb = lambda b: None if b is None else (up(np.broadcast_to(np.asarray(b, float), (nn, k))) if per_cell else np.ascontiguousarray(b, dtype=np.float64))
        lo_a, hi_a = fb(lo), fb(hi)
        ins = [up(theta_k), up(cost), up(grad), up(JtJ), up(n_data, np.int32)]
        o = outputs(nn, k, torch, dev)
        rc = model._lib.plh_fit_cov(model._h, nn, k, tf.ctypes.data, cap.ptr(ins[0]), cap.ptr(lo_a), cap.ptr(hi_a), per_cell, cap.ptr(ins[1]), cap.ptr(ins[2]), cap.ptr(ins[3]),
                                    cap.ptr(ins[4]), *[cap.ptr(o[a]) for a in OUT], cap.PLH_DEVICE, stream.cuda_stream)
        host = {a: v.cpu().numpy() for a, v in o.items()}                # (the copy is queued on the same stream and waited for)
    return rc, host


# ---- inputs
def make_problem(n, k, seed, transform=None, cond_H=1e4, per_cell_bounds=False, bounded=True):
    """n random fits of k keys (lm_cases.make_fit: JtJ = J'J with prescribed singular values), theta in [0.5, 2], a mix of LOG / LINEAR keys, and bounds: every third problem
    has key 0 on its lower bound with the gradient pointing outward (held), every third (offset 1) with the gradient pointing inward (free), key k - 1 of every fourth problem
    sits on its upper bound with the gradient outward (held)"""
    r = np.random.default_rng(seed)
    cost, grad, JtJ = lm.make_fit(n, k, seed + 1, cond_H=cond_H)
    theta, cols = lm.make_theta(n, k, seed + 2)
    theta_k = np.ascontiguousarray(theta[:, cols])
    tf = np.asarray([LOG if i % 2 == 0 else LINEAR for i in range(k)] if transform is None else transform, np.int32)
    lo, hi = np.full((n, k), 0.25), np.full((n, k), 4.0)
    if bounded:
        for c in range(n):
            if c % 3 == 0:
                lo[c, 0] = theta_k[c, 0]; grad[c, 0] = abs(grad[c, 0])           # at lo, gs > 0: held
            elif c % 3 == 1:
                lo[c, 0] = theta_k[c, 0]; grad[c, 0] = -abs(grad[c, 0])          # at lo, gs < 0: free
            if c % 4 == 2 and k > 1:
                hi[c, k - 1] = theta_k[c, k - 1]; grad[c, k - 1] = -abs(grad[c, k - 1])      # at hi, gs < 0: held
    if not per_cell_bounds:
        lo, hi = np.full(k, 0.25), np.full(k, 4.0)
        if bounded:                                                     # shared bounds: every problem's key 0 is put ON the shared lower bound instead
            theta_k[:, 0] = lo[0]
    n_data = np.full(n, lm.M_ROWS, np.int32)
    return dict(theta_k=theta_k, transform=tf, lo=lo, hi=hi, cost=cost, grad=grad, JtJ=JtJ, n_data=n_data)


def status_problems(pr, at):
    """overwrite the problems at `at` (11 indices) of a k >= 2 problem set with per-cell bounds by one special case each; returns {name: index}"""
    k = pr["grad"].shape[1]
    names = ("nan_cost", "inf_grad", "nan_jtj_upper", "nan_theta", "outside_bounds", "log_nonpositive", "scaled_overflow", "negative_diagonal", "all_held", "unseen", "no_dof")
    ix = dict(zip(names, at))
    pr["cost"][ix["nan_cost"]] = np.nan
    pr["grad"][ix["inf_grad"], k - 1] = np.inf
    pr["JtJ"][ix["nan_jtj_upper"], 0, k - 1] = np.nan
    pr["theta_k"][ix["nan_theta"], 1] = np.nan
    c = ix["outside_bounds"]; pr["theta_k"][c, 1] = 9.0
    c = ix["log_nonpositive"]; pr["theta_k"][c, 0] = -0.5; pr["lo"][c, 0] = -1.0      # (key 0 is LOG; inside its bounds)
    c = ix["scaled_overflow"]; pr["theta_k"][c, 0] = 1e200; pr["hi"][c, 0] = np.inf; pr["JtJ"][c, 0, 0] = 1e200      # s^2 H overflows
    c = ix["negative_diagonal"]; pr["JtJ"][c, 1, 1] = -1.0
    c = ix["all_held"]
    pr["lo"][c] = pr["theta_k"][c]; pr["grad"][c] = np.abs(pr["grad"][c]) + 1.0; pr["hi"][c] = 4.0
    c = ix["unseen"]
    pr["JtJ"][c, 1, :] = 0.0; pr["JtJ"][c, :, 1] = 0.0; pr["grad"][c, 1] = 0.0
    pr["lo"][c], pr["hi"][c] = 0.25, 4.0
    pr["n_data"][ix["no_dof"]] = 1
    return ix

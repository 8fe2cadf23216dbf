"""Shared by tests/test_predict.py (wave emulator) and tests/test_gpu_predict.py: inputs, yardstick and bounds for plh_predict / EnsembleSolution.predict.

Inputs.  resample_cases.make_case(width = 1 + 8) on lsq_cases.CASES ("main": every small-n branch and a long run; "edge": runs that end on, one past and one before a
64-point tile, a one-point run, the shortest spline): column 0 of the field is the curve, column 1 + k (transposed to [cell][k][max_pts]) is row k of dcurve, as in lsq_cases.
The columns do not depend on the width, so the case at K = 8 holds K = 1 and K = 3 as prefixes and ONE scipy reference per (case, extrapolate) serves them all.  A second and
third channel are other columns of the same field (channel_arrays): every column is a column of the reference.  "main" is resample_cases' own grid (seed 11).  "edge" is
drawn with seed 12: on the seed-11 grid of these point counts the numpy restatement itself sits at 0.0123 eps_6 from FITPACK in one sensitivity column of the (63, 1) cell
(lsq_cases never looks at a single sensitivity value, only at sums of them), which is more than TOL's definition allows the reference -- an input to replace, not a bound to
widen; on the seed-12 grid it sits at 0.0092.

Yardstick.  Never the code under test: scipy splrep / splev values (resample_cases.fitpack_reference) are pred and dpred; var = s' M s is formed from them in
numpy.longdouble, in which the (2 K + 2) roundings per entry are 2^-11 of a double's.

Covariances.  Per cell and K the inverse, by Gauss-Jordan elimination in numpy.longdouble (cov_cases.gauss_jordan), of the information matrix sum_q w_q^2 s_q s_q' of the same
case (s_q: the K reference sensitivities at query q under extrapolate = 0, finite at every finite query; w: lsq_cases' non-uniform weights), rounded to double and made
symmetric: what plh_fit_cov would hand over with sigma2 = 1.  The short cells of the cases have fewer points than keys and the smooth synthetic columns span six functions of
time, so for K >= 3 the raw matrix is singular to rounding (condition 1e15 .. 1e20: its "inverse" is noise of size 1e15 with negative variances).  Its diagonal is therefore
multiplied by 1 + RIDGE = 1 + 1e-8 -- a weak prior on every key, in Marquardt's scaling -- which leaves K = 1 as it is to 1e-8 and bounds the condition of the normalised
matrix by K / RIDGE: positive definite matrices with the conditioning of a real, poorly identified fit (1e8 .. 1e9), cancellation in s' M s included.  Variants: "held" -- one
key's row and column 0 (a key at a bound), "unseen" -- one key's row and column NaN (plh_fit_cov's rows of a key the data do not move).

Bounds.  Each resampled value is within eps_c = resample_cases.TOL max|column c| of FITPACK's: the bound the resample kernels are held to (resample_cases' docstring).  So
    |d pred|    <= eps_0
    |d dpred_k| <= eps_k
and with s the reference values, ds the deviation of the evaluated ones (|ds_i| <= eps_i), M symmetric and v = M s:
    (s + ds)' M (s + ds) - s' M s = 2 ds' v + ds' M ds,       so the propagated part is    <= 2 sum_i eps_i |v_i| + sum_ij eps_i |M_ij| eps_j;
the evaluation itself, in double: v_i is a sum of K products (K roundings of the products, K - 1 of the sums: each relative to at most sum_j |M_ij s_j|), var a sum of K
products s_i v_i (again 2 K): to first order at most (2 K + 2) 2^-53 sum_ij |s_i M_ij s_j|, with or without contraction into FMAs.  With the house slack of lm_cases /
cov_cases over that worst case:
    |d var| <= 2 sum_i eps_i |sum_j M_ij s_j| + sum_ij eps_i |M_ij| eps_j + 64 K 2^-52 sum_ij |s_i M_ij s_j|.
test_predict.py::test_restatement_sits_far_inside_the_bounds measures where the numpy float64 restatement (resample_cases.restatement and the two sums in the stated order)
sits in these bounds, with no code under test: <= 0.01 for pred and dpred (TOL's definition), <= 0.1 for var ((2 K + 2) / (64 K) <= 0.0625, and the propagated part is
1 / 100 of its bound)."""
import numpy as np

import cov_cases as cc
import lsq_cases as lc
import resample_cases as rc

KS = (1, 3, 8)
K_MAX = 8
RIDGE = 1e-8
CASES = lc.CASES
SEEDS = {"main": 11, "edge": 12}
E_ARG = rc.E_ARG
SENTINEL = -777.0
OUTS = ("pred", "dpred", "var")
HELD, UNSEEN = 1, 0                                  # the key zeroed in the "held" variant (needs K >= 2), the key made NaN in the "unseen" variant


class Problem:
    """one case with its reference: .k (the resample case at width 1 + K_MAX), .S[ex] [cell, n_q, 1 + K_MAX] by scipy, .W [cell, n_q] (the weights of the information
    matrices), .cov[K] [cell, K, K]"""


def information(S, w, K, first=1):
    """sum_q w_q^2 s_q s_q' in longdouble over the queries with a weight (s_q = S[q, first : first + K]), its diagonal times 1 + RIDGE"""
    use = w != 0
    J = (w[use, None] * S[use, first:first + K]).astype(np.longdouble)
    H = J.T @ J
    return H + np.diag(np.diag(H) * np.longdouble(RIDGE))


def covariance(S, w, K, first=1):
    M = cc.gauss_jordan(information(S, w, K, first)).astype(np.float64)
    M = np.triu(M) + np.triu(M, 1).T
    assert np.isfinite(M).all()
    return M


def make_problem(pkg, name):
    p = Problem()
    p.k = k = rc.make_case(pkg, cell_points=CASES[name], width=1 + K_MAX, seed=SEEDS[name])
    p.S = {ex: rc.fitpack_reference(k, ex) for ex in (0, 1)}
    base = 0.25 + 1.5 * np.random.default_rng(23).random(len(k.tq))
    base[np.isnan(k.tq)] = 0.0
    p.W = np.tile(base, (k.n, 1))
    p.cov = {K: np.stack([covariance(p.S[0][c], p.W[c], K) for c in range(k.n)]) for K in KS}
    return p


def held(M, i=HELD):
    M = M.copy()
    M[..., i, :] = 0.0
    M[..., :, i] = 0.0
    return M


def unseen(M, i=UNSEEN):
    M = M.copy()
    M[..., i, :] = np.nan
    M[..., :, i] = np.nan
    return M


def channel_arrays(k, K, first=0):
    """curve [cell][max_pts] = column `first` of the field and dcurve [cell][K][max_pts] = the K columns after it (first = 0: lsq_cases.arrays)"""
    return np.ascontiguousarray(k.src[:, :, first]), np.ascontiguousarray(k.src[:, :, first + 1:first + 1 + K].transpose(0, 2, 1))


def reference(S, K, M=None, first=0):
    """pred [n_q], dpred [K, n_q], var [n_q] of one cell from resampled values S [n_q, width] and the cell's covariance M [K, K], with what the bounds need: absv [K, n_q] =
    |sum_j M_ij s_j| and A [n_q] = sum_ij |s_i M_ij s_j|"""
    ref = dict(pred=S[:, first].copy(), dpred=np.ascontiguousarray(S[:, first + 1:first + 1 + K].T), var=None)
    if M is not None:
        s, Ml = ref["dpred"].astype(np.longdouble), np.asarray(M, np.longdouble)
        v = Ml @ s
        ref["var"] = (s * v).sum(axis=0).astype(np.float64)
        ref["absv"] = np.abs(v).astype(np.float64)
        ref["A"] = np.einsum("iq,ij,jq->q", np.abs(s), np.abs(Ml), np.abs(s)).astype(np.float64)
    return ref


def bounds(k, c, K, ref, M=None, first=0):
    """the bounds of the module docstring for cell c: pred (scalar), dpred [K, 1], var [n_q]"""
    eps = rc.TOL * np.abs(k.src[c, :int(k.n_pts[c]), first:first + 1 + K]).max(axis=0)
    e0, ek = eps[0], eps[1:]
    b = dict(pred=e0, dpred=ek[:, None])
    if M is not None:
        b["var"] = 2.0 * (ek[:, None] * ref["absv"]).sum(axis=0) + float(ek @ np.abs(M) @ ek) + 64.0 * K * 2.0 ** -52 * ref["A"]
    return b


def ratios(got, ref, bnd, rows):
    """{name: largest |got - ref| / bound over the queries `rows` [n_q] bool}"""
    out = {}
    for nm in OUTS:
        if got.get(nm) is None or ref.get(nm) is None:
            continue
        d = np.abs(np.asarray(got[nm], dtype=float) - ref[nm])[..., rows]
        b = np.broadcast_to(np.asarray(bnd[nm], dtype=float), ref[nm].shape)[..., rows]
        assert np.isfinite(d).all(), (nm, got[nm])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(d == 0, 0.0, d / b)
        out[nm] = float(q.max()) if d.size else 0.0
    return out


def compared(k, c, ex):
    """[n_q] bool: the queries of cell c that are compared under `ex` (resample_cases: finite, and under extrapolate = 1 not far outside the run's points)"""
    rows = ~np.isnan(k.tq)
    return rows & rc.mild(k, c) if ex else rows


def check_cell(pb, K, ex, c, got, M, label, first=0):
    """one cell's outputs (dict: pred [n_q], dpred [K, n_q], var [n_q] or None) against the yardstick; prints every ratio before asserting.  A NaN query gives NaN in
    every output; a query that is not compared (far extrapolation) must be finite"""
    k = pb.k
    ref = reference(pb.S[ex][c], K, M, first)
    rows, nanq = compared(k, c, ex), np.isnan(k.tq)
    rat = ratios(got, ref, bounds(k, c, K, ref, M, first), rows)
    print("%s K %d extrapolate %d cell %d: |got - ref| / bound " % (label, K, ex, c) + " ".join("%s %.3g" % kv for kv in rat.items()))
    assert all(v <= 1.0 for v in rat.values()), (label, K, ex, c, rat)
    for nm in OUTS:
        if got.get(nm) is not None:
            a = np.asarray(got[nm])
            assert np.isnan(a[..., nanq]).all() and np.isfinite(a[..., ~nanq]).all(), (label, nm, c)
    return rat


def restated_var(M, s):
    """the two sums in the stated order, in float64: v_i = sum_j M_ij s_j (j ascending), var = sum_i s_i v_i (i ascending); s [K, n_q]"""
    K = s.shape[0]
    var = np.zeros(s.shape[1])
    for i in range(K):
        v = np.zeros(s.shape[1])
        for j in range(K):
            v = v + M[i, j] * s[j]
        var = var + s[i] * v
    return var


def call(pkg, p, k, K, extrapolate, cov=None, cells=None, tq=None, chans=(0,), want=None, group_off=None, n_groups=0, want_status=True, kind=None, stream=None, dev=None,
         arrays=None, raw=None):
    """plh_predict on the case (the listed cells): channel i is column chans[i] of the field with the K columns after it.  want: per channel the outputs asked for (default
    all three, var only with a cov); the others are NULL.  cov: [n_prob, K, K] or None.  arrays: {channel index: (curve, dcurve)} replacing a channel's inputs.  raw: a dict
    of C arguments that replace the computed ones (the argument checks).  Host pointers, or device tensors made from the same arrays with kind = PLH_DEVICE.  Returns
    (rc, [per channel dict(pred, dpred, var)], status); outputs start as SENTINEL, status as -7"""
    cap = pkg._capi
    cells = list(range(k.n)) if cells is None else cells
    n = len(cells)
    tq = k.tq if tq is None else tq
    nq = len(tq)
    want = [OUTS if cov is not None else OUTS[:2]] * len(chans) if want is None else want
    ins = [np.ascontiguousarray(k.t[cells]), np.ascontiguousarray(k.n_pts[cells]), np.ascontiguousarray(k.run_info[cells]), None if cov is None else np.ascontiguousarray(cov, dtype=np.float64)]
    cin, cout = [], []
    for i, first in enumerate(chans):
        cu, dc = (arrays or {}).get(i) or channel_arrays(k, K, first)
        cin.append([np.ascontiguousarray(cu[cells]), np.ascontiguousarray(dc[cells])])
        cout.append([np.full((n, nq), SENTINEL) if "pred" in want[i] else None, np.full((n, K, nq), SENTINEL) if "dpred" in want[i] else None, np.full((n, nq), SENTINEL) if "var" in want[i] else None])
    status = np.full(n, -7, np.int32)
    if kind == cap.PLH_DEVICE:
        import torch
        up = lambda a: None if a is None else torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).to(dev)
        ins, cin, cout, status = [up(a) for a in ins], [[up(a) for a in r] for r in cin], [[up(a) for a in r] for r in cout], up(status)
        P = lambda a: None if a is None else a.data_ptr()
    else:
        kind = cap.PLH_HOST
        P = lambda a: None if a is None else a.ctypes.data
    ch = (cap.PredictChannel * max(len(chans), 1))()
    for i in range(len(chans)):
        ch[i] = cap.PredictChannel(P(cin[i][0]), P(cin[i][1]), P(cout[i][0]), P(cout[i][1]), P(cout[i][2]))
    off = None if group_off is None else np.ascontiguousarray(group_off, dtype=np.int32)
    a = dict(n=n, n_runs=k.n_runs, max_pts=k.max_pts, t=P(ins[0]), n_pts=P(ins[1]), run_info=P(ins[2]), n_ch=len(chans), ch=ch, n_sens=K, n_q=nq, tq=tq.ctypes.data,
             extrapolate=extrapolate, cov=P(ins[3]), n_groups=n_groups, group_off=None if off is None else off.ctypes.data, status=P(status) if want_status else None)
    if raw:
        for nm, v in raw.items():
            if "." in nm:                                             # "ch0.curve": one member of one channel
                setattr(ch[int(nm[2])], nm.split(".")[1], v)
            else:
                a[nm] = v
    code = p._lib.plh_predict(p._h, a["n"], a["n_runs"], a["max_pts"], a["t"], a["n_pts"], a["run_info"], a["n_ch"], a["ch"], a["n_sens"], a["n_q"], a["tq"], a["extrapolate"],
                              a["cov"], a["n_groups"], a["group_off"], a["status"], kind, stream)
    if kind == cap.PLH_DEVICE:
        import torch
        torch.cuda.synchronize()
        cout, status = [[None if x is None else x.cpu().numpy() for x in r] for r in cout], status.cpu().numpy()
    return code, [dict(zip(OUTS, r)) for r in cout], status


def cell_of(got, i):
    return {nm: (None if v is None else v[i]) for nm, v in got.items()}


def same_bits(a, b, names=OUTS):
    return all((a[nm] is None and b[nm] is None) or (a[nm] is not None and b[nm] is not None and np.array_equal(a[nm], b[nm], equal_nan=True)) for nm in names)


def untouched(got, status=None):
    """every output still holds its sentinel"""
    return all(v is None or (v == SENTINEL).all() for g in got for v in g.values()) and (status is None or (status == -7).all())

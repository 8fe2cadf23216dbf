"""Shared by tests/test_lsq.py (wave emulator) and tests/test_gpu_lsq.py: inputs, yardstick and bounds for plh_lsq / EnsembleSolution.lsq.

Inputs.  resample_cases.make_case(width = 1 + K): column 0 of its field is V, column 1 + k (transposed to [cell][k][max_pts]) is row k of dV_dtheta.  The columns do not depend
on the width, so the case with K = 8 holds every smaller K as a prefix and ONE scipy reference per (case, extrapolate) serves them all.  The data of a cell are the
FITPACK-resampled V of the next cell (clamped: finite at every finite query) plus a smooth offset, so that residuals are O(0.1), not rounding; the weights are non-uniform,
0 at the NaN query and, under extrapolate = 1, 0 at the queries resample_cases.mild excludes for that cell (far extrapolation: resample_cases' docstring).

Yardstick.  Never the code under test: scipy splrep / splev values (resample_cases.fitpack_reference), from which r, J, cost, grad and JtJ are formed in numpy.

Bounds.  Derived from resample_cases.TOL (each resampled value is within eps_c = TOL max|column c| of FITPACK's, the bound the resample kernels are held to), propagated
through the definition to first and second order, plus the rounding of a sum of n_used products:
    |d resid_q| <= |w_q| eps_0
    |d cost|    <= sum |w_q| |r_q| eps_0 + 1/2 sum (w_q eps_0)^2 + n_used 2^-52 cost
    |d grad_k|  <= sum (|J_qk| |w_q| eps_0 + |w_q| eps_k |r_q| + w_q^2 eps_0 eps_k) + n_used 2^-52 sum |J_qk r_q|
    |d JtJ_kl|  <= sum (|J_qk| |w_q| eps_l + |w_q| eps_k |J_ql| + w_q^2 eps_k eps_l) + n_used 2^-52 sum |J_qk J_ql|
with the reference's r and J.  test_lsq.py::test_restatement_sits_far_inside_the_bounds measures where the numpy restatement of the resample algorithm sits in them (no code
under test involved): TOL is 100 x the restatement's distance from FITPACK, so it must sit at <= 1 / 100 of every bound."""
import numpy as np

import resample_cases as rc

KS = (0, 1, 3, 8)
K_MAX = 8
EDGE_POINTS = ((64, 65), (63, 1), (4, 4))            # runs that end on, one past and one before a 64-point tile; a one-point run; the shortest spline
CASES = {"main": rc.CELL_POINTS, "edge": EDGE_POINTS}
RESTATEMENT_SHARE = 0.01                             # = RESTATEMENT_VS_FITPACK / TOL


class Problem:
    """one case with its reference and data: .k (the resample case at width 1 + K_MAX), .S[ex] [cell, n_q, 1 + K_MAX] by scipy, .Y [cell, n_q], .W[ex] [cell, n_q]"""


def make_problem(pkg, name):
    p = Problem()
    p.k = k = rc.make_case(pkg, cell_points=CASES[name], width=1 + K_MAX)
    p.S = {ex: rc.fitpack_reference(k, ex) for ex in (0, 1)}
    nq = len(k.tq)
    q = np.arange(nq)
    p.Y = np.stack([p.S[0][(c + 1) % k.n, :, 0] + 0.1 * np.cos(3.0 * q / nq + c) for c in range(k.n)])       # (NaN at the NaN query)
    base = 0.25 + 1.5 * np.random.default_rng(23).random(nq)
    base[np.isnan(k.tq)] = 0.0
    p.W = {0: np.tile(base, (k.n, 1)), 1: np.stack([np.where(rc.mild(k, c), base, 0.0) for c in range(k.n)])}
    for ex in (0, 1):
        assert (p.W[ex] != 0).sum(axis=1).min() >= 20
    return p


def arrays(k, K):
    """V [cell][max_pts] and dV_dtheta [cell][K][max_pts] (None for K = 0) of the case"""
    V = np.ascontiguousarray(k.src[:, :, 0])
    dV = np.ascontiguousarray(k.src[:, :, 1:1 + K].transpose(0, 2, 1)) if K else None
    return V, dV


def reference(S, y, w):
    """r, J, cost, grad, JtJ of one cell from resampled values S [n_q, 1 + K], data y [n_q], weights w [n_q] (points with w = 0 are left out, whatever S and y hold there)"""
    use = w != 0
    r = np.where(use, w * (S[:, 0] - y), 0.0)
    J = np.where(use[:, None], w[:, None] * S[:, 1:], 0.0)
    return dict(resid=r, J=J, cost=0.5 * float(r @ r), grad=J.T @ r, JtJ=J.T @ J)


def bounds(k, c, K, ref, w):
    """the bounds of the module docstring for cell c"""
    eps = rc.TOL * np.abs(k.src[c, :int(k.n_pts[c]), :1 + K]).max(axis=0)
    e0, ek = eps[0], eps[1:]
    r, J, aw = np.abs(ref["resid"]), np.abs(ref["J"]), np.abs(w)
    u = (w != 0).sum() * 2.0 ** -52
    b = dict(resid=aw * e0)
    b["cost"] = float((aw * r).sum() * e0 + 0.5 * ((aw * e0) ** 2).sum() + u * ref["cost"])
    b["grad"] = (J * aw[:, None]).sum(axis=0) * e0 + (aw * r).sum() * ek + (aw ** 2).sum() * e0 * ek + u * (J * r[:, None]).sum(axis=0)
    JW = (J * aw[:, None]).sum(axis=0)
    b["JtJ"] = JW[:, None] * ek[None, :] + ek[:, None] * JW[None, :] + (aw ** 2).sum() * ek[:, None] * ek[None, :] + u * (J.T @ J)
    return b


def ratios(got, ref, bnd):
    """{name: largest |got - ref| / bound} (an empty array -- K = 0 -- gives 0)"""
    out = {}
    for nm in ("resid", "cost", "grad", "JtJ"):
        if got.get(nm) is None:
            continue
        d, b = np.abs(np.asarray(got[nm], dtype=float) - ref[nm]), np.asarray(bnd[nm], dtype=float)
        assert np.isfinite(d).all(), (nm, got[nm])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(d == 0, 0.0, d / b)                                    # (a point left out: bound 0, and the difference must be 0)
        out[nm] = float(q.max()) if d.size else 0.0
    return out


def check_cell(pb, K, ex, c, got, y, w, label):
    """one cell's outputs (dict: cost, grad, JtJ, resid -- numpy, this cell's rows) against the yardstick; prints every ratio before asserting"""
    ref = reference(pb.S[ex][c][:, :1 + K], y, w)
    rat = ratios(got, ref, bounds(pb.k, c, K, ref, w))
    print("%s K %d extrapolate %d cell %d: |got - ref| / bound " % (label, K, ex, c) + " ".join("%s %.3g" % kv for kv in rat.items()))
    assert all(v <= 1.0 for v in rat.values()), (label, K, ex, c, rat)
    return rat


def call(pkg, p, k, K, y, w, per_cell, extrapolate, cells=None, tq=None, V=None, dV=None, want_resid=True, want_status=True, kind=None, stream=None, dev=None):
    """plh_lsq on the case (the first K sensitivity rows, the listed cells); host pointers, or device tensors made from the same arrays with kind = PLH_DEVICE.
    y / w: [n_q] with per_cell = 0, [len(cells), n_q] with per_cell = 1; w may be None.  Returns (rc, dict(cost, grad, JtJ, resid, status))"""
    cap = pkg._capi
    cells = list(range(k.n)) if cells is None else cells
    n = len(cells)
    tq = k.tq if tq is None else tq
    V0, dV0 = arrays(k, K)
    V, dV = V0 if V is None else V, dV0 if dV is None else dV
    ins = [np.ascontiguousarray(k.t[cells]), np.ascontiguousarray(k.n_pts[cells]), np.ascontiguousarray(k.run_info[cells]), np.ascontiguousarray(V[cells]),
           np.ascontiguousarray(dV[cells]) if K else None, np.ascontiguousarray(y, dtype=np.float64), None if w is None else np.ascontiguousarray(w, dtype=np.float64)]
    outs = [np.full(n, -777.0), np.full((n, K), -777.0) if K else None, np.full((n, K, K), -777.0) if K else None,
            np.full((n, len(tq)), -777.0) if want_resid else None, np.full(n, -7, np.int32)]
    lib = p._lib
    if kind == cap.PLH_DEVICE:
        import torch
        up = lambda a: None if a is None else torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).to(dev)
        ins, outs = [up(a) for a in ins], [up(a) for a in outs]
        P = lambda a: None if a is None else a.data_ptr()
    else:
        kind = cap.PLH_HOST
        P = lambda a: None if a is None else a.ctypes.data
    code = lib.plh_lsq(p._h, n, k.n_runs, k.max_pts, P(ins[0]), P(ins[1]), P(ins[2]), P(ins[3]), K, P(ins[4]), len(tq), tq.ctypes.data, P(ins[5]), P(ins[6]), per_cell,
                       extrapolate, P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), P(outs[4]) if want_status else None, kind, stream)
    if kind == cap.PLH_DEVICE:
        import torch
        torch.cuda.synchronize()
        outs = [None if a is None else a.cpu().numpy() for a in outs]
    return code, dict(zip(("cost", "grad", "JtJ", "resid", "status"), outs))


def cell_of(got, i):
    return {nm: (None if v is None else v[i]) for nm, v in got.items()}


def same_bits(a, b, names=("cost", "grad", "JtJ", "resid")):
    return all((a[nm] is None and b[nm] is None) or np.array_equal(a[nm], b[nm], equal_nan=True) for nm in names)

"""plh_lsq: the least-squares misfit of every cell's voltage curve against data, its gradient and Gauss-Newton matrix, here on the wave-emulator build of the device source
(no GPU).  The yardstick is scipy's splrep / splev (FITPACK) with r, J, cost, grad and JtJ formed in numpy, never the code under test; inputs, yardstick and the derivation
of the bounds are in tests/lsq_cases.py."""
import copy
import os

import numpy as np
import pytest

import lsq_cases as lc
import resample_cases as rc


@pytest.fixture(scope="module")
def problems(pkg):
    return {name: lc.make_problem(pkg, name) for name in lc.CASES}


def test_restatement_sits_far_inside_the_bounds(problems):
    """where the numpy restatement of the resample algorithm (resample_cases.restatement) sits in the bounds, K = 8, every cell, both extrapolate values: no code under test
    involved.  The bounds are built on TOL = 100 x the restatement's distance from FITPACK, so it must sit at <= 1 / 100 of each."""
    worst = {}
    for name, pb in problems.items():
        for ex in (0, 1):
            mine = rc.restatement(pb.k, ex)
            for c in range(pb.k.n):
                y, w = pb.Y[c], pb.W[ex][c]
                ref, got = lc.reference(pb.S[ex][c], y, w), lc.reference(mine[c], y, w)
                rat = lc.ratios(got, ref, lc.bounds(pb.k, c, lc.K_MAX, ref, w))
                print("%s extrapolate %d cell %d: restatement at " % (name, ex, c) + " ".join("%s %.2g" % kv for kv in rat.items()) + " of the bounds")
                for nm, v in rat.items():
                    worst[nm] = max(worst.get(nm, 0.0), v)
    assert max(worst.values()) > 0 and all(v <= lc.RESTATEMENT_SHARE for v in worst.values()), worst


@pytest.mark.parametrize("extrapolate", (0, 1))
@pytest.mark.parametrize("K", lc.KS)
@pytest.mark.parametrize("name", tuple(lc.CASES))
def test_against_the_yardstick(emu_model, pkg, problems, name, K, extrapolate):
    pb, ex = problems[name], extrapolate
    k = pb.k
    # every cell with its own data and weights in one call
    code, got = lc.call(pkg, emu_model, k, K, pb.Y, pb.W[ex], 1, ex)
    assert code == 0, emu_model._lib.plh_last_error()
    assert (got["status"] == 0).all()
    if K:
        assert np.array_equal(got["JtJ"], got["JtJ"].transpose(0, 2, 1))                                   # exactly symmetric
    else:
        assert got["grad"] is None and got["JtJ"] is None
    for c in range(k.n):
        lc.check_cell(pb, K, ex, c, lc.cell_of(got, c), pb.Y[c], pb.W[ex][c], "per-cell data")
        assert (got["resid"][c][pb.W[ex][c] == 0] == 0).all()
        # the same through shared data, cell by cell: the same bits
        code, one = lc.call(pkg, emu_model, k, K, pb.Y[c], pb.W[ex][c], 0, ex, cells=[c])
        assert code == 0 and one["status"].tolist() == [0]
        lc.check_cell(pb, K, ex, c, lc.cell_of(one, 0), pb.Y[c], pb.W[ex][c], "shared data")
        assert lc.same_bits(lc.cell_of(one, 0), lc.cell_of(got, c))
    if not ex:                                                                                             # (one weight row serves every cell)
        code, sh = lc.call(pkg, emu_model, k, K, pb.Y[0], pb.W[0][0], 0, 0, want_resid=False, want_status=False)
        assert code == 0 and sh["resid"] is None and (sh["status"] == -7).all()
        for c in range(k.n):
            lc.check_cell(pb, K, 0, c, lc.cell_of(sh, c), pb.Y[0], pb.W[0][0], "shared data, all cells")


@pytest.mark.parametrize("name", tuple(lc.CASES))
def test_null_weights_are_ones(emu_model, pkg, problems, name):
    pb, K = problems[name], 3
    k = pb.k
    keep = ~np.isnan(k.tq)
    tq, Y = np.ascontiguousarray(k.tq[keep]), np.ascontiguousarray(pb.Y[:, keep])
    code, got = lc.call(pkg, emu_model, k, K, Y, None, 1, 0, tq=tq)
    assert code == 0
    code, ones = lc.call(pkg, emu_model, k, K, Y, np.ones_like(Y), 1, 0, tq=tq)
    assert code == 0 and lc.same_bits(got, ones)
    sub = copy.copy(pb)
    sub.S = {0: pb.S[0][:, keep]}
    for c in range(k.n):
        lc.check_cell(sub, K, 0, c, lc.cell_of(got, c), Y[c], np.ones(len(tq)), "w = NULL")
    # with the NaN query among them, every point counts: the cost and what the point enters are NaN
    code, got = lc.call(pkg, emu_model, k, K, pb.Y, None, 1, 0)
    assert code == 0 and np.isnan(got["cost"]).all() and np.isnan(got["grad"]).all() and np.isnan(got["JtJ"]).all()
    assert np.isnan(got["resid"][:, ~keep]).all() and np.isfinite(got["resid"][:, keep]).all()


def test_residual_at_a_saved_time_is_the_saved_value(emu_model, pkg, problems):
    pb = problems["main"]
    k, hits = pb.k, 0
    for ex in (0, 1):
        code, got = lc.call(pkg, emu_model, k, 1, pb.Y, pb.W[ex], 1, ex)
        assert code == 0
        for c in range(k.n):
            which = rc.assign_runs(k, c)
            for r, (row, m) in enumerate(k.runs[c]):
                if m < 2:
                    continue
                for q in np.nonzero((which == r) & (pb.W[ex][c] != 0))[0]:
                    at = np.nonzero(k.t[c, row:row + m] == k.tq[q])[0]
                    if len(at):
                        np.testing.assert_allclose(got["resid"][c, q], pb.W[ex][c, q] * (k.src[c, row + at[0], 0] - pb.Y[c, q]), rtol=1e-14, atol=0)
                        hits += 1
    assert hits >= 24


def test_points_left_out_and_nan_points(emu_model, pkg, problems):
    pb, K = problems["main"], 3
    k = pb.k
    W = pb.W[0].copy()
    finite = np.nonzero(~np.isnan(k.tq))[0]
    out = finite[[2, 40, 66]]                                                                              # (one of them in the second pass of the lanes = queries loop)
    W[:, out] = 0.0
    code, base = lc.call(pkg, emu_model, k, K, pb.Y, W, 1, 0)
    assert code == 0 and (base["resid"][:, out] == 0).all() and np.isfinite(base["cost"]).all()
    # w = 0: the point is not evaluated -- NaN data and a NaN time there change no bit
    Y, tq = pb.Y.copy(), k.tq.copy()
    Y[:, out], tq[out[:2]] = np.nan, np.nan
    code, got = lc.call(pkg, emu_model, k, K, Y, W, 1, 0, tq=tq)
    assert code == 0 and lc.same_bits(got, base)
    # w != 0 and NaN data: cost, grad and that residual are NaN; JtJ does not hold the data
    W2 = W.copy()
    W2[1, out[0]] = 0.7
    code, got = lc.call(pkg, emu_model, k, K, Y, W2, 1, 0, tq=k.tq)
    assert code == 0 and np.isnan(got["cost"][1]) and np.isnan(got["grad"][1]).all() and np.isfinite(got["JtJ"][1]).all()
    assert np.isnan(got["resid"][1, out[0]]) and np.isfinite(np.delete(got["resid"][1], out[0])).all()
    assert lc.same_bits(lc.cell_of(got, 0), lc.cell_of(base, 0)) and lc.same_bits(lc.cell_of(got, 2), lc.cell_of(base, 2))
    # w != 0 and a NaN time: every sum of the cell is NaN (the time is shared: of every cell that weighs it)
    code, got = lc.call(pkg, emu_model, k, K, pb.Y, W2, 1, 0, tq=tq)
    assert code == 0 and np.isnan(got["cost"][1]) and np.isnan(got["grad"][1]).all() and np.isnan(got["JtJ"][1]).all()
    assert lc.same_bits(lc.cell_of(got, 0), lc.cell_of(base, 0)) and lc.same_bits(lc.cell_of(got, 2), lc.cell_of(base, 2))


def test_failed_cell_is_nan_and_its_neighbours_do_not_notice(emu_model, pkg, problems):
    pb, K = problems["main"], 3
    k = pb.k
    code, whole = lc.call(pkg, emu_model, k, K, pb.Y, pb.W[0], 1, 0)
    assert code == 0
    bad = copy.copy(k)
    bad.run_info = k.run_info.copy()
    bad.run_info[1, 1]["flag"] = pkg._capi.ERR_STALL
    bad.src = k.src.copy()
    bad.src[1] = np.nan                                                                                    # (none of its points is read)
    code, got = lc.call(pkg, emu_model, bad, K, pb.Y, pb.W[0], 1, 0)
    assert code == 0 and got["status"].tolist() == [0, 1, 0]
    assert all(np.isnan(got[nm][1]).all() for nm in ("cost", "grad", "JtJ", "resid"))
    for c in (0, 2):
        assert lc.same_bits(lc.cell_of(got, c), lc.cell_of(whole, c))
    code, got0 = lc.call(pkg, emu_model, bad, 0, pb.Y, pb.W[0], 1, 0, want_resid=False)                    # the misfit-only call
    assert code == 0 and np.isnan(got0["cost"][1]) and np.array_equal(got0["cost"][[0, 2]], whole["cost"][[0, 2]])


def test_nan_sensitivities_stay_in_their_cell(emu_model, pkg, problems):
    pb, K = problems["main"], 3
    k = pb.k
    code, whole = lc.call(pkg, emu_model, k, K, pb.Y, pb.W[0], 1, 0)
    V, dV = lc.arrays(k, K)
    dV[2, 1, :int(k.n_pts[2])] = np.nan                                                                    # one row of one cell, as a failed sensitivity leaves it
    code, got = lc.call(pkg, emu_model, k, K, pb.Y, pb.W[0], 1, 0, dV=dV)
    assert code == 0 and (got["status"] == 0).all()
    assert np.isnan(got["grad"][2, 1]) and np.isnan(got["JtJ"][2, 1, :]).all() and np.isnan(got["JtJ"][2, :, 1]).all()
    keep = [0, 2]
    assert np.array_equal(got["grad"][2, keep], whole["grad"][2, keep]) and np.array_equal(got["JtJ"][2][np.ix_(keep, keep)], whole["JtJ"][2][np.ix_(keep, keep)])
    assert lc.same_bits(lc.cell_of(got, 2), lc.cell_of(whole, 2), names=("cost", "resid"))
    for c in (0, 1):
        assert lc.same_bits(lc.cell_of(got, c), lc.cell_of(whole, c))


def test_argument_errors(emu_model, pkg, problems):
    pb, K = problems["main"], 2
    k, lib, h, cap = pb.k, emu_model._lib, emu_model._h, pkg._capi
    V, dV = lc.arrays(k, K)
    nq = len(k.tq)
    y, w = np.ascontiguousarray(pb.Y[0]), np.ascontiguousarray(pb.W[0][0])
    cost, grad, JtJ, resid, status = np.full(k.n, -777.0), np.full((k.n, K), -777.0), np.full((k.n, K, K), -777.0), np.full((k.n, nq), -777.0), np.full(k.n, -7, np.int32)
    P = lambda a: None if a is None else a.ctypes.data

    def go(n=k.n, n_runs=k.n_runs, max_pts=k.max_pts, t=k.t, n_pts=k.n_pts, ri=k.run_info, V=V, n_sens=K, dV=dV, n_q=nq, tq=k.tq, y=y, w=w, per_cell=0, extrapolate=0,
           cost=cost, grad=grad, JtJ=JtJ, kind=cap.PLH_HOST):
        return lib.plh_lsq(h, n, n_runs, max_pts, P(t), P(n_pts), P(ri), P(V), n_sens, P(dV), n_q, P(tq), P(y), P(w), per_cell, extrapolate, P(cost), P(grad), P(JtJ),
                           P(resid), P(status), kind, None)

    assert go() == 0 and (cost != -777.0).all()
    for a in (cost, grad, JtJ, resid):
        a[:] = -777.0
    status[:] = -7
    for kw in (dict(n=0), dict(n_runs=0), dict(max_pts=0), dict(n_q=0), dict(n_q=-2), dict(n_sens=-1), dict(n_sens=cap.LSQ_MAX_SENS + 1), dict(per_cell=2), dict(per_cell=-1),
               dict(extrapolate=2), dict(t=None), dict(n_pts=None), dict(ri=None), dict(V=None), dict(tq=None), dict(y=None), dict(cost=None), dict(dV=None), dict(grad=None),
               dict(JtJ=None), dict(n_sens=0), dict(n_sens=0, dV=None), dict(n_sens=0, dV=None, grad=None), dict(n_sens=0, grad=None, JtJ=None),
               dict(kind=cap.PLH_HOST_ASYNC)):
        assert go(**kw) == rc.E_ARG, kw
        assert lib.plh_last_error()
    assert all((a == -777.0).all() for a in (cost, grad, JtJ, resid)) and (status == -7).all()           # refused before anything ran
    assert go(n_sens=0, dV=None, grad=None, JtJ=None) == 0
    assert lib.plh_lsq(None, k.n, k.n_runs, k.max_pts, P(k.t), P(k.n_pts), P(k.run_info), P(V), K, P(dV), nq, P(k.tq), P(y), P(w), 0, 0, P(cost), P(grad), P(JtJ), None, None,
                       cap.PLH_HOST, None) == rc.E_ARG


def test_chunked_workspace_gives_the_same_bits(emu_model, pkg, monkeypatch):
    """PLH_RESAMPLE_WS_BYTES bounds the slope workspace: the cells go through in chunks (one, then two cells at a time), with the bits of the call in one piece"""
    K = 8
    k = rc.make_case(pkg, cell_points=((5, 9), (1, 2), (70, 3), (4, 4), (2, 30)), width=1 + K, seed=5)
    rng = np.random.default_rng(1)
    Y, W = 4.0 + rng.random((k.n, len(k.tq))), np.where(np.isnan(k.tq), 0.0, 0.5 + rng.random((k.n, len(k.tq))))
    code, whole = lc.call(pkg, emu_model, k, K, Y, W, 1, 0)
    assert code == 0 and (whole["status"] == 0).all() and np.isfinite(whole["JtJ"]).all()
    for budget in (1, 2 * 8 * k.max_pts * (1 + K) + 8192):
        monkeypatch.setenv("PLH_RESAMPLE_WS_BYTES", str(budget))
        code, got = lc.call(pkg, emu_model, k, K, Y, W, 1, 0)
        assert code == 0 and (got["status"] == 0).all() and lc.same_bits(got, whole), budget


def test_reverse_lane_order():
    """The yardstick and chunking tests again with the emulator's lanes run 63..0 between sync points and its LDS and lane stacks starting as garbage (PL_EMU_ORDER=reverse,
    PL_EMU_POISON): an LDS hand-over between the lanes = points and lanes = columns phases that lacks a sync point reads stale data in one of the two orders.  The environment
    is read once per process, hence the subprocess."""
    import subprocess, sys
    env = dict(os.environ, PL_EMU_POISON="1", PL_EMU_ORDER="reverse")
    sel = "(against_the_yardstick and 8-) or chunked"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the Python layer: EnsembleSolution.lsq on a host ensemble (two cells, a run that ends on a bound, then a run that ends on time) ----
def test_ensemble_lsq_on_the_host(emu_model, pkg):
    from test_selected_outputs import PROTO, SOC0, two_cells
    Th = two_cells(pkg, emu_model)
    keys = ["D_sp", "k_p"]
    ens = pkg.simulate_ensemble(emu_model, Th, PROTO, SOC=SOC0, sens=keys)
    t0 = ens.t[0, :int(ens.n_pts[0])]
    rng = np.random.default_rng(4)
    tq = np.concatenate([rng.uniform(0.0, min(ens.t[i, int(ens.n_pts[i]) - 1] for i in range(2)), 30), [t0[3], ens.run_info[0, 0]["t_end"]]])
    data = ens(tq, fields="V").V[0] + 0.01 * np.sin(tq)
    w = 0.5 + rng.random(len(tq))
    fit = ens.lsq(tq, data, weights=w, resid=True)
    assert fit.keys == keys and fit.cost.shape == (2,) and fit.grad.shape == (2, 2) and fit.JtJ.shape == (2, 2, 2) and fit.resid.shape == (2, len(tq)) and (fit.status == 0).all()
    # against scipy on the ensemble's own arrays, within the bounds
    k = rc.Case()
    k.n, k.n_runs, k.max_pts, k.width, k.tq = 2, 2, ens.t.shape[1], 3, tq
    k.t, k.n_pts, k.run_info = ens.t, ens.n_pts, ens.run_info
    k.src = np.concatenate([ens.V[:, :, None], ens.dV_dtheta.transpose(0, 2, 1)], axis=2)
    k.runs = [[(int(sum(ens.run_info[c, :r]["iterations"])), int(ens.run_info[c, r]["iterations"])) for r in range(2)] for c in range(2)]
    pb = lc.Problem()
    pb.k, pb.S = k, {0: rc.fitpack_reference(k, 0)}
    for c in range(2):
        lc.check_cell(pb, 2, 0, c, dict(cost=fit.cost[c], grad=fit.grad[c], JtJ=fit.JtJ[c], resid=fit.resid[c]), data, w, "ens.lsq")
    # per-cell data and weights, no residuals; the misfit-only ensemble
    both = ens.lsq(tq, np.stack([data, data]), weights=np.stack([w, w]))
    assert both.resid is None and np.array_equal(both.cost, fit.cost) and np.array_equal(both.JtJ, fit.JtJ)
    plain = pkg.simulate_ensemble(emu_model, Th, PROTO, SOC=SOC0)
    mis = plain.lsq(tq, data, weights=w)
    assert mis.grad is None and mis.JtJ is None and mis.keys == [] and np.array_equal(mis.cost, fit.cost)
    for args in ((tq, data[:-1]), (tq, np.stack([data] * 3)), (tq[None, :], data), (tq, data, w[:-1])):
        with pytest.raises(ValueError):
            ens.lsq(*args)
    with pytest.raises(ValueError):
        ens.lsq(tq, data, interp_bc="nearest")
    ens.keys = keys * 5                                                                                    # (more than 8 rows of dV_dtheta: refused before the library sees them)
    ens.dV_dtheta = np.concatenate([ens.dV_dtheta] * 5, axis=1)
    with pytest.raises(ValueError, match="8"):
        ens.lsq(tq, data)

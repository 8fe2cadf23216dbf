"""plh_resample / EnsembleSolution.__call__: whole ensembles on one time grid (reference sol(t), src/save_outputs.jl:74-133), here on the wave-emulator build of the device
source (no GPU).  The yardstick is scipy's splrep / splev with s = 0 (FITPACK = the reference's Dierckx), column by column, never the code under test; inputs, yardstick and
the reasoning behind the tolerance are in tests/resample_cases.py."""
import numpy as np
import pytest

import resample_cases as rc
from test_selected_outputs import PROTO, SOC0, two_cells


@pytest.fixture(scope="module")
def case(pkg):
    return rc.make_case(pkg)


@pytest.fixture(scope="module")
def reference(case):
    return {ex: rc.fitpack_reference(case, ex) for ex in (0, 1)}


def test_case_is_what_it_claims(case):
    k = case
    assert k.n == 3 and k.n_runs == 2 and [tuple(m for _, m in r) for r in k.runs] == list(rc.CELL_POINTS)
    assert np.isnan(k.tq).sum() == 1 and (np.diff(k.tq[~np.isnan(k.tq)]) < 0).any()                       # one NaN; unsorted
    t2 = k.t[2, :int(k.n_pts[2])]
    assert (k.tq < 0).any() and (k.tq > t2[-1]).any() and k.run_info[2, 0]["t_end"] in k.tq               # before the first point, after the last, a join
    for c in range(k.n):
        for row, m in k.runs[c]:
            if m >= 2:
                h = np.diff(k.t[c, row:row + m])
                assert 1e-5 <= h[0] <= 1e-2 and (h > 0).all() and h.max() <= 200.0
                assert np.isin(k.t[c, [row, row + m - 1]], k.tq).all()                                    # exact saved times among the queries


def test_restatement_is_as_close_to_fitpack_as_recorded(case, reference):
    """the figure the tolerance is 100 x of, re-measured on these inputs (numpy restatement of the algorithm against FITPACK; no code under test involved)"""
    worst = 0.0
    for ex in (0, 1):
        mine = rc.restatement(case, ex)
        for c in range(case.n):
            worst = max(worst, rc.scaled_error(case, mine, reference[ex], c, rc.mild(case, c)))
    print("restatement vs FITPACK: %.3e of max|column| (recorded bound %.1e, tolerance %.1e)" % (worst, rc.RESTATEMENT_VS_FITPACK, rc.TOL))
    assert 0 < worst <= rc.RESTATEMENT_VS_FITPACK


@pytest.mark.parametrize("extrapolate", (0, 1))
@pytest.mark.parametrize("width", rc.WIDTHS)
def test_against_fitpack(emu_model, pkg, case, reference, width, extrapolate):
    k = case
    code, got, status = rc.call(pkg, emu_model, k, extrapolate, width=width)
    assert code == 0, emu_model._lib.plh_last_error()
    assert (status == 0).all()
    ref = reference[extrapolate][:, :, :width]
    nanq = np.isnan(k.tq)
    assert np.isnan(got[:, nanq]).all() and np.isfinite(got[:, ~nanq]).all()                               # a NaN query gives NaN, nothing else does (no row past n_pts was read)
    for c in range(k.n):
        rows = rc.mild(k, c) if extrapolate else None
        err = rc.scaled_error(k, got, ref, c, rows)
        print("width %d extrapolate %d cell %d: %.3e of max|column| (tolerance %.1e)" % (width, extrapolate, c, err, rc.TOL))
        assert err <= rc.TOL, (c, err)


@pytest.mark.parametrize("extrapolate", (0, 1))
def test_saved_times_return_the_saved_values(emu_model, pkg, case, extrapolate):
    k = case
    code, got, _ = rc.call(pkg, emu_model, k, extrapolate)
    assert code == 0
    hits = 0
    for c in range(k.n):
        which = rc.assign_runs(k, c)
        for r, (row, m) in enumerate(k.runs[c]):
            if m < 2:
                continue
            for q in np.nonzero(which == r)[0]:
                at = np.nonzero(k.t[c, row:row + m] == k.tq[q])[0]
                if len(at):
                    np.testing.assert_allclose(got[c, q], k.src[c, row + at[0]], rtol=1e-14, atol=0)
                    hits += 1
    assert hits >= 12


def test_failed_cell_is_nan_and_its_neighbours_do_not_notice(emu_model, pkg, case):
    import copy
    k = case
    code, whole, _ = rc.call(pkg, emu_model, k, 0, width=65)
    bad = copy.copy(k)
    bad.run_info = k.run_info.copy()
    bad.run_info[1, 1]["flag"] = pkg._capi.ERR_STALL
    bad.src = k.src.copy()
    bad.src[1] = np.nan                                                                                    # (none of its points is read)
    code, got, status = rc.call(pkg, emu_model, bad, 0, width=65)
    assert code == 0 and status.tolist() == [0, 1, 0]
    assert np.isnan(got[1]).all()
    code, without, st2 = rc.call(pkg, emu_model, k, 0, width=65, cells=[0, 2])
    assert code == 0 and st2.tolist() == [0, 0]
    assert np.array_equal(got[[0, 2]], without, equal_nan=True) and np.array_equal(got[[0, 2]], whole[[0, 2]], equal_nan=True)
    # the two other reasons: the output buffer ran full; the point count is not the sum of the runs' (a trajectory cut at max_pts)
    full = copy.copy(k)
    full.run_info = k.run_info.copy()
    full.run_info[2, 1]["flag"] = pkg._capi.ERR_OUTPUT_FULL
    full.n_pts = k.n_pts.copy()
    full.n_pts[0] -= 1
    code, got, status = rc.call(pkg, emu_model, full, 1, width=3)
    assert code == 0 and status.tolist() == [1, 0, 1] and np.isnan(got[[0, 2]]).all() and np.isfinite(got[1][~np.isnan(k.tq)]).all()
    # status may be NULL
    code, got2, untouched = rc.call(pkg, emu_model, full, 1, width=3, want_status=False)
    assert code == 0 and (untouched == -7).all() and np.array_equal(got, got2, equal_nan=True)


def test_argument_errors(emu_model, pkg, case):
    k, lib, h, cap = case, emu_model._lib, emu_model._h, pkg._capi
    t, n_pts, ri, src = k.t, k.n_pts, k.run_info, np.ascontiguousarray(k.src[:, :, :2])
    dst, status = np.full((k.n, len(k.tq), 2), -777.0), np.zeros(k.n, np.int32)
    P = lambda a: None if a is None else a.ctypes.data

    def go(n_runs=k.n_runs, max_pts=k.max_pts, width=2, n_q=len(k.tq), t=t, n_pts=n_pts, ri=ri, src=src, tq=k.tq, dst=dst, extrapolate=0, kind=cap.PLH_HOST):
        return lib.plh_resample(h, k.n, n_runs, max_pts, P(t), P(n_pts), P(ri), width, P(src), n_q, P(tq), extrapolate, P(dst), P(status), kind, None)

    assert go() == 0
    dst[:] = -777.0
    for kw in (dict(n_q=0), dict(n_q=-3), dict(width=0), dict(n_runs=0), dict(max_pts=0), dict(t=None), dict(n_pts=None), dict(ri=None), dict(src=None), dict(tq=None),
               dict(dst=None), dict(extrapolate=2), dict(kind=cap.PLH_HOST_ASYNC)):
        assert go(**kw) == rc.E_ARG, kw
        assert lib.plh_last_error()
    assert (dst == -777.0).all()                                                                           # refused before anything ran
    assert lib.plh_resample(None, k.n, k.n_runs, k.max_pts, P(t), P(n_pts), P(ri), 2, P(src), len(k.tq), P(k.tq), 0, P(dst), None, cap.PLH_HOST, None) == rc.E_ARG


def test_chunked_workspace_gives_the_same_bits(emu_model, pkg, monkeypatch):
    """PLH_RESAMPLE_WS_BYTES bounds the slope workspace: the cells go through in chunks (here one or two cells at a time), with the bits of the call in one piece"""
    k = rc.make_case(pkg, cell_points=((5, 9), (1, 2), (40, 3), (4, 4), (2, 30)), width=70, seed=5)
    code, whole, st = rc.call(pkg, emu_model, k, 1)
    assert code == 0 and (st == 0).all()
    per_cell = 8 * k.max_pts * 70
    for budget in (1, 2 * per_cell + 4096):
        monkeypatch.setenv("PLH_RESAMPLE_WS_BYTES", str(budget))
        code, got, st = rc.call(pkg, emu_model, k, 1)
        assert code == 0 and (st == 0).all() and np.array_equal(got, whole, equal_nan=True), budget


# ---- end to end: a run that ends on a bound, then a run that ends on time (the two-cell protocol of tests/test_selected_outputs.py) ----
@pytest.fixture(scope="module")
def ensembles(emu_model, pkg):
    Th = two_cells(pkg, emu_model)
    full = pkg.simulate_ensemble(emu_model, Th, PROTO, SOC=SOC0, outputs="all")
    part = pkg.simulate_ensemble(emu_model, Th, PROTO, SOC=SOC0, sections=("Φ_s", "c_e"))
    assert (full.run_info["flag"][:, 0] == 4).all() and (full.run_info["flag"][:, 1] == 0).all()
    t = full.t[0, :int(full.n_pts[0])]
    join = full.run_info[0, 0]["t_end"]
    rng = np.random.default_rng(3)
    tq = np.concatenate([rng.uniform(0.0, t[-1], 12), [t[3], join, 0.5 * (join + t[-1]), -0.5 * t[1], t[-1] + 0.5 * (t[-1] - t[-2])]])
    return full, part, tq[rng.permutation(len(tq))]


@pytest.mark.parametrize("interp_bc", ("interpolate", "extrapolate"))
def test_ensemble_call_agrees_with_the_single_cell_spline(ensembles, interp_bc):
    """ens(tq) against ens[i](tq) = Solution.__call__ = scipy per state column, for every array the ensembles hold"""
    full, part, tq = ensembles
    for ens, names in ((full, ("V", "I", "SOC", "Y_all")), (part, ("V", "I", "SOC", "Y_sel"))):
        res = ens(tq, interp_bc=interp_bc)
        assert np.array_equal(res.t, tq) and (res.status == 0).all() and res.sel_ind == ens.sel_ind
        for i in range(2):
            one = ens[i](tq, interp_bc=interp_bc)
            n = int(ens.n_pts[i])
            for nm in names:
                got, ref, saved = getattr(res, nm)[i], getattr(one, nm), getattr(ens, nm)[i, :n]
                assert got.shape == ref.shape
                got, ref, saved = got.reshape(len(tq), -1), ref.reshape(len(tq), -1), saved.reshape(n, -1)
                scale = np.abs(saved).max(axis=0)
                keep = scale > 0                                                                     # (a column that is zero at every saved point is zero at every query)
                assert np.array_equal(got[:, ~keep], ref[:, ~keep])
                worst = float((np.abs(got - ref)[:, keep] / scale[keep]).max())
                print("%s cell %d %s: %.3e of max|column| (tolerance %.1e)" % (nm, i, interp_bc, worst, rc.TOL))
                assert worst <= rc.TOL, (nm, i, worst)
        if ens is part:
            assert np.array_equal(res.section("c_e"), res.Y_sel[:, :, ens.sel_ind["c_e"]]) and res.section("c_e").shape == (2, len(tq), 30)
        else:
            assert np.array_equal(res.section("c_e"), res.Y_all[:, :, ens.p.ind["c_e"]])
    # the selected section is the bits of the full dump's columns (same data, same kernel): both routes to c_e give one answer
    assert np.array_equal(part(tq, interp_bc=interp_bc).section("c_e"), full(tq, interp_bc=interp_bc).section("c_e"))


def test_ensemble_call_fields_and_refusals(ensembles):
    full, part, tq = ensembles
    res = part(tq[:3], fields=("V", "Y_sel"))
    assert res.V.shape == (2, 3) and res.Y_sel.shape == (2, 3, 50) and res.I is None and res.SOC is None and res.Y_all is None
    assert np.array_equal(part(tq[:3], fields="V").V, res.V)
    assert full(float(tq[0])).V.shape == (2, 1)
    with pytest.raises(KeyError):
        part(tq, fields=("Y_all",))
    with pytest.raises(KeyError):
        res.section("j")
    with pytest.raises(ValueError, match=r"ens\[i\]\(t, k="):
        full(tq, k=2)
    with pytest.raises(ValueError):
        full(tq, interp_bc="nearest")

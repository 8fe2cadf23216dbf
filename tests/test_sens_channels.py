"""dI/dtheta and dT_avg/dtheta at every saved point (plh_integrate_sens_out; csrc/dfn_sens.h sens_put_V): what a fit of a constant-voltage leg or of thermocouple data consumes.

Yardstick: the oracle differenced, as parity.oracle_fd_sens does for the voltage -- six tight-tolerance runs per key with common stop times and a step of 5 % of theta,
np.interp of the oracle's I / T at the stop times.  One cell, parity.TIGHT, fixed-tf runs (the run starts do not move with theta); the stop times are run-local and are compared
at global time = run start + stop time.
Criterion per (case, key, channel):  max |device - d6| / max |d6|  <=  1e-4 + 10 gap,  1e-4 being the project's dV/dtheta figure and gap = max |d6 - d4| / max |d6| the
difference between the sixth- and the fourth-order differences of the SAME six oracle runs (no device input).  Every pair is worth measuring: theta max |d6| >= 1e-3 (C-rate, K)
is asserted, nothing is skipped.
Every case runs on the wave emulator and, marked gpu, on the GPU."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import parity

STOPS = np.arange(20.0, 300.0, 20.0)
CASES = {
    # name: model fixture stem, oracle variant, SOC, protocol, keys, stop times, channel, (global times compared at)
    "A": dict(model="", variant="lco_iso_quiet", soc=0.2, keys=["D_sp", "k_n"], stops=STOPS, chan="I", field="I", at=300.0 + np.arange(20.0, 200.0, 20.0),
              proto=[{"I": 2.0, "tf": 300, "V_max": 5.0}, {"V": "hold", "tf": 200, "V_max": 5.0, "I_min": 0.0}]),
    "B": dict(model="", variant="lco_iso", soc=0.9, keys=["D_sp", "k_p"], stops=np.arange(20.0, 200.0, 20.0), chan="I", field="I", at=300.0 + np.arange(20.0, 150.0, 20.0),
              proto=[{"I": -2.0, "tf": 200}, {"I": "rest", "tf": 100}, {"V": 4.0, "tf": 150}]),
    "C": dict(model="_thermal", variant="lco_thermal_tdiff", soc=0.2, keys=["h_cell", "k_p"], stops=np.arange(25.0, 150.0, 25.0), chan="T_avg", field="T",
              at=np.arange(25.0, 150.0, 25.0), proto=[{"I": 3.0, "tf": 150}]),
}
_fd_cache = {}


def oracle_fd(O, pkg, p, name):
    """{key: (d6, d4)} of the case's channel at its comparison times: sixth- and fourth-order central differences of the same six oracle runs (computed once per session)"""
    if name in _fd_cache:
        return _fd_cache[name]
    c = CASES[name]
    th = p.theta_vector()
    runs = parity.runs_to_oracle(O, p, pkg, c["proto"])
    kw = dict(maxiters=400000, tstops=list(c["stops"]), **parity.TIGHT)
    jobs = [(key, f) for key in c["keys"] for f in (3, 2, 1, -1, -2, -3)]

    def run(job):
        key, f = job
        col = p.θ_keys.index(key)
        t2 = th.copy(); t2[col] += f * 0.05 * th[col]
        r = O.simulate(c["variant"], t2, c["soc"], runs, opts=O.default_opts(**kw), max_out=40000)
        assert min(x["flag"] for x in r["runs"]) >= 0, (name, key, f, r["runs"])
        keep = np.concatenate([[True], np.diff(r["t"]) > 0])           # (a run boundary repeats its time: keep the first of the pair)
        return np.interp(c["at"], r["t"][keep], r[c["field"]][keep])
    with ThreadPoolExecutor(min(12, len(os.sched_getaffinity(0)))) as ex:       # (the oracle runs release the GIL)
        g = dict(zip(jobs, ex.map(run, jobs)))
    out = {}
    for key in c["keys"]:
        h = 0.05 * th[p.θ_keys.index(key)]
        d6 = (g[key, 3] / 60 - 3 * g[key, 2] / 20 + 3 * g[key, 1] / 4 - 3 * g[key, -1] / 4 + 3 * g[key, -2] / 20 - g[key, -3] / 60) / h
        d4 = (-g[key, 2] / 12 + 2 * g[key, 1] / 3 - 2 * g[key, -1] / 3 + g[key, -2] / 12) / h
        out[key] = (d6, d4)
    _fd_cache[name] = out
    return out


def tight_opts(pkg, stops=None):
    o = pkg.Opts(); o.reltol, o.abstol, o.maxiters = parity.TIGHT["reltol"], parity.TIGHT["abstol"], 200000
    if stops is not None:
        o.tstops = list(stops)
    return o


def run_case(pkg, p, name):
    c = CASES[name]
    return pkg.simulate_ensemble(p, p.theta_vector()[None, :].copy(), c["proto"], SOC=c["soc"], opts=tight_opts(pkg, c["stops"]), max_points=20000, sens=c["keys"],
                                 sens_outputs=("V", c["chan"]))


def check_case(pkg, p, O, name, where):
    c = CASES[name]
    ens = run_case(pkg, p, name)
    assert (ens.run_info["flag"] >= 0).all() and (np.asarray(ens.sens_stat)[:, 1] == 0).all()
    n = int(ens.n_pts[0]); td = np.asarray(ens.t[0, :n])
    idx = [int(np.argmin(np.abs(td - t))) for t in c["at"]]
    assert np.abs(td[idx] - c["at"]).max() < 1e-6, "a stop time is not among the saved points"
    dev = np.asarray(ens.dI_dtheta if c["chan"] == "I" else ens.dT_avg_dtheta)[0]
    th = p.theta_vector()
    fd = oracle_fd(O, pkg, p, name)
    res = {}
    for k, key in enumerate(c["keys"]):
        d6, d4 = fd[key]
        scale = np.abs(d6).max()
        worth, gap, err = th[p.θ_keys.index(key)] * scale, np.abs(d6 - d4).max() / scale, np.abs(dev[k, idx] - d6).max() / scale
        print("case %s (%s) d%s/d%s: theta max |d6| %.2e, gap %.1e, |device - d6| / max |d6| %.2e (limit %.2e)" % (name, where, c["chan"], key, worth, gap, err, 1e-4 + 10 * gap))
        res[key] = (worth, gap, err)
    for key, (worth, gap, err) in res.items():
        assert worth >= 1e-3, (name, key, worth)                      # no pair is skipped: each is worth measuring
        assert err <= 1e-4 + 10 * gap, (name, key, err, gap)
    return ens


# In a run whose input IS the current (constant I, :rest) the control row is I - value = 0 and dI/dtheta must vanish.  It does so to the rounding of the control row's difference
# quotient: F_theta of that row is (F(theta + d) - F(theta)) / d with both terms exactly I - value, and the directional quotient in s is exact for a linear row, so the corrector
# leaves s[I] at the level of the solve's rounding.  The project's criterion for dV/dtheta at a voltage bound -- 1e-8 of the scale of the quantity where it does move -- is what
# is asserted.
ZERO_REL = 1e-8


def check_zero_in_current_runs(ens, proto, name):
    its = [int(x) for x in ens.run_info[0]["iterations"]]
    start = np.concatenate([[0], np.cumsum(its)])
    dI = np.asarray(ens.dI_dtheta)[0]
    vleg = len(proto) - 1                                             # (both cases end with their voltage leg)
    assert "V" in proto[vleg]
    scale = np.abs(dI[:, start[vleg] + 1:start[vleg + 1]]).max(axis=1)
    assert (scale > 0).all()
    for r in range(vleg):
        seg = np.abs(dI[:, start[r]:start[r + 1]])
        print("case %s run %d (%s): max |dI/dtheta| / max over the voltage leg %s" % (name, r, proto[r], (seg.max(axis=1) / scale).tolist()))
        assert (seg.max(axis=1) <= ZERO_REL * scale).all(), (name, r, seg.max(axis=1), scale)


def _case_with_zero_check(pkg, p, O, name, where):
    ens = check_case(pkg, p, O, name, where)
    check_zero_in_current_runs(ens, CASES[name]["proto"], name)


def test_dI_through_a_hold_leg_emu(emu_model, O, pkg):
    _case_with_zero_check(pkg, emu_model, O, "A", "emulator")


def test_dI_in_a_constant_voltage_leg_emu(emu_model, O, pkg):
    _case_with_zero_check(pkg, emu_model, O, "B", "emulator")


def test_dT_avg_thermal_emu(emu_model_thermal, O, pkg):
    check_case(pkg, emu_model_thermal, O, "C", "emulator")


@pytest.mark.gpu
def test_dI_through_a_hold_leg_gpu(hip_model, O, pkg):
    _case_with_zero_check(pkg, hip_model, O, "A", "GPU")


@pytest.mark.gpu
def test_dI_in_a_constant_voltage_leg_gpu(hip_model, O, pkg):
    _case_with_zero_check(pkg, hip_model, O, "B", "GPU")


@pytest.mark.gpu
def test_dT_avg_thermal_gpu(hip_model_thermal, O, pkg):
    check_case(pkg, hip_model_thermal, O, "C", "GPU")


# ---- a run that ends on a current bound: the derivative of the end state as simulate() returns it -- the current there IS the bound ----
def _current_bound_case(pkg, p):
    proto = [{"I": 2.0, "V_max": 4.0, "tf": 3000.0}, {"V": "hold", "V_max": 4.0, "tf": 3000.0, "I_min": 1 / 20}]
    ens = pkg.simulate_ensemble(p, p.theta_vector()[None, :].copy(), proto, SOC=0.3, opts=tight_opts(pkg), max_points=20000, sens=["D_sp", "k_n"], sens_outputs=("V", "I"))
    assert [int(f) for f in ens.run_info[0]["flag"]] == [2, 8], ens.run_info[0]
    n = int(ens.n_pts[0])
    assert n == int(ens.run_info[0]["iterations"].sum())
    dI = np.asarray(ens.dI_dtheta)[0]
    print("dI/dtheta at the last two points of the run that ended on I_min:", dI[:, n - 2].tolist(), dI[:, n - 1].tolist())
    assert np.isfinite(dI[:, :n]).all() and (np.abs(dI[:, n - 2]) > 0).all()
    assert (np.abs(dI[:, n - 1]) <= 1e-8 * np.abs(dI[:, n - 2])).all(), (dI[:, n - 1], dI[:, n - 2])


def test_dI_of_a_run_that_ends_on_a_current_bound_emu(emu_model, pkg):
    _current_bound_case(pkg, emu_model)


@pytest.mark.gpu
def test_dI_of_a_run_that_ends_on_a_current_bound_gpu(hip_model, pkg):
    _current_bound_case(pkg, hip_model)


# ---- nothing else moves: the old entry with dV only and the new one with every channel are the same kernel ----
THERMAL_PROTO = [{"I": 3.0, "tf": 60.0}, {"V": "hold", "tf": 30.0}]


def two_thermal_cells(p):
    Th = np.tile(p.theta_vector(), (2, 1))
    Th[1, p.θ_keys.index("D_sp")] *= 1.3
    Th[1, p.θ_keys.index("h_cell")] *= 0.7
    return Th


def _same_saved(a, b, names, n_pts):
    for nm in names:
        x, y = np.asarray(getattr(a, nm)), np.asarray(getattr(b, nm))
        for i, k in enumerate(n_pts):                                  # (entries beyond n_pts of the plain per-point arrays are whatever the allocator handed out)
            assert np.array_equal(x[i, ..., :k], y[i, ..., :k], equal_nan=True), nm


def _nothing_else_moves(pkg, p):
    Th, keys = two_thermal_cells(p), ["h_cell", "k_p", "D_sp"]
    old = pkg.simulate_ensemble(p, Th, THERMAL_PROTO, SOC=0.2, sens=keys)
    new = pkg.simulate_ensemble(p, Th, THERMAL_PROTO, SOC=0.2, sens=keys, sens_outputs=("V", "I", "T_avg"))
    assert old.dI_dtheta is None and old.dT_avg_dtheta is None and new.dI_dtheta.shape == new.dV_dtheta.shape == new.dT_avg_dtheta.shape
    assert (old.run_info["flag"] >= 0).all()
    n_pts = [int(k) for k in old.n_pts]
    assert np.array_equal(old.n_pts, new.n_pts) and np.array_equal(np.asarray(old.Y), np.asarray(new.Y)) and np.array_equal(np.asarray(old.YP), np.asarray(new.YP))
    _same_saved(old, new, ("t", "V", "I", "SOC", "T_avg"), n_pts)
    for f in pkg._capi.COUNTER_FIELDS:
        assert np.array_equal(old.counters[f], new.counters[f]), f
    for f in ("flag", "iterations", "t_end", "V", "I", "SOC", "T_avg"):
        assert np.array_equal(old.run_info[f], new.run_info[f]), f
    assert np.array_equal(np.asarray(old.dY_dtheta), np.asarray(new.dY_dtheta)) and np.array_equal(np.asarray(old.sens_stat), np.asarray(new.sens_stat))
    assert np.array_equal(np.asarray(old.dV_dtheta), np.asarray(new.dV_dtheta), equal_nan=True)           # (NaN past n_pts: the prefill)
    for i, k in enumerate(n_pts):
        for a in (new.dI_dtheta, new.dT_avg_dtheta):
            assert np.isfinite(np.asarray(a)[i, :, :k]).all() and np.isnan(np.asarray(a)[i, :, k:]).all()
    assert np.abs(np.asarray(new.dT_avg_dtheta)[0, 0, :n_pts[0]]).max() > 0
    return new


def test_requesting_channels_changes_no_other_bit_emu(emu_model_thermal, pkg):
    _nothing_else_moves(pkg, emu_model_thermal)


@pytest.mark.gpu
def test_requesting_channels_changes_no_other_bit_gpu(hip_model_thermal, pkg):
    host = _nothing_else_moves(pkg, hip_model_thermal)
    # host pointers and device pointers: equal bits
    import torch
    p = hip_model_thermal
    dev = pkg.simulate_ensemble(p, torch.from_numpy(two_thermal_cells(p)).cuda(), THERMAL_PROTO, SOC=0.2, sens=["h_cell", "k_p", "D_sp"], sens_outputs=("V", "I", "T_avg"), device=True)
    torch.cuda.synchronize()
    for nm in ("dY_dtheta", "dV_dtheta", "dI_dtheta", "dT_avg_dtheta", "sens_stat", "Y"):
        assert np.array_equal(getattr(dev, nm).cpu().numpy(), np.asarray(getattr(host, nm)), equal_nan=True), nm
    only_I = pkg.simulate_ensemble(p, torch.from_numpy(two_thermal_cells(p)).cuda(), THERMAL_PROTO, SOC=0.2, sens=["h_cell", "k_p", "D_sp"], sens_outputs=("I",), device=True)
    torch.cuda.synchronize()
    assert only_I.dV_dtheta is None and only_I.dT_avg_dtheta is None and np.array_equal(only_I.dI_dtheta.cpu().numpy(), np.asarray(host.dI_dtheta), equal_nan=True)


def test_dT_avg_of_an_isothermal_model_is_refused(emu_model, pkg):
    p = emu_model
    with pytest.raises(pkg._capi.PetlionHipError, match=r"\(-2\)"):                                       # PLH_E_UNSUPPORTED
        pkg.simulate_ensemble(p, p.theta_vector()[None, :].copy(), [{"I": -1.0, "tf": 10.0}], SOC=0.9, sens=["D_sp"], sens_outputs=("V", "T_avg"))
    with pytest.raises(ValueError, match="sens_outputs"):
        pkg.simulate_ensemble(p, p.theta_vector()[None, :].copy(), [{"I": -1.0, "tf": 10.0}], SOC=0.9, sens=["D_sp"], sens_outputs=("V", "SOC"))


def test_sens_outputs_struct_argument_rules(emu_model, pkg):
    """the C entry itself: a NULL struct and a struct without a derivative array are PLH_E_ARG"""
    import ctypes as C
    p, cap = emu_model, pkg._capi
    runs, _ = pkg.make_protocol(p, [{"I": -1.0, "tf": 5.0}], 1)
    arr = (cap.Run * 1)(*runs)
    th, soc = p.theta_vector()[None, :].copy(), np.array([0.9])
    out = cap.Outputs(); out.max_pts = 64
    ri = np.zeros((1, 1), cap.RUN_INFO_DTYPE); out.run_info = ri.ctypes.data
    os_ = pkg.api._opts_struct(p.opts, p)
    cols = np.array([p.θ_keys.index("D_sp")], np.int32)
    stat = np.zeros((1, 3), np.int32)
    go = lambda so: p._lib.plh_integrate_sens_out(p._h, 1, th.ctypes.data, soc.ctypes.data, 1, arr, C.byref(os_), C.byref(out), 1, cols.ctypes.data, so, cap.PLH_HOST, None)
    assert go(None) == -1
    assert go(C.byref(cap.SensOutputs(None, None, None, None, stat.ctypes.data))) == -1
    dI = np.zeros((1, 1, 64))
    assert go(C.byref(cap.SensOutputs(None, None, dI.ctypes.data, None, None))) == 0 and np.isfinite(dI[0, 0, :2]).all() and (dI[0, 0, :int(ri[0, 0]["iterations"])] == 0).all()


def _failed_cell(pkg, p):
    """two cells with tf of their own; maxiters between their step counts: the long one fails (PLH_ERR_MAXITERS), the short one completes"""
    Th = np.tile(p.theta_vector(), (2, 1))
    proto = lambda tf: [{"I": -1.0, "tf": 20.0}, {"V": "hold", "tf": tf}]
    tf = np.array([5.0, 400.0])
    plain = pkg.simulate_ensemble(p, Th, proto(tf), SOC=0.9)
    it = plain.run_info["iterations"].sum(axis=1)
    assert (plain.run_info["flag"] >= 0).all() and it[0] + 4 < it[1]
    o = pkg.Opts(); o.maxiters = int(plain.run_info["iterations"][0].max() + plain.run_info["iterations"][1, 1]) // 2
    assert plain.run_info["iterations"][0].max() < o.maxiters < plain.run_info["iterations"][1, 1]
    kw = dict(SOC=0.9, opts=o, sens=["D_sp", "k_n"], sens_outputs=("V", "I"))
    both = pkg.simulate_ensemble(p, Th, proto(tf), **kw)
    assert (both.run_info["flag"][0] >= 0).all() and int(both.run_info["flag"][1, 1]) == pkg._capi.ERR_MAXITERS
    alone = pkg.simulate_ensemble(p, Th[:1], proto(tf[:1]), **kw)
    dI, dV = np.asarray(both.dI_dtheta), np.asarray(both.dV_dtheta)
    n0, n1 = int(both.n_pts[0]), int(both.n_pts[1])
    # the failed cell: NaN where dV_dtheta is NaN -- the point the protocol failed at and everything behind it -- and at the end state
    assert np.array_equal(np.isnan(dI[1]), np.isnan(dV[1])) and np.isnan(dI[1, :, n1 - 1:]).all() and np.isfinite(dI[1, :, :n1 - 1]).all()
    assert np.isnan(np.asarray(both.dY_dtheta)[1]).all()
    # its neighbour does not notice
    for nm in ("dI_dtheta", "dV_dtheta", "dY_dtheta"):
        assert np.array_equal(np.asarray(getattr(both, nm))[0], np.asarray(getattr(alone, nm))[0], equal_nan=True), nm
    assert np.isfinite(dI[0, :, :n0]).all() and np.isnan(dI[0, :, n0:]).all()


def test_a_failed_cell_is_nan_and_its_neighbour_does_not_notice_emu(emu_model, pkg):
    _failed_cell(pkg, emu_model)


@pytest.mark.gpu
def test_a_failed_cell_is_nan_and_its_neighbour_does_not_notice_gpu(hip_model, pkg):
    _failed_cell(pkg, hip_model)

"""GPU: the protocols of tests/test_step_boundary_emu.py -- each leaves the normal path of the plain integrate kernel's step boundary in its own way -- on 8 C4 cells
against the oracle, with the criteria tests/test_gpu_parity.py applies to the same quantities: equal flags, t_end within 1e-6 where the stop time does not depend on the step
grid, and every cell's final state within 1e-6 or 10x the cell's own reproducibility floor, never above 1e-4 (assert_within_floor)."""
import numpy as np
import pytest

import parity
from test_gpu_parity import assert_within_floor

pytestmark = pytest.mark.gpu

N_CELLS = 8
ERR_OUTPUT_FULL = -14

# name -> (protocol, device / oracle option overrides)
CASES = {
    "bound": ([{"I": -1.0}], {}),
    "tf_inside_step": ([{"I": -1.0, "tf": 1000.0}], {}),
    "continuation": ([{"I": -1.0, "tf": 600.0}, {"I": "rest", "tf": 600.0}], {}),
    "large_h0": ([{"I": -1.0, "tf": 300.0}], {"init_step": 100.0}),
    "max_order_1": ([{"I": -1.0, "tf": 1500.0}], {"max_order": 1}),
    "max_order_2": ([{"I": -1.0, "tf": 1500.0}], {"max_order": 2}),
    "max_order_5": ([{"I": -1.0, "tf": 300.0}], {"max_order": 5, "reltol": 1e-8, "abstol": 1e-10}),
}


def run_case(pkg, p, proto, okw, **kw):
    o = pkg.Opts()
    for k, v in okw.items():
        setattr(o, k, v)
    Th = pkg.configs.sweep_theta(p, np.arange(N_CELLS), 4)
    return Th, pkg.simulate_ensemble(p, Th, proto, SOC=1.0, opts=o, **kw)


@pytest.mark.parametrize("case", sorted(CASES))
def test_protocol_against_the_oracle(hip_model, O, pkg, case):
    p = hip_model
    proto, okw = CASES[case]
    Th, ens = run_case(pkg, p, proto, okw)
    runs = parity.runs_to_oracle(O, p, pkg, proto)
    rows = []
    for i in range(N_CELLS):
        ro = O.simulate("lco_iso", Th[i], 1.0, runs, opts=O.default_opts(**okw))
        for k, rr in enumerate(ro["runs"]):
            assert ens.run_info[i, k]["flag"] == rr["flag"], (i, k, ens.run_info[i, k], rr)
            assert abs(ens.run_info[i, k]["t_end"] - rr["t_end"]) <= 1e-6 * max(1.0, rr["t_end"]), (i, k, ens.run_info[i, k]["t_end"], rr["t_end"])      # (SOC_min or tf: exact whatever the step grid)
        same = all(ens.run_info[i, k]["iterations"] == rr["iterations"] for k, rr in enumerate(ro["runs"])) and all(
            ens.counters[i][f] == ro["counters"][f] for f in ("n_steps", "n_res", "n_jac", "n_newton", "n_errfail", "n_convfail"))
        err = parity.state_rel_err(ens.Y[i], ro["Y"])
        band = 0.0 if err <= 1e-6 else parity.oracle_noise_band(O, "lco_iso", Th[i], 1.0, runs, okw)[1]      # (the floor only matters to a cell above 1e-6: seven oracle runs)
        rows.append((bool(same), err, band))
    assert_within_floor(rows, "step boundary, " + case)
    # the path the case is about was taken, on the device
    flags, c = ens.run_info["flag"], ens.counters
    if case == "bound":
        assert (flags[:, 0] == 3).all()
    elif case == "tf_inside_step":
        assert (flags[:, 0] == 0).all() and (ens.run_info["t_end"][:, 0] == 1000.0).all()
    elif case == "continuation":
        t1 = np.nextafter(600.0, 1e300) + 1.0
        assert (flags == 0).all() and all((np.asarray(ens.t[i, :int(ens.n_pts[i])]) == t1).any() for i in range(N_CELLS))
    elif case == "large_h0":
        _, base = run_case(pkg, p, proto, {})
        assert (c["n_errfail"] > base.counters["n_errfail"]).any()
    elif case == "max_order_1":
        assert (c["sum_kp2"] == 3 * c["n_steps"]).all()
    elif case == "max_order_2":
        assert (c["sum_kp2"] <= 4 * c["n_steps"]).all() and (c["sum_kp2"] > 3.5 * c["n_steps"]).any()
    else:
        assert (c["sum_kp2"] > 6 * c["n_steps"]).any()                  # mean order above 4: order 5 was used


def test_output_buffer_full_against_the_oracle(hip_model, O, pkg):
    """max_points = 12: the device ends the run on PLH_ERR_OUTPUT_FULL at its 12th point.  The oracle has no such limit: the device's points and its final state are compared
    with the first 12 points of the oracle's full run and the state saved there, as parity.compare_trajectory compares points and states."""
    p = hip_model
    proto, mp, rtol = [{"I": -1.0}], 12, 1e-6
    Th, ens = run_case(pkg, p, proto, {}, max_points=mp)
    runs = parity.runs_to_oracle(O, p, pkg, proto)
    assert (ens.run_info["flag"][:, 0] == ERR_OUTPUT_FULL).all() and (np.asarray(ens.n_pts) == mp).all()
    for i in range(N_CELLS):
        ro = O.simulate("lco_iso", Th[i], 1.0, runs, keep_Y=True)
        t, V = np.asarray(ens.t[i, :mp]), np.asarray(ens.V[i, :mp])
        assert np.abs(t - ro["t"][:mp]).max() <= 10 * rtol * max(1.0, ro["t"][mp - 1])
        dt = np.abs(t - ro["t"][:mp])
        sl = np.abs(np.diff(ro["V"][:mp + 1])) / np.diff(ro["t"][:mp + 1])
        slope = np.maximum(np.r_[0.0, sl[:-1]], sl)
        assert (np.abs(V - ro["V"][:mp]) <= 10 * rtol * 4.0 + 2 * slope * dt).all()
        assert parity.state_rel_err(np.asarray(ens.Y[i]), ro["Y_all"][mp - 1]) <= rtol, (i, parity.state_rel_err(np.asarray(ens.Y[i]), ro["Y_all"][mp - 1]))

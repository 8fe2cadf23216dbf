"""CPU-side checks of the DEVICE SOURCE (petlion.jl_amd/csrc/*.h, *.hip) through the test-only lock-step wave emulator
(tests/wave_emu): the same C ABI, the same kernels, 64 emulated lanes.  The GPU versions of these checks are in
test_gpu_parity.py; this file is what keeps the device code testable in a container without a GPU."""
import os

import numpy as np
import pytest

import parity


def test_keys_and_jacobian_pattern(emu_model, O):
    parity.check_keys_and_pattern(emu_model, O)


def test_evaluators_residual_jacobian_solve(emu_model, O):
    parity.check_evaluators(emu_model, O, n_cells=3)


def test_consistent_initialisation(emu_model, O):
    parity.check_init(emu_model, O)


def test_cc_discharge_trajectory_same_decisions(emu_model, O, pkg):
    p = emu_model
    Th = pkg.theta_matrix(p, 2, {"D_sp": np.array([1.0, 0.6]) * p.θ["D_sp"]})
    ens = pkg.simulate_ensemble(p, Th, [{"I": -1.0}], SOC=1.0)
    for i in range(2):
        ro = O.simulate("lco_iso", Th[i], 1.0, parity.runs_to_oracle(O, p, pkg, [{"I": -1.0}]))
        parity.compare_trajectory(ens, i, ro, rtol_state=1e-6)
    assert abs(ens.run_info[0, 0]["t_end"] - 3600.0) < 1e-6          # reference getting_started.ipynb:100-108


def test_cc_cv_with_fresh_jacobians(emu_model, O, pkg):
    """CC -> V=:hold.  With a fresh Jacobian every step both implementations agree to 1e-7; under IDA's Jacobian-reuse policy
    the CV leg is only reproducible to the integration tolerance ('parity of CV legs')."""
    p = emu_model
    proto = [{"I": 2.0, "tf": 1800.0, "V_max": 4.1}, {"V": "hold", "V_max": 4.1, "I_min": 1 / 20}]
    o = pkg.Opts(); o.jac_every_step = True
    ens = pkg.simulate_ensemble(p, pkg.theta_matrix(p, 1), proto, SOC=0.0, opts=o)
    ro = O.simulate("lco_iso", p.theta_vector(), 0.0, parity.runs_to_oracle(O, p, pkg, proto), opts=O.default_opts(jac_every_step=1))
    parity.compare_trajectory(ens, 0, ro, rtol_state=1e-6)
    ens2 = pkg.simulate_ensemble(p, pkg.theta_matrix(p, 1), proto, SOC=0.0)
    ro2 = O.simulate("lco_iso", p.theta_vector(), 0.0, parity.runs_to_oracle(O, p, pkg, proto))
    assert [int(f) for f in ens2.run_info[0]["flag"]] == [r["flag"] for r in ro2["runs"]] == [2, 4]
    assert abs(ens2.run_info[0, 0]["t_end"] - ro2["runs"][0]["t_end"]) < 1e-6 * ro2["runs"][0]["t_end"]      # CC leg: tight
    assert abs(ens2.run_info[0, 1]["t_end"] - ro2["runs"][1]["t_end"]) < 2e-3 * ro2["runs"][1]["t_end"]      # CV leg: reltol
    assert abs(ens2.run_info[0, 1]["I"] - ro2["runs"][1]["I"]) < 1e-2 * ro2["runs"][1]["I"]


def test_c4_sweep_cells_pinned_initial_step(emu_model, O, pkg):
    """6 cells of the C4 parameter sweep with h0 pinned: same decisions, end state to 1e-6 (see test_gpu_parity.py for the
    tolerance structure with the automatic h0)."""
    import test_gpu_parity as tg
    o = pkg.Opts(); o.init_step = 1e-2
    rows = tg.sweep_check(pkg, emu_model, O, 6, opts=o, oopts_kw=dict(init_step=1e-2))
    assert all(r[0] for r in rows) and max(r[1] for r in rows) <= 1e-6, rows


def test_c4_cells_within_the_reference_reproducibility_floor(emu_model, O, pkg):
    """default options (automatic h0): every cell within 1e-6 or within 10x its own reproducibility floor; cell 9 of the sweep is one whose floor is above
    1e-6 (a discharge that ends on the voltage knee).  test_gpu_parity.py explains the criterion."""
    import test_gpu_parity as tg
    rows = tg.sweep_check(pkg, emu_model, O, 0, cells=[0, 2, 9])
    tg.assert_within_floor(rows, "emulator, C4 cells 0, 2, 9")
    assert rows[2][2] > 1e-6          # the oracle alone is not reproducible to 1e-6 for this cell


def test_linear_solver_accuracy_against_extended_precision(emu_model, emu_model_sei, emu_model_thermal, O):
    """structured device solve (emulated) and oracle sparse LU against an 80-bit extended-precision solution: see tools/solve_accuracy.py"""
    for p in (emu_model, emu_model_sei, emu_model_thermal):
        parity.check_solver_accuracy(p, O)


def test_nmc_chemistry_evaluators_and_discharge(emu_model_nmc, O, pkg):
    """second chemistry (NMC / LiC6_NMC, reference src/params.jl:295-507): nonlinear D_eff(c_e,T), its own OCVs, brugg = 1.5"""
    p = emu_model_nmc
    parity.check_keys_and_pattern(p, O)
    parity.check_evaluators(p, O, n_cells=3)
    parity.check_init(p, O, None)
    Th = pkg.theta_matrix(p, 1)
    ens = pkg.simulate_ensemble(p, Th, [{"I": -1.0}], SOC=1.0)
    ro = O.simulate("nmc_iso", Th[0], 1.0, parity.runs_to_oracle(O, p, pkg, [{"I": -1.0}]))
    assert ro["runs"][0]["flag"] == 1                      # NMC bounds: V_min = 2.8 fires before SOC_min
    parity.compare_trajectory(ens, 0, ro, rtol_state=1e-6)


GITT_SEI = [{"I": 1.0, "tf": 300.0}, {"I": "rest", "tf": 300.0}, {"I": -0.5, "tf": 300.0}, {"I": "rest", "tf": 200.0}, {"I": 1.0, "tf": 300.0}]


def check_sei_model(p, O, pkg):
    """aging = :SEI (film, SOH, j_s rows; reference residuals.jl:260-297,519-552): evaluators, consistent initialisation, a CC charge
    with identical step decisions, and a pulse/rest chain with IDA's first step pinned (the default first step amplifies the
    finite-difference YP_alg estimate of newtons_method!, DESIGN.md "reproducibility floor")."""
    parity.check_keys_and_pattern(p, O)
    parity.check_evaluators(p, O, n_cells=3)
    parity.check_init(p, O, None)
    th = p.theta_vector()
    proto = [{"I": 1.0, "tf": 1500.0}]
    ens = pkg.simulate_ensemble(p, th[None, :], proto, SOC=0.0)
    ro = O.simulate(p.variant, th, 0.0, parity.runs_to_oracle(O, p, pkg, proto))
    parity.compare_trajectory(ens, 0, ro, rtol_state=1e-6)
    film = ens.Y[0][230:240]
    assert (film > 0).all() and ens.Y[0][240] < 1.0          # the side reaction ran: film grew, SOH dropped
    o = pkg.Opts(); o.jac_every_step = True; o.init_step = 1e-2
    ens = pkg.simulate_ensemble(p, th[None, :], GITT_SEI, SOC=0.3, opts=o)
    ro = O.simulate(p.variant, th, 0.3, parity.runs_to_oracle(O, p, pkg, GITT_SEI), opts=O.default_opts(jac_every_step=1, init_step=1e-2))
    parity.compare_trajectory(ens, 0, ro, rtol_state=1e-6)


def test_lco_sei_aging(emu_model_sei, O, pkg):
    check_sei_model(emu_model_sei, O, pkg)


def test_nmc_sei_aging_c5_model(emu_model_nmc_sei, O, pkg):
    check_sei_model(emu_model_nmc_sei, O, pkg)


CC_CT_CV_KW = dict(T_max=313.15, V_max=4.1, I_max=4.0, I_min=1 / 20)
CC_CT_CV = [dict(I=4.0, **CC_CT_CV_KW), dict(dT="hold", **CC_CT_CV_KW), dict(V="hold", **CC_CT_CV_KW)]


def check_thermal_model(p, O, pkg, Th=None, cells=(0,)):
    """temperature = true (config C3's model): evaluators in the I / V / dT modes, consistent initialisation, the CC leg with identical
    step decisions at 1e-6, and the reference's CC-CT-CV fast-charge protocol (examples/fast_charging_CC-CT-CV.ipynb).
    The dT control row sums 50 nearly cancelling conduction terms (flux conservation), so the current found by its algebraic twin
    carries ~1e-6 relative round-off in the reference formulation itself; the CT/CV legs are therefore compared at 1e-3 like the
    notebook KATs, and the CC leg at 1e-6."""
    import json, os
    parity.check_keys_and_pattern(p, O)
    parity.check_evaluators(p, O, n_cells=2)
    parity.check_init(p, O, None)
    if Th is None:
        Th = p.theta_vector()[None, :]
    ens1 = pkg.simulate_ensemble(p, Th, CC_CT_CV[:1], SOC=0.0)
    ens = pkg.simulate_ensemble(p, Th, CC_CT_CV, SOC=0.0)
    o = pkg.Opts(); o.jac_every_step = True
    ensj = pkg.simulate_ensemble(p, Th, CC_CT_CV, SOC=0.0, opts=o)
    G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "notebook_kats.json")))
    for i in cells:
        ro1 = O.simulate(p.variant, Th[i], 0.0, parity.runs_to_oracle(O, p, pkg, CC_CT_CV[:1]))
        parity.compare_trajectory(ens1, i, ro1, rtol_state=1e-6)
        if ro1["runs"][0]["flag"] == 5:
            assert abs(ens1.run_info[i, 0]["T_avg"] - 313.15) < 1e-6                                  # stopped on T_max, back-interpolated
        # whole protocol with a fresh Jacobian every step.  CC leg: same step sequence, stop time to 1e-4.  The CT leg starts from a current
        # that its algebraic twin only defines to ~1e-6 (see the docstring), so its step sequence may differ: stop time to 1e-3.
        roj = O.simulate(p.variant, Th[i], 0.0, parity.runs_to_oracle(O, p, pkg, CC_CT_CV), opts=O.default_opts(jac_every_step=1))
        for k, rr in enumerate(roj["runs"]):
            info = ensj.run_info[i, k]
            assert info["flag"] == rr["flag"] and abs(int(info["iterations"]) - rr["iterations"]) <= (2 if k == 0 else 0.15 * rr["iterations"]), (i, k, info, rr)
            assert abs(info["t_end"] - rr["t_end"]) <= (1e-4, 1e-3, 1e-2)[k] * rr["t_end"], (i, k, info, rr)
            assert abs(info["T_avg"] - rr["T_avg"]) < (2e-2 if k < 2 else 0.2) and abs(info["SOC"] - rr["SOC"]) < (1e-4, 1e-3, 2e-3)[k]
        # default options (Jacobian reuse): the step sequences may differ within the integration tolerance; the reference's
        # linear back-interpolation over the last step then moves the stop time by O(h^2)
        ro = O.simulate(p.variant, Th[i], 0.0, parity.runs_to_oracle(O, p, pkg, CC_CT_CV))
        # the hold legs (dT = :hold, V = :hold) start from set points and predictor histories that carry the rounding noise of the legs before them: the oracle's own
        # spread under evaluation-rounding-sized perturbations (orc_opts.fd_perturb, see test_gpu_parity.py) bounds what a second implementation can reproduce
        pert = [O.simulate(p.variant, Th[i], 0.0, parity.runs_to_oracle(O, p, pkg, CC_CT_CV), opts=O.default_opts(fd_perturb=2.2e-16, perturb_seed=sd)) for sd in (1, 2, 3, 4)]
        for k, rr in enumerate(ro["runs"]):
            info = ens.run_info[i, k]
            it_band = max(abs(q["runs"][k]["iterations"] - rr["iterations"]) for q in pert)
            te_band = max(abs(q["runs"][k]["t_end"] - rr["t_end"]) for q in pert)
            assert info["flag"] == rr["flag"] and abs(int(info["iterations"]) - rr["iterations"]) <= max(2, 0.15 * rr["iterations"], 3 * it_band), (i, k, info, rr, it_band)
            assert abs(info["t_end"] - rr["t_end"]) <= max((2e-3 if k < 2 else 1e-2) * rr["t_end"], 3 * te_band) and abs(info["I"] - rr["I"]) <= 3e-2 * abs(rr["I"]), (i, k, info, rr)
            assert abs(info["T_avg"] - rr["T_avg"]) < (2e-2 if k < 2 else 0.2) and abs(info["SOC"] - rr["SOC"]) < 2e-3
        if ro["runs"][0]["flag"] == 5:
            assert abs(ens.run_info[i, 1]["T_avg"] - 313.15) < 1e-4                                    # the CT leg holds 40 C
    if np.array_equal(Th[0], p.theta_vector()):       # default parameters: the notebook's printed values
        for key, info in zip(("thermal_4C", "thermal_dT_hold", "thermal_V_hold"), ens.run_info[0]):
            k = G["runs"][key]
            assert info["flag"] == k["flag"] and abs(info["t_end"] - k["t_end"]) <= k["tol"]["t_end_rel"] * k["t_end"], (key, info)


def test_lco_thermal_cc_ct_cv(emu_model_thermal, O, pkg):
    check_thermal_model(emu_model_thermal, O, pkg)


def check_lgm50_thermal(p, O, pkg):
    """NMC_LGM50 + LiC6_LGM50 with temperature = true -- the reference's DEFAULT configuration of that chemistry (src/params.jl:695): K_eff(c_e), D_eff(c_e) per control volume,
    tanh OCVs with dU/dT = 0, Arrhenius k and D_s per node; 54 parameters.  Oracle variant lgm50_thermal (equations only: the reference holds no vector for this chemistry)."""
    assert p.temperature and p.variant == "lgm50_thermal" and len(p.θ_keys) == 54
    parity.check_keys_and_pattern(p, O)
    # (the solve is compared with the oracle's sparse LU at 1e-7 here and with an 80-bit solution below: on this chemistry -- sigma_p = 0.18 S/m -- the ORACLE's LU is the
    #  less accurate of the two, 1.9e-8 from the truth in the V mode where the structured solve is within 3e-10)
    parity.check_evaluators(p, O, n_cells=3, solve_tol=1e-7)
    rows = np.array([r[3:] for r in parity.solver_accuracy_rows(p, O, n_states=2, modes=((0, -1.0), (1, 3.9), (2, 0.01)))])
    assert rows[:, 0].max() <= 2e-9, rows[:, 0].max()
    parity.check_init(p, O, None)
    Th = pkg.theta_matrix(p, 2, {"h_cell": np.array([1.0, 5.0]) * p.θ["h_cell"]})
    ens = pkg.simulate_ensemble(p, Th, [{"I": -1.0}], SOC=1.0)
    for i in range(2):
        ro = O.simulate(p.variant, Th[i], 1.0, parity.runs_to_oracle(O, p, pkg, [{"I": -1.0}]))
        parity.compare_trajectory(ens, i, ro, rtol_state=2e-6)
    assert ens.run_info[0, 0]["T_avg"] > 305.0                               # a 1C discharge heats this cell by ~9 K (sigma_p = 0.18 S/m)
    kw = dict(T_max=313.15, V_max=4.2, I_min=1 / 20)
    proto = [dict(I=2.0, **kw), dict(dT="hold", **kw), dict(V="hold", **kw)]
    ens = pkg.simulate_ensemble(p, Th[:1], proto, SOC=0.0)
    ro = O.simulate(p.variant, Th[0], 0.0, parity.runs_to_oracle(O, p, pkg, proto))
    assert [int(f) for f in ens.run_info[0]["flag"]] == [r["flag"] for r in ro["runs"]] == [5, 2, 8]
    assert int(ens.run_info[0, 0]["iterations"]) == ro["runs"][0]["iterations"] and abs(ens.run_info[0, 0]["t_end"] - ro["runs"][0]["t_end"]) < 1e-6 * ro["runs"][0]["t_end"]
    for k in (1, 2):
        assert abs(ens.run_info[0, k]["t_end"] - ro["runs"][k]["t_end"]) < (2e-3, 1e-2)[k - 1] * ro["runs"][k]["t_end"], k


def test_lgm50_with_temperature(emu_model_lgm50_thermal, O, pkg):
    check_lgm50_thermal(emu_model_lgm50_thermal, O, pkg)


def check_power_and_plating_modes(p, O, pkg):
    """constant / held power `P` and plating overpotential `η_p` (reference input_methods.jl:80-152, scalar_residual.jl:189-225): single runs
    with identical step decisions at 1e-6; chained :hold / :rest legs with a fresh Jacobian every step and IDA's first step pinned (reproducibility floor)."""
    th = p.theta_vector()
    I1C = p.θ["I1C"]
    for proto, soc in (([{"P": -3.7 * I1C, "tf": 1800.0}], 1.0), ([{"η_p": 0.08, "tf": 600.0, "I_max": 10.0}], 0.2)):
        ens = pkg.simulate_ensemble(p, th[None, :], proto, SOC=soc)
        ro = O.simulate(p.variant, th, soc, parity.runs_to_oracle(O, p, pkg, proto))
        parity.compare_trajectory(ens, 0, ro, rtol_state=1e-6)
    o = pkg.Opts(); o.jac_every_step = True; o.init_step = 1e-2
    for proto, soc in (([{"I": -1.0, "tf": 600.0}, {"P": "hold", "tf": 600.0}, {"P": "rest", "tf": 100.0}], 1.0),
                       ([{"I": 2.0, "tf": 900.0}, {"η_p": "hold", "tf": 600.0}], 0.1)):
        ens = pkg.simulate_ensemble(p, th[None, :], proto, SOC=soc, opts=o)
        ro = O.simulate(p.variant, th, soc, parity.runs_to_oracle(O, p, pkg, proto), opts=O.default_opts(jac_every_step=1, init_step=1e-2))
        # (an error test close to its threshold may flip in a later step: compare end states at the integration-tolerance level)
        parity.compare_trajectory(ens, 0, ro, rtol_state=5e-3, same_decisions=False)      # reltol = 1e-3 level (relaxing fields)
        for a, b in zip(ens.run_info[0], ro["runs"]):
            assert abs(a["V"] - b["V"]) < 5e-4 and abs(a["I"] - b["I"]) < 5e-4 and abs(a["SOC"] - b["SOC"]) < 1e-5
        assert max(abs(int(a["iterations"]) - b["iterations"]) for a, b in zip(ens.run_info[0], ro["runs"])) <= 3
    # the held power really is the power at the end of the CC leg
    ens = pkg.simulate_ensemble(p, th[None, :], [{"I": -1.0, "tf": 600.0}, {"P": "hold", "tf": 600.0}], SOC=1.0)
    P0 = ens.run_info[0, 0]["I"] * I1C * ens.run_info[0, 0]["V"]
    assert abs(ens.run_info[0, 1]["I"] * I1C * ens.run_info[0, 1]["V"] - P0) < 1e-6 * abs(P0)


def test_power_and_plating_overpotential_modes(emu_model, O, pkg):
    check_power_and_plating_modes(emu_model, O, pkg)


def check_stop_conditions(p, O, pkg):
    """every boundary_stop_condition of the reference (src/checks.jl:31-224; flags 1..11) fires on the same step and back-interpolates to the
    same point as the oracle; plus check_bounds = false, interp_final = false and the output-buffer guard."""
    th = p.theta_vector()
    cases = [
        ("V_min", [{"I": -2.0, "V_min": 3.6}], 1.0, 1),
        ("V_max", [{"I": 1.0, "V_max": 3.95}], 0.3, 2),
        ("SOC_min", [{"I": -1.0, "SOC_min": 0.6}], 1.0, 3),
        ("SOC_max", [{"I": 1.0, "SOC_max": 0.5}], 0.2, 4),
        ("c_s_n_max", [{"I": 2.0, "c_s_n_max": 0.6}], 0.2, 6),
        ("I_max", [{"V": 4.05, "I_max": 2.5, "tf": 600.0}], 0.6, None),      # fires only if the voltage step demands more than I_max
        ("I_min", [{"I": 1.0, "tf": 600.0}, {"V": "hold", "I_min": 0.3}], 0.3, 8),
        ("c_e_min", [{"I": -3.0, "c_e_min": 600.0}], 1.0, 9),
        ("η_plating_min", [{"I": 3.0, "η_plating_min": 0.02}], 0.2, 11),
    ]
    if p.aging:
        cases.append(("dfilm_max", [{"I": 1.0, "tf": 200.0}, {"I": 3.0, "dfilm_max": 2e-15}], 0.3, 10))
    for name, proto, soc, flag in cases:
        ens = pkg.simulate_ensemble(p, th[None, :], proto, SOC=soc)
        ro = O.simulate(p.variant, th, soc, parity.runs_to_oracle(O, p, pkg, proto))
        got = int(ens.run_info[0, -1]["flag"])
        assert got == ro["runs"][-1]["flag"], (name, got, ro["runs"][-1])
        if flag is not None:
            assert got == flag, (name, got)
        if len(proto) == 1:
            parity.compare_trajectory(ens, 0, ro, rtol_state=1e-5)      # identical decisions; state floor of DESIGN.md section 5
        else:
            assert abs(ens.run_info[0, -1]["t_end"] - ro["runs"][-1]["t_end"]) <= 2e-3 * ro["runs"][-1]["t_end"], name
    # check_bounds = false: runs to tf whatever the states do (flag 0); interp_final = false: the last point is the overshooting step
    o = pkg.Opts(); o.check_bounds = False
    ens = pkg.simulate_ensemble(p, th[None, :], [{"I": -1.0, "tf": 500.0, "V_min": 4.0}], SOC=1.0, opts=o)
    ro = O.simulate(p.variant, th, 1.0, parity.runs_to_oracle(O, p, pkg, [{"I": -1.0, "tf": 500.0, "V_min": 4.0}]), opts=O.default_opts(check_bounds=0))
    assert ens.run_info[0, 0]["flag"] == 0 == ro["runs"][0]["flag"] and abs(ens.run_info[0, 0]["t_end"] - 500.0) < 1e-9
    o = pkg.Opts(); o.interp_final = False
    ens = pkg.simulate_ensemble(p, th[None, :], [{"I": -1.0, "V_min": 3.8}], SOC=1.0, opts=o)
    ro = O.simulate(p.variant, th, 1.0, parity.runs_to_oracle(O, p, pkg, [{"I": -1.0, "V_min": 3.8}]), opts=O.default_opts(interp_final=0))
    assert ens.run_info[0, 0]["flag"] == 1 and ens.run_info[0, 0]["V"] < 3.8 and abs(ens.run_info[0, 0]["t_end"] - ro["runs"][0]["t_end"]) < 1e-5 * ro["runs"][0]["t_end"]
    # output buffers smaller than the trajectory: the cell reports PLH_ERR_OUTPUT_FULL (-14) instead of writing out of bounds
    ens = pkg.simulate_ensemble(p, th[None, :], [{"I": -1.0}], SOC=1.0, max_points=16)
    assert ens.run_info[0, 0]["flag"] == -14 and int(ens.n_pts[0]) == 16


def test_every_stop_condition(emu_model, O, pkg):
    check_stop_conditions(emu_model, O, pkg)


def test_dfilm_stop_condition(emu_model_sei, O, pkg):
    p = emu_model_sei
    th = p.theta_vector()
    proto = [{"I": 1.0, "tf": 200.0}, {"I": 3.0, "dfilm_max": 2e-15}]
    ens = pkg.simulate_ensemble(p, th[None, :], proto, SOC=0.3)
    ro = O.simulate(p.variant, th, 0.3, parity.runs_to_oracle(O, p, pkg, proto))
    assert int(ens.run_info[0, -1]["flag"]) == ro["runs"][-1]["flag"] == 10          # "Above max. film growth rate", checks.jl:203-224
    assert abs(ens.run_info[0, -1]["t_end"] - ro["runs"][-1]["t_end"]) < 1e-6 * ro["runs"][-1]["t_end"]


def check_function_inputs(p, O, pkg):
    """time-dependent inputs (reference run_function: `simulate(p, tf, I = t -> ...)`) as piecewise-linear tables, `tdiscon` tstops and
    check_reinitialization! (model_evaluation.jl:295-297, checks.jl:251-269, 341-364); the first four cases are the notebook's
    (examples/variable_input_functions.ipynb), whose printed results pin the oracle in tests/test_oracle_golden.py."""
    th = p.theta_vector()
    tt = np.linspace(0, 10, 201)
    cases = [("step_td", [{"I": ([0, 100, 100, 200], [1, 1, 0.5, 0.5]), "tf": 200.0}], 0.0, [100.0], True),
             ("step", [{"I": ([0, 100, 100, 200], [1, 1, 0.5, 0.5]), "tf": 200.0}], 0.0, [], False),      # the jump is crossed by step-size collapse
             ("ramp", [{"I": ([0, 100], [0, 1.0]), "tf": 100.0}], 0.0, [], True),
             ("ramp10", [{"I": ([0, 100], [0, 10.0]), "tf": 100.0}], 0.0, [], False),   # same steps; one Newton stop test sits on its threshold (2 extra iterations)
             ("P_sin", [{"P": (tt, 29.23 * np.sin(tt)), "tf": 10.0}], 0.5, [], False),      # starts from zero power: the first steps are set by round-off
             ("V_cos", [{"V": (tt, 3.9 + 0.05 * np.cos(tt)), "tf": 10.0}], 0.5, [], True),
             ("cc_then_drive", [{"I": -1.0, "tf": 300.0}, {"I": ([0, 50, 50, 120, 120, 200], [-1, -2, 0.5, 0.5, -1.5, -1.5]), "tf": 200.0}], 1.0, [50.0, 120.0], True)]
    for name, proto, soc, td, same in cases:
        o = pkg.Opts(); o.tdiscon = td
        ens = pkg.simulate_ensemble(p, th[None, :], proto, SOC=soc, opts=o)
        ro = O.simulate(p.variant, th, soc, parity.runs_to_oracle(O, p, pkg, proto), opts=O.default_opts(tdiscon=td))
        parity.compare_trajectory(ens, 0, ro, rtol_state=5e-6, same_decisions=same)
    check_closure_inputs(p, O, pkg)


def check_closure_inputs(p, O, pkg):
    """input closures `I = (t, Y, YP, p) -> ...` traced into the C ABI's postfix programs (PLH_VAL_EXPR; petlion.jl_amd/closures.py): the notebook's P = sin(t) and
    V = 3.5 + 0.1 cos(t) (examples/variable_input_functions.ipynb) evaluated exactly instead of through a sampled table, a ramp whose slope is a model parameter of the cell, a
    step written with where() + tdiscon, and closures of the STATE (a current that tapers with the cell voltage; one that reads YP).  The oracle runs the same programs
    (ORC_VAL_EXPR): same decisions, state 5e-6."""
    cl = pkg.closures
    th = p.theta_vector()
    P1 = 29.23                                                     # (1C power scale of this cell, W/m^2: the notebook's sin(t) is in the reference's power unit)
    cases = [("P_sin", [{"P": lambda t: P1 * cl.sin(t), "tf": 10.0}], 0.5, [], False),
             ("V_cos", [{"V": lambda t: 3.9 + 0.05 * np.cos(t), "tf": 10.0}], 0.5, [], True),
             ("ramp_theta", [{"I": lambda t, q: q.θ["t₊"] * t / 36.4, "tf": 100.0}], 0.0, [], True),          # slope from a theta entry of the cell (0.364 / 36.4 = 1/100)
             ("step_where", [{"I": lambda t: cl.where(t < 100, 1.0, 0.5), "tf": 200.0}], 0.0, [100.0], True),
             ("taper_V", [{"I": lambda t, Y, q: -cl.minimum(1.0, cl.maximum(0.05, (cl.calc_V(Y, q) - 3.0) * 2.0)), "tf": 4000.0, "V_min": 3.05}], 1.0, [], True),
             # closures of the state: their symbolic derivative goes into the control row of the Newton matrix (scalar_residual.jl:276-416; closures.row_derivatives ->
             # plh_run.dcol / dofs): a current that depends on a DIFFERENTIAL state, a voltage set-point that depends on the current (without the derivative the control row
             # has no I entry left to pivot on), a power that follows the voltage through tanh
             ("I_of_ce", [{"I": lambda t, Y, q: -1.0 + 2e-4 * (Y[q.ind["c_e"].start] - 1000.0), "tf": 600.0}], 1.0, [], True),
             ("V_of_I", [{"V": lambda t, Y, q: 4.0 - 0.05 * cl.calc_I(Y, q), "tf": 300.0}], 0.5, [], True),
             ("P_tanh", [{"P": lambda t, Y, q: -29.0 * cl.tanh(2.0 * (cl.calc_V(Y, q) - 3.2)), "tf": 600.0}], 1.0, [], True),
             # closures of YP (differential states): cj d f / d YP in the integration row, the chain through the differential equation in the consistent-initialisation row
             # (scalar_residual.jl:335-362).  Without the derivative these runs stall in the oracle ("Model failed to converge"): the row enters scaled by cj = O(1/h)
             ("reads_YP", [{"I": lambda t, Y, YP, q: -1.0 + 0.02 * YP[q.ind["c_e"].start], "tf": 300.0}], 1.0, [], True),
             ("YP_and_Y", [{"I": lambda t, Y, YP, q: -1.0 + 1e-3 * YP[q.ind["c_s_avg"].start + 9] - 0.1 * (cl.calc_V(Y, q) - 4.0), "tf": 300.0}], 1.0, [], True),
             ("res_of_YP", [{"res": (-0.5, lambda t, Y, YP, q: YP[q.ind["c_e"].start + 15] + 0.5 * cl.calc_I(Y, q)), "tf": 200.0}], 0.5, [], True),
             # NONLINEAR in YP, with a Y / YP cross term: the derivative programs read YP themselves, so in the consistent initialisation they must be evaluated where the closure
             # is -- at YP = rhs(Y) -- not at the init's raw YP = 0, where 2 YP[i] = 0 would leave the row without its chain entries
             ("YP_squared", [{"I": lambda t, Y, YP, q: -1.0 + 0.5 * YP[q.ind["c_e"].start] * YP[q.ind["c_e"].start] + 1e-4 * YP[q.ind["c_e"].start + 29] * (Y[q.ind["c_e"].start] - 1000.0), "tf": 300.0}], 1.0, [], True)]
    n_der = {"taper_V": 2, "I_of_ce": 1, "V_of_I": 1, "P_tanh": 2, "reads_YP": 1, "YP_and_Y": 3, "res_of_YP": 2, "YP_squared": 3}
    for name, proto, soc, td, same in cases:
        o = pkg.Opts(); o.tdiscon = td
        ens = pkg.simulate_ensemble(p, th[None, :], proto, SOC=soc, opts=o)
        runs = parity.runs_to_oracle(O, p, pkg, proto)
        assert runs[0]["value_kind"] == 4 and len(runs[0].get("dcol", ())) == n_der.get(name, 0)
        ro = O.simulate(p.variant, th, soc, runs, opts=O.default_opts(tdiscon=td))
        assert ens.run_info[0, 0]["flag"] == ro["runs"][0]["flag"] >= 0, (name, ens.run_info[0, 0], ro["runs"][0])
        parity.compare_trajectory(ens, 0, ro, rtol_state=5e-6, same_decisions=same)
        if name == "reads_YP":
            for r in runs:
                r.pop("dcol")
            assert O.simulate(p.variant, th, soc, runs, opts=O.default_opts(tdiscon=td))["runs"][0]["flag"] < 0
        if name in ("taper_V", "V_of_I"):
            # the derivative is what the reference algorithm uses: without it (its fallback for closures it cannot differentiate) the same run takes other Newton steps --
            # 92 steps instead of 85 through the taper -- or cannot be initialised at all (V = f(I): singular control row)
            for r in runs:
                r.pop("dcol")
            r0 = O.simulate(p.variant, th, soc, runs, opts=O.default_opts(tdiscon=td))
            assert (r0["runs"][0]["flag"] < 0) if name == "V_of_I" else (r0["counters"]["n_steps"] != ro["counters"]["n_steps"])
            # with iterative refinement (the general row takes part in the residual product)
            o.refine = 1
            e1 = pkg.simulate_ensemble(p, th[None, :], proto, SOC=soc, opts=o)
            r1 = O.simulate(p.variant, th, soc, parity.runs_to_oracle(O, p, pkg, proto), opts=O.default_opts(tdiscon=td, refine=1))
            parity.compare_trajectory(e1, 0, r1, rtol_state=5e-6, same_decisions=True)
    # the exact closure and its 201-point table agree to the table's interpolation error
    tt = np.linspace(0, 10, 201)
    e1 = pkg.simulate_ensemble(p, th[None, :], [{"V": lambda t: 3.9 + 0.05 * np.cos(t), "tf": 10.0}], SOC=0.5)
    e2 = pkg.simulate_ensemble(p, th[None, :], [{"V": (tt, 3.9 + 0.05 * np.cos(tt)), "tf": 10.0}], SOC=0.5)
    assert abs(e1.run_info[0, 0]["V"] - (3.9 + 0.05 * np.cos(10.0))) < 1e-5 and abs(e1.run_info[0, 0]["I"] - e2.run_info[0, 0]["I"]) < 2e-3 * abs(e2.run_info[0, 0]["I"])
    # per-cell parameters reach the closure: two cells with different t_plus get different ramps
    Th = pkg.theta_matrix(p, 2, {"t₊": np.array([0.364, 0.182])})
    e3 = pkg.simulate_ensemble(p, Th, [{"I": lambda t, q: q.θ["t₊"] * t / 36.4, "tf": 100.0}], SOC=0.0)
    assert abs(e3.run_info[0, 0]["I"] - 1.0) < 1e-9 and abs(e3.run_info[1, 0]["I"] - 0.5) < 1e-9
    # what cannot be traced says so
    with pytest.raises(cl.TraceError, match="where"):
        pkg.make_protocol(p, [{"I": lambda t: 1.0 if t < 100 else 0.5}])
    import math
    with pytest.raises(cl.TraceError, match="numpy"):
        pkg.make_protocol(p, [{"I": lambda t: math.sin(t)}])
    with pytest.raises(ValueError):
        pkg.make_protocol(p, [{"dT": lambda t: 0.0}])


def check_closure_derivatives_other_models(p_th, p_sei, O, pkg):
    """closures of the state with the thermal model (a charge current that backs off with the temperature of the separator's middle node; a CV set-point with a
    temperature coefficient) and with SEI aging (a charge current that backs off as the film grows): the general control row through the 4x4-block thermal solve and the
    3-unknown node-local elimination of the SEI electrode, same decisions as the oracle's sparse LU of the merged pattern"""
    cl = pkg.closures
    for p, soc, protos in ((p_th, 0.2, [[{"I": lambda t, Y, q: 3.0 - 0.08 * (Y[q.ind["T"].start + 20] - 298.15), "tf": 400.0}],
                                       [{"I": lambda t, Y, YP, q: 3.0 - 20.0 * YP[q.ind["T"].start + 20], "tf": 100.0}],          # a current that backs off with the heating RATE

                                       [{"I": 2.0, "tf": 100.0}, {"V": lambda t, Y, q: 4.0 + 1e-3 * (Y[q.ind["T"].start + 20] - 298.15) - 0.02 * cl.calc_I(Y, q), "tf": 200.0}]]),
                           (p_sei, 0.1, [[{"I": lambda t, Y, q: 1.0 - 2e7 * Y[q.ind["film"].start + 3], "tf": 900.0}]])):
        th = p.theta_vector()
        for proto in protos:
            ens = pkg.simulate_ensemble(p, th[None, :], proto, SOC=soc)
            runs = parity.runs_to_oracle(O, p, pkg, proto)
            assert len(runs[-1]["dcol"]) >= 1
            ro = O.simulate(p.variant, th, soc, runs)
            assert ens.run_info[0, -1]["flag"] == ro["runs"][-1]["flag"] >= 0, (ens.run_info[0], ro["runs"])
            parity.compare_trajectory(ens, 0, ro, rtol_state=5e-6, same_decisions=True)


def check_control_row_capacity(p_th, pkg):
    """the general control row has one entry per lane (64): a closure whose row would need more -- here the rate of the mean of thirty temperature nodes, each chaining through
    the algebraic entries of its heat equation in the consistent initialisation -- is refused, not truncated"""
    T0 = p_th.ind["T"].start
    def mean_rate(t, Y, YP, q):
        s = YP[T0 + 10]
        for k in range(11, 40):
            s = s + YP[T0 + k]
        return 3.0 - s
    with pytest.raises(RuntimeError, match="64 entries"):
        pkg.simulate_ensemble(p_th, p_th.theta_vector()[None, :], [{"I": mean_rate, "tf": 10.0}], SOC=0.2)


def test_closure_derivatives_thermal_and_sei(emu_model_thermal, emu_model_sei, O, pkg):
    check_control_row_capacity(emu_model_thermal, pkg)
    check_closure_derivatives_other_models(emu_model_thermal, emu_model_sei, O, pkg)


def check_res_mode(p, p_th, O, pkg):
    """the user-defined control residual, `simulate(p, tf; res = (x, f))` (reference input_methods.jl:155-175, run_residual: x - f(t, Y, p) = 0 as the last row, always
    differentiated): "V + 0.05 I = 4" written as a residual gives the run of the V = 4 - 0.05 I closure; a residual on the temperature of one node (thermal model) and
    one that ties the current to a DIFFERENTIAL state run with the oracle's decisions; what is not built (closures of YP, i.e. also dc_s_* / dc_e_*) is refused"""
    cl = pkg.closures
    th = p.theta_vector()
    res = [{"res": (4.0, lambda t, Y, q: cl.calc_V(Y, q) + 0.05 * cl.calc_I(Y, q)), "tf": 300.0}]
    asV = [{"V": lambda t, Y, q: 4.0 - 0.05 * cl.calc_I(Y, q), "tf": 300.0}]
    e1, e2 = pkg.simulate_ensemble(p, th[None, :], res, SOC=0.5), pkg.simulate_ensemble(p, th[None, :], asV, SOC=0.5)
    assert e1.run_info[0, 0]["flag"] == e2.run_info[0, 0]["flag"] == 0 and abs(e1.run_info[0, 0]["V"] + 0.05 * e1.run_info[0, 0]["I"] - 4.0) < 1e-9
    assert parity.state_rel_err(e1.Y[0], e2.Y[0]) < 2e-5 and int(e1.counters[0]["n_steps"]) == int(e2.counters[0]["n_steps"])
    cases = [(p, 0.5, res), (p, 1.0, [{"I": -1.0, "tf": 200.0}, {"res": lambda t, Y, q: cl.calc_I(Y, q) + 1.0 - 3e-4 * (Y[q.ind["c_e"].start] - 1000.0), "tf": 400.0}])]
    if p_th is not None:
        cases.append((p_th, 0.2, [{"I": 3.0, "tf": 150.0}, {"res": (0.0, lambda t, Y, q: Y[q.ind["T"].start + 20] - 302.0 + 2.0 * cl.calc_I(Y, q)), "tf": 300.0}]))
    for pm, soc, proto in cases:
        thm = pm.theta_vector()
        ens = pkg.simulate_ensemble(pm, thm[None, :], proto, SOC=soc)
        runs = parity.runs_to_oracle(O, pm, pkg, proto)
        assert runs[-1]["mode"] == 5 and len(runs[-1]["dcol"]) >= 1
        ro = O.simulate(pm.variant, thm, soc, runs)
        assert ens.run_info[0, -1]["flag"] == ro["runs"][-1]["flag"] >= 0, (ens.run_info[0], ro["runs"])
        parity.compare_trajectory(ens, 0, ro, rtol_state=5e-6, same_decisions=True)
    with pytest.raises(ValueError, match="state"):
        pkg.make_protocol(p, [{"res": lambda t, Y, YP, q: YP[p.N.diff + 1] - 1.0}])            # YP of an algebraic state: no differential equation to chain through
    with pytest.raises(ValueError):
        pkg.make_protocol(p, [{"res": 1.0}])


def test_res_mode(emu_model, emu_model_thermal, O, pkg):
    check_res_mode(emu_model, emu_model_thermal, O, pkg)


def check_dstate_modes(models, O, pkg):
    """the rate of ONE differential state held: dc_s_p_max / dc_s_p_min / dc_s_n_max / dc_s_n_min / dc_e_max / dc_e_min (reference input_methods.jl:190-247: state_deriv_func(ind)
    as a run_residual, ind = the extreme surface / electrolyte concentration at the end of the previous run; consistent initialisation with YP[ind] replaced by the differential
    equation, scalar_residual.jl:335-362).  "Constant surface concentration" charging after a CC leg, on the isothermal, thermal, SEI and quadratic-diffusion models: the oracle's
    decisions; the chosen state really is held; refusals."""
    for p, soc, proto in models:
        th = p.theta_vector()
        ens = pkg.simulate_ensemble(p, th[None, :], proto, SOC=soc, outputs="all")
        runs = parity.runs_to_oracle(O, p, pkg, proto)
        assert runs[-1]["mode"] == 6 and runs[-1]["dstate"] >= 1
        ro = O.simulate(p.variant, th, soc, runs, keep_Y=True)
        assert ens.run_info[0, -1]["flag"] == ro["runs"][-1]["flag"] >= 0, (p.variant, ens.run_info[0], ro["runs"])
        parity.compare_trajectory(ens, 0, ro, rtol_state=5e-6, same_decisions=True)
        # the held state: its value moves at the requested rate over the last run (every saved point of it)
        name = [k for k in proto[-1] if k.startswith("dc_")][0]
        rate = 0.0 if proto[-1][name] == "hold" else float(proto[-1][name])
        n = int(ens.n_pts[0]); k = int(ens.run_info[0, -1]["iterations"])
        Yr, tr = ens.Y_all[0, n - k:n], ens.t[0, n - k:n]
        sec = p.ind["c_e"] if "c_e" in name else p.ind["c_s_avg"]
        cand = np.arange(sec.start, sec.stop)
        if "c_s" in name:
            nr = (sec.stop - sec.start) // (p.N.p + p.N.n)
            surf = cand[nr - 1::nr]
            cand = surf[:p.N.p] if "_p_" in name else surf[p.N.p:]
        ind = cand[np.argmax(Yr[0, cand])] if name.endswith("max") else cand[np.argmin(Yr[0, cand])]
        drift = Yr[:, ind] - (Yr[0, ind] + rate * (tr - tr[0]))
        assert np.abs(drift).max() <= 2e-3 * max(1.0, abs(rate) * (tr[-1] - tr[0])) + 1e-6 * abs(Yr[0, ind]), (p.variant, name, np.abs(drift).max())
    p = models[0][0]
    with pytest.raises(RuntimeError, match="first run"):
        pkg.simulate_ensemble(p, p.theta_vector()[None, :], [{"dc_s_n_max": 0.0, "tf": 10.0}], SOC=0.5)
    with pytest.raises(ValueError):
        pkg.make_protocol(p, [{"I": 1.0, "tf": 10.0}, {"dc_e_min": lambda t: 0.0}])


def dstate_cases(p, p_th, p_sei, p_quad):
    return [(p, 0.2, [{"I": 2.0, "tf": 300.0}, {"dc_s_n_max": 0.0, "tf": 300.0}]),
            (p, 1.0, [{"I": -1.0, "tf": 600.0}, {"dc_e_max": "hold", "tf": 200.0}]),
            (p, 0.2, [{"I": 2.0, "tf": 200.0}, {"dc_s_p_min": -0.5, "tf": 100.0}]),
            (p_th, 0.2, [{"I": 3.0, "tf": 150.0}, {"dc_s_n_max": "hold", "tf": 200.0}]),
            (p_sei, 0.1, [{"I": 1.0, "tf": 300.0}, {"dc_e_min": 0.0, "tf": 200.0}]),
            (p_quad, 1.0, [{"I": -1.0, "tf": 300.0}, {"dc_s_p_max": 0.5, "tf": 100.0}, {"dc_s_n_min": "hold", "tf": 100.0}])]


def test_dstate_modes(emu_model, emu_model_thermal, emu_model_sei, emu_models_f4, O, pkg):
    check_dstate_modes(dstate_cases(emu_model, emu_model_thermal, emu_model_sei, emu_models_f4["quad"]), O, pkg)


def test_function_inputs(emu_model, O, pkg):
    check_function_inputs(emu_model, O, pkg)


def check_outputs_all(p, O, pkg, proto, soc):
    """outputs = :all (reference solution_states_logic, src/outputs.jl:107-131; set_vars!, src/save_outputs.jl:11-40): every saved state vector
    comes back as Y_all[cell, point, state] with the named sections of p.ind, plus T_avg per point when temperature = true."""
    th = p.theta_vector()
    ens = pkg.simulate_ensemble(p, np.tile(th, (2, 1)), proto, SOC=soc, outputs="all")
    ref = pkg.simulate_ensemble(p, np.tile(th, (2, 1)), proto, SOC=soc)
    n = int(ens.n_pts[0])
    assert ref.Y_all is None and np.array_equal(ref.t[:, :n], ens.t[:, :n]) and np.array_equal(ref.Y, ens.Y)       # asking for the states changes nothing else
    ro = O.simulate(p.variant, th, soc, parity.runs_to_oracle(O, p, pkg, proto), keep_Y=True)
    parity.compare_trajectory(ens, 0, ro, rtol_state=1e-6)
    assert n == len(ro["t"]) and ens.Y_all.shape == (2, ens.t.shape[1], p.N.tot)
    assert np.array_equal(ens.Y_all[0, n - 1], ens.Y[0]) and np.array_equal(ens.Y_all[0, :n], ens.Y_all[1, :n])
    for name, sl in p.ind.items():
        a, b = ens.Y_all[0, :n, sl], ro["Y_all"][:, sl]
        floor = {"j_s": 1e-13, "film": 1e-14}.get(name, 1e-300)
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max() + floor, name                              # 1e-6 relative per section, every step
    s = ens[0]
    assert np.array_equal(s.Φ_s[:, 0] - s.Φ_s[:, -1], s.V) and np.array_equal(s.I, s.Y_all[:, p.ind["I"]][:, 0]) and s.c_e.shape == (n, 30)
    if p.temperature:
        assert np.abs(ens.T_avg[0, :n] - ro["T"]).max() < 1e-6 * 300 and s.T.shape == (n, 50)
    else:
        assert ens.T_avg is None
        with pytest.raises(AttributeError):
            s.T
    # the single-cell API: outputs keyword, continuation keeps the states, sol(t) interpolates them
    sol = pkg.simulate(p, proto[0].get("tf", 1e6), SOC=soc, outputs="all", **{k: v for k, v in proto[0].items() if k != "tf"})
    assert np.array_equal(sol.Y_all, ens.Y_all[0, :len(sol.t)][:len(sol.t)]) or len(proto) > 1
    mid = sol(0.5 * (sol.t[1] + sol.t[2]))
    assert mid.Y_all.shape == (1, p.N.tot) and abs((mid.Φ_s[0, 0] - mid.Φ_s[0, -1]) - mid.V[0]) < 1e-9


def test_outputs_all_states_per_step(emu_model, O, pkg):
    check_outputs_all(emu_model, O, pkg, [{"I": -1.0, "tf": 400.0}], 1.0)


def test_outputs_all_thermal(emu_model_thermal, O, pkg):
    check_outputs_all(emu_model_thermal, O, pkg, [{"I": 3.0, "tf": 150.0}], 0.1)


def check_per_cell_protocol(p, O, pkg, n=6):
    """per-cell input values and run lengths (plh_run.value_cell / tf_cell): a C-rate sweep followed by rests of different lengths, every cell
    against the oracle run with that cell's values at 1e-6 (same step decisions)"""
    th = p.theta_vector()
    rates = -np.linspace(0.5, 3.0, n)
    rests = np.linspace(30.0, 300.0, n)
    proto = [{"I": rates, "tf": 600.0}, {"I": "rest", "tf": rests}]
    ens = pkg.simulate_ensemble(p, np.tile(th, (n, 1)), proto, SOC=1.0)
    for i in range(n):
        ro = O.simulate(p.variant, th, 1.0, parity.runs_to_oracle(O, p, pkg, proto, cell=i, n_cells=n))
        parity.compare_trajectory(ens, i, ro, rtol_state=1e-6)
        assert abs(ens.run_info[i, 0]["I"] - rates[i]) < 1e-12 and abs(ens.run_info[i, 1]["t_end"] - ens.run_info[i, 0]["t_end"] - rests[i]) < 1e-6
    with pytest.raises(ValueError):
        pkg.simulate_ensemble(p, np.tile(th, (n, 1)), [{"I": rates[:-1]}], SOC=1.0)
    with pytest.raises(pkg._capi.PetlionHipError):
        pkg.simulate_ensemble(p, np.tile(th, (n, 1)), [{"I": -1.0, "tf": np.zeros(n)}], SOC=1.0)


def test_per_cell_protocol_values(emu_model, O, pkg):
    check_per_cell_protocol(emu_model, O, pkg, n=4)


def check_user_tstops(p, O, pkg, soc=1.0, proto=None, rtol_state=1e-6, same_decisions=True):
    """opts.tstops (reference src/model_evaluation.jl:292-294: appended to the integrator's tstops, run-local times): the integrator hits every stop exactly -- a saved
    point lands on each one inside the run -- and the trajectory keeps the oracle's decisions (same step / Newton counters, states at 1e-6)"""
    proto = proto or [{"I": -1.0, "tf": 900.0}, {"I": "rest", "tf": 300.0}]
    stops = [400.0, 37.25, 250.5, 250.5, 899.0, 1200.0, -3.0, 0.0]          # unsorted, duplicated, one beyond tf of either run, non-positive ones (dropped like the reference does)
    # (init_step pinned in both: a stop clips the step before it to tstop - t_n, which turns the 1e-6 relative h0 noise of the step grid, DESIGN.md 5, into 1e-3 of that step)
    o = pkg.Opts(); o.tstops = stops; o.init_step = 1e-3
    ens = pkg.simulate_ensemble(p, pkg.theta_matrix(p, 2), proto, SOC=soc, opts=o)
    ro = O.simulate(p.variant, p.theta_vector(), soc, parity.runs_to_oracle(O, p, pkg, proto), opts=O.default_opts(tstops=stops, init_step=1e-3))
    parity.compare_trajectory(ens, 1, ro, rtol_state=rtol_state, same_decisions=same_decisions)
    n = int(ens.n_pts[0]); t = ens.t[0, :n]
    k1 = int(ens.run_info[0, 0]["iterations"])
    for st in (37.25, 250.5, 400.0, 899.0):
        assert (t[:k1] == st).sum() == 1, st                                   # exactly, once, in run 1
    loc2 = t[k1:] - t[k1]
    for st in (37.25, 250.5):
        assert np.abs(loc2 - st).min() < 1e-9 * 900.0, st                     # run 2 (local time restarts at nextfloat(t_end)): 37.25 and 250.5 again; 400 is beyond its tf
    assert np.abs(loc2 - 400.0).min() > 1.0
    plain = pkg.simulate_ensemble(p, pkg.theta_matrix(p, 1), proto, SOC=soc)
    assert parity.state_rel_err(plain.Y[0], ens.Y[0]) < 2e-2 and int(plain.n_pts[0]) < n     # the stops cost steps, the solution stays within the integration tolerance


def test_user_tstops(emu_model, O, pkg):
    check_user_tstops(emu_model, O, pkg)


def check_notebook_step_history_device(p, pkg):
    """the printed step history of examples/model_inputs_and_outputs.ipynb (SUNDIALS IDA + KLU output: 121 points, sol.V[1:13], sol.c_e[1:5]) through the host API and
    the device integrator with opts.yp_alg_zero (tests/test_oracle_golden.py::check_notebook_step_history has the story)"""
    import test_oracle_golden as tg

    def sim(z):
        sol = pkg.simulate(p, I=2, SOC=0, V_max=4.1, outputs=("t", "V", "c_e"), yp_alg_zero=z)
        pkg.simulate_b(sol, p, V="hold", outputs=("t", "V", "c_e"), yp_alg_zero=z)
        runs = [dict(flag=r.flag, iterations=r.iterations, t_end=float(r.info["t_end"]), I=float(r.info["I"]), SOC=float(r.info["SOC"])) for r in sol.results]
        return dict(t=sol.t, V=sol.V, c_e=sol.c_e, runs=runs)
    tg.check_notebook_step_history(sim, exact_hold_leg=False)


def test_notebook_step_history_on_the_device_source(emu_model, pkg):
    check_notebook_step_history_device(emu_model, pkg)


def test_emulator_hostile_modes():
    """The same device-source tests with the emulator's LDS block and lane stacks starting as garbage (PL_EMU_POISON: on the GPU LDS holds what the
    previous workgroup left) and the lanes run 63..0 between sync points (PL_EMU_ORDER=reverse: a cross-lane LDS hand-over that lacks a sync point --
    on the GPU only a compiler barrier keeps the load below the store -- reads stale data in one of the two orders).  The environment is read once
    per process, hence the subprocess."""
    import subprocess, sys
    env = dict(os.environ, PL_EMU_POISON="1", PL_EMU_ORDER="reverse")
    sel = "cc_discharge_trajectory or lco_sei_aging or outputs_all_thermal or power_and_plating"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def check_two_waves(pkg, O):
    import build_emu
    p = pkg.petlion(pkg.LCO, waves_per_cell=2, _lib_path=build_emu.build())
    parity.check_keys_and_pattern(p, O)
    parity.check_evaluators(p, O, n_cells=2)
    parity.check_init(p, O)
    Th = pkg.theta_matrix(p, 2, {"D_sp": np.array([1.0, 0.6]) * p.θ["D_sp"]})
    ens = pkg.simulate_ensemble(p, Th, [{"I": -1.0}], SOC=1.0)
    for i in range(2):
        parity.compare_trajectory(ens, i, O.simulate("lco_iso", Th[i], 1.0, parity.runs_to_oracle(O, p, pkg, [{"I": -1.0}])), rtol_state=1e-6)
    # a closure of the state with derivative programs: the general control row reads across the two waves (also under the hostile schedules below)
    cl = pkg.closures
    taper = [{"I": lambda t, Y, q: -cl.minimum(1.0, cl.maximum(0.05, (cl.calc_V(Y, q) - 3.0) * 2.0)), "tf": 4000.0, "V_min": 3.05}]
    ens = pkg.simulate_ensemble(p, Th[:1], taper, SOC=1.0)
    parity.compare_trajectory(ens, 0, O.simulate("lco_iso", Th[0], 1.0, parity.runs_to_oracle(O, p, pkg, taper)), rtol_state=5e-6)


def test_two_waves_per_cell_variant(pkg, O):
    """waves_per_cell = 2 (a 128-thread workgroup per cell, wave 1 owns the particle rows): same evaluators, initialisation and trajectory as the oracle"""
    check_two_waves(pkg, O)


@pytest.mark.parametrize("wave", ["0", "1"])
def test_two_waves_per_cell_hostile_schedules(wave):
    """the two-wave variant with one wave always run as far ahead of the other as the workgroup barriers allow (PL_EMU_WAVE: a cross-wave LDS hand-over that lacks a
    barrier reads stale data under one of the two preferences), lanes in reverse order, LDS and stacks poisoned"""
    import subprocess, sys
    env = dict(os.environ, PL_EMU_POISON="1", PL_EMU_ORDER="reverse", PL_EMU_WAVE=wave)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-k", "two_waves_per_cell_variant", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def check_f4_variant(p, O, pkg, tag, n_traj=2, rtol_state=2e-5):
    """one SURVEY 8(f).4 model variant: key order and CSC pattern identical to the oracle's symbolic pipeline, residual 1e-12 / Jacobian 1e-9 / solve 1e-8,
    consistent initialisation, and 1C discharges with identical solver decisions (final state within the reproducibility floor discussed in test_gpu_parity.py)"""
    parity.check_keys_and_pattern(p, O)
    if tag == "mhc":                                        # the reference default lambda = 6.26e-20 saturates the erf: also exercise a dimensionless lambda where it matters
        p.θ["λ_MHC_p"], p.θ["λ_MHC_n"] = 8.0, 6.0
    parity.check_evaluators(p, O, n_cells=3)
    parity.check_init(p, O, None)
    Th = pkg.theta_matrix(p, n_traj, {"D_sp": np.linspace(1.0, 0.7, n_traj) * p.θ["D_sp"]})
    ens = pkg.simulate_ensemble(p, Th, [{"I": -1.0}], SOC=1.0)
    for i in range(n_traj):
        ro = O.simulate(p.variant, Th[i], 1.0, parity.runs_to_oracle(O, p, pkg, [{"I": -1.0}]))
        parity.compare_trajectory(ens, i, ro, rtol_state=rtol_state)
    return ens


def test_f4_quadratic_and_polynomial_solid_diffusion(emu_models_f4, O, pkg):
    """residuals_c_s_avg! / residuals_Q! / build_c_s_star! of the quadratic and polynomial approximations (residuals.jl:108-127, 237-258; aux...jl:212-248)"""
    eq = check_f4_variant(emu_models_f4["quad"], O, pkg, "quad")
    ep = check_f4_variant(emu_models_f4["poly"], O, pkg, "poly")
    assert emu_models_f4["quad"].N.tot == 121 and emu_models_f4["poly"].N.tot == 141 and "Q" in emu_models_f4["poly"].ind
    assert eq.run_info[0, 0]["flag"] == 3 and ep.run_info[0, 0]["flag"] == 1          # the polynomial surface concentration reaches the knee earlier: V_min


def test_f4_nonlinear_thermodynamic_factor(emu_models_f4, O, pkg):
    """thermodynamic_factor(c_e, T) (custom_functions.jl:191-203) in the c_e source and, with the row's own nu_i on both edges, in the Phi_e rows (residuals.jl:95-98, 626-645)"""
    check_f4_variant(emu_models_f4["nu"], O, pkg, "nu")


def test_f4_mhc_kinetics(emu_models_f4, O, pkg):
    """rxn_MHC (custom_functions.jl:241-298): evaluators at lambda = 8 / 6 (the erf matters) and trajectories"""
    check_f4_variant(emu_models_f4["mhc"], O, pkg, "mhc")


def test_f4_lgm50_chemistry(emu_models_f4, O, pkg):
    """NMC_LGM50 + LiC6_LGM50 (Chen et al. 2020, reference src/params.jl:514-849): tanh OCVs, D_eff(c_e) and K_eff(c_e) closures, 33 parameters"""
    p = emu_models_f4["lgm50"]
    assert "D_e" in p.θ_keys and "D_p" not in p.θ_keys and len(p.θ_keys) == 33
    ens = check_f4_variant(p, O, pkg, "lgm50")
    assert ens.run_info[0, 0]["flag"] == 1 and 3500.0 < ens.run_info[0, 0]["t_end"] < 3600.0          # a 1C discharge ends on V_min = 2.5 V shortly before 1 h


# ---- other discretisations (reference src/params.jl:119-136): the kernels of another grid are one more build of the same device source -------------------------
def emu_grid_model(pkg, cathode, grid, variant_id, **kw):
    """grid = (N_p, N_s, N_n, N_r) or, with temperature = true, (N_p, N_s, N_n, N_r, N_a, N_z)"""
    import build_emu
    g = tuple(grid) + (10, 10) if len(grid) == 4 else tuple(grid)       # (a 7th entry: N_r_n != N_r_p)
    return pkg.petlion(cathode, N_p=g[0], N_s=g[1], N_n=g[2], N_r_p=g[3], N_r_n=g[6] if len(g) == 7 else g[3], N_a=g[4], N_z=g[5], _lib_path=build_emu.build(),
                       _grid_lib=build_emu.build_grid(g, [variant_id]), **kw)


def check_grid_model(p, O, pkg, identical=True, solve_tol=1e-8):
    """a model on another grid against the oracle variant generated for that grid (oracle/codegen.py): theta keys and CSC pattern, residual 1e-12 / Jacobian 1e-9 /
    solve 1e-8, consistent initialisation, two 1C discharges"""
    parity.check_keys_and_pattern(p, O)
    parity.check_evaluators(p, O, n_cells=2, solve_tol=solve_tol)
    parity.check_init(p, O, None)
    Th = pkg.theta_matrix(p, 2, {"D_sp": np.array([1.0, 0.6]) * p.θ["D_sp"]})
    ens = pkg.simulate_ensemble(p, Th, [{"I": -1.0}], SOC=1.0)
    for i in range(2):
        ro = O.simulate(p.variant, Th[i], 1.0, parity.runs_to_oracle(O, p, pkg, [{"I": -1.0}]))
        if identical:
            parity.compare_trajectory(ens, i, ro, rtol_state=1e-6)
        else:   # a discharge that ends on the voltage knee: the stop time is reproducible to the floor discussed in test_gpu_parity.py, one Newton iteration may differ
            assert ens.run_info[i, 0]["flag"] == ro["runs"][0]["flag"] and int(ens.counters[i]["n_steps"]) == ro["counters"]["n_steps"]
            assert abs(int(ens.counters[i]["n_newton"]) - ro["counters"]["n_newton"]) <= 2
            assert abs(ens.run_info[i, 0]["t_end"] - ro["runs"][0]["t_end"]) < 1e-7 * ro["runs"][0]["t_end"] and parity.state_rel_err(ens.Y[i], ro["Y"]) < 2e-6


def test_other_discretisation_lco_12_7_9_11(pkg, O):
    """N_p = 12, N_s = 7, N_n = 9, N_r = 11 (330 states): unequal sections, N_r != 10, six trips per lane"""
    check_grid_model(emu_grid_model(pkg, pkg.LCO, (12, 7, 9, 11), 0), O, pkg)


def check_thermal_grid_model(p, O, pkg, solve_tol=1e-8):
    """temperature = true on another grid (N_p != N_n, N_a != N_z, N_r != 10) against the oracle variant generated for it: pattern, evaluators in every mode incl. dT,
    consistent initialisation, a 1C discharge with identical decisions, and the CC-CT-CV protocol (CC leg at 1e-6, hold legs at the default-tolerance floor)"""
    check_grid_model(p, O, pkg, solve_tol=solve_tol)
    ens = pkg.simulate_ensemble(p, pkg.theta_matrix(p, 1), CC_CT_CV, SOC=0.0)
    ro = O.simulate(p.variant, p.theta_vector(), 0.0, parity.runs_to_oracle(O, p, pkg, CC_CT_CV))
    fl = [int(f) for f in ens.run_info[0]["flag"]]
    assert fl == [r["flag"] for r in ro["runs"]] == [5, 2, 4]
    assert int(ens.run_info[0, 0]["iterations"]) == ro["runs"][0]["iterations"] and abs(ens.run_info[0, 0]["t_end"] - ro["runs"][0]["t_end"]) < 1e-6 * ro["runs"][0]["t_end"]
    for k in (1, 2):
        assert abs(ens.run_info[0, k]["t_end"] - ro["runs"][k]["t_end"]) < (2e-3, 1e-2)[k - 1] * ro["runs"][k]["t_end"], k


def test_other_discretisation_thermal_8_6_7_11_5_7(pkg, O):
    """LCO with temperature = true on N_p = 8, N_s = 6, N_n = 7, N_r = 11, N_a = 5, N_z = 7 (271 states): the two far-behind T rows become final at different stages of their
    chains, the collector chains have different lengths, five particles per pass"""
    check_thermal_grid_model(emu_grid_model(pkg, pkg.LCO, (8, 6, 7, 11, 5, 7), 4, temperature=True), O, pkg)


@pytest.mark.parametrize("grid", [(5, 9, 5, 10, 2, 3), (9, 4, 6, 12, 12, 4), (12, 8, 12, 10, 10, 10)])
def test_thermal_extreme_discretisations(pkg, grid):
    """temperature = true at the limits of what the elimination takes (five nodes per electrode, an electrode filling its half of the sweeps, two-node collectors, an odd
    number of nodes): evaluators self-consistent and equal to the oracle's Python restatement in the I, V and dT modes, and the CC-CT-CV protocol runs through"""
    from oracle import dfn_model as dm
    p = emu_grid_model(pkg, pkg.LCO, grid, 4, temperature=True)
    check_grid_self_consistency(p, pkg, dm)
    ens = pkg.simulate_ensemble(p, pkg.theta_matrix(p, 1), CC_CT_CV, SOC=0.0)
    assert [int(f) for f in ens.run_info[0]["flag"]] == [5, 2, 4] and abs(ens.run_info[0, 1]["T_avg"] - 313.15) < 1e-3


def test_other_discretisation_nmc_sei_6_5_8_13(pkg, O):
    """NMC + SEI on N_p = 6, N_s = 5, N_n = 8, N_r = 13 (266 states): an odd number of nodes (the two halves of the twisted sweeps differ by one), four particles per pass"""
    check_grid_model(emu_grid_model(pkg, pkg.NMC, (6, 5, 8, 13), 3, aging="SEI"), O, pkg, identical=False)


# ---- N_r_p != N_r_n (reference src/params.jl:124-136: the two particle grids are independent options) ----------------------------------------------------------------
def test_unequal_particle_grids_lco_7_6_8_12_rn10(pkg, O):
    """N_r_p = 12, N_r_n = 10 on N_p = 7, N_s = 6, N_n = 8 (237 states; five particles per pass on the lane stride 12, the anode's operator zero-padded): theta keys, CSC
    pattern, evaluators, consistent initialisation and two 1C discharges against the oracle variant generated for this grid"""
    check_grid_model(emu_grid_model(pkg, pkg.LCO, (7, 6, 8, 12, 10, 10, 10), 0), O, pkg)


def test_unequal_particle_grids_thermal_8_6_7_11_5_7_rn13(pkg, O):
    """temperature = true with N_r_p = 11 < N_r_n = 13 (the cathode's operator is the padded one): per-particle spectral resolvents from per-electrode tables, the CC-CT-CV protocol"""
    # (solve: 5e-8 instead of 1e-8 -- thirteen radial nodes raise the stiffest particle mode and with it the condition number (2e16 for these matrices); the structured solve and the
    #  oracle's LU differ by 1.7e-8 in the I entry of the eta_plating system and are BOTH 4.7e-8 from a dense LAPACK solve of the same matrix)
    check_thermal_grid_model(emu_grid_model(pkg, pkg.LCO, (8, 6, 7, 11, 5, 7, 13), 4, temperature=True), O, pkg, solve_tol=5e-8)


@pytest.mark.parametrize("grid,vid,kw", [((7, 6, 8, 10, 10, 10, 13), 0, {}), ((6, 5, 8, 11, 10, 10, 14), 2, dict(aging="SEI")), ((8, 6, 7, 14, 5, 7, 10), 4, dict(temperature=True)),
                                         ((5, 3, 20, 16, 10, 10, 10), 0, {})])
def test_unequal_particle_grids_self_consistency(pkg, grid, vid, kw):
    """both orders of N_r_p / N_r_n, with SEI aging, with temperature, and the largest stride against the smallest grid: the device residual against the oracle's Python
    restatement, the Jacobian against differences of the residual, the solve against a dense solve; a 600 s 1C discharge lands on the default grid's voltage"""
    from oracle import dfn_model as dm
    p = emu_grid_model(pkg, pkg.LCO, grid, vid, **kw)
    assert p.ind["c_s_avg"].stop - p.ind["c_s_avg"].start == grid[0] * grid[3] + grid[2] * grid[6]
    check_grid_self_consistency(p, pkg, dm)
    ens = pkg.simulate_ensemble(p, pkg.theta_matrix(p, 1), [{"I": -1.0, "tf": 600.0}], SOC=1.0)
    assert ens.run_info[0, 0]["flag"] == 0 and abs(ens.run_info[0, 0]["t_end"] - 600.0) < 1e-9
    assert abs(ens.run_info[0, 0]["V"] - (3.94638 if kw.get("temperature") else (3.94023 if kw.get("aging") else 3.945410))) < 2e-3, ens.run_info[0, 0]["V"]


def check_grid_self_consistency(p, pkg, dm, n_fd=6):
    """grids without a generated oracle variant: the device residual against the oracle's PYTHON restatement evaluated directly (oracle/dfn_model.py, FloatOps), the
    device Jacobian against central differences of the device residual, the device solve against a dense solve of the device Jacobian"""
    lib, h, N = p._lib, p._h, p.N.tot
    model = dm.Model(cathode={"LCO": "LCO", "NMC": "NMC", "NMC_LGM50": "LGM50"}.get(p.cathode, p.cathode), aging=bool(p.aging), temperature=p.temperature, Np=p.N.p, Ns=p.N.s, Nn=p.N.n, Nrp=p.N.r_p, Nrn=p.N.r_n, **(dict(Na=p.N.a, Nz=p.N.z) if p.temperature else {}))
    assert model.lay.N == N
    th = p.theta_vector()[None, :].copy()
    thd = dict(model.theta); thd.update(dict(zip(p.θ_keys, th[0])))
    rng = np.random.default_rng(5)
    Y = np.array([dm.initial_guess(model, 0.6, thd)]); Y[0, -1] = -1.0
    Yd = np.zeros((1, N)); soc = np.array([0.6])
    assert lib.plh_initial_guess(h, 1, th.ctypes.data, soc.ctypes.data, Yd.ctypes.data, 0, None) == 0
    assert np.allclose(Yd[0, :-1], Y[0, :-1], rtol=1e-13, atol=0)
    Y *= 1 + 1e-3 * rng.standard_normal(Y.shape); YP = 1e-4 * np.abs(Y) * rng.standard_normal(Y.shape)
    if p.temperature:                                           # a temperature profile with gradients, so that every conduction / heat-source term is exercised
        Y[0, p.ind["T"]] += 3.0 * np.sin(np.linspace(0.0, 3.0, p.ind["T"].stop - p.ind["T"].start))
    for mode, val in ((0, -1.0), (1, 3.9)) + (((2, 0.01),) if p.temperature else ()):
        def F_of(y):
            F = np.zeros((1, N)); y = np.ascontiguousarray(y)
            assert lib.plh_residual(h, 1, th.ctypes.data, y.ctypes.data, YP.ctypes.data, mode, val, F.ctypes.data, 0, None) == 0
            return F[0]
        F = F_of(Y)
        Fo = np.array([float(v) for v in dm.residual(model, dm.FloatOps(), list(Y[0]), list(YP[0]), thd, mode=mode, value=val)])
        cp, ri = p.jac_pattern(mode)
        def J_at(cj):
            nz = np.zeros((1, len(ri)))
            assert lib.plh_jacobian(h, 1, th.ctypes.data, Y.ctypes.data, YP.ctypes.data, cj, mode, nz.ctypes.data, 0, None) == 0
            A = np.zeros((N, N))
            for c in range(N):
                A[ri[cp[c]:cp[c + 1]], c] = nz[0, cp[c]:cp[c + 1]]
            return A
        J0, cj = J_at(0.0), 0.37
        A = J_at(cj)
        term = np.abs(J0) @ np.abs(Y[0]) + np.abs(A - J0) @ np.abs(YP[0]) / cj + abs(val) * (np.arange(N) == N - 1)
        assert (np.abs(F - Fo) <= 1e-11 * term + 1e-300).all(), (mode, np.flatnonzero(np.abs(F - Fo) > 1e-11 * term)[:6])
        for _ in range(n_fd):                                   # J(cj = 0) v against the directional central difference of the residual
            v = rng.standard_normal(N) * np.abs(Y[0]); eps = 1e-6
            fd = (F_of(Y + eps * v) - F_of(Y - eps * v)) / (2 * eps)
            assert (np.abs(J0 @ v - fd) <= 1e-6 * (np.abs(J0) @ np.abs(v)) + 1e-300).all(), mode
        b = rng.standard_normal((1, N)); x = b.copy()
        assert lib.plh_linear_solve(h, 1, th.ctypes.data, Y.ctypes.data, YP.ctypes.data, cj, mode, x.ctypes.data, 0, None) == 0
        xo = np.linalg.solve(A, b[0])
        for name, sl in p.ind.items():
            assert np.abs(x[0, sl] - xo[sl]).max() <= 1e-7 * np.abs(xo[sl]).max() + 1e-300, (mode, name)


@pytest.mark.parametrize("grid", [(2, 2, 2, 10), (16, 16, 16, 16), (5, 3, 20, 12)])
def test_extreme_discretisations(pkg, grid):
    """the smallest and the largest supported grids, and a lopsided one: evaluators self-consistent and equal to the oracle's Python restatement, and a 1C discharge that
    reproduces the default grid's cell voltage to the discretisation error"""
    from oracle import dfn_model as dm
    p = emu_grid_model(pkg, pkg.LCO, grid, 0)
    check_grid_self_consistency(p, pkg, dm)
    ens = pkg.simulate_ensemble(p, pkg.theta_matrix(p, 1), [{"I": -1.0, "tf": 600.0}], SOC=1.0)
    assert ens.run_info[0, 0]["flag"] == 0 and abs(ens.run_info[0, 0]["t_end"] - 600.0) < 1e-9
    # default grid: 3.945410 V after 600 s at 1C; 16/16/16/16: 3.945626; 5/3/20/12: 3.944614; two nodes per section: 3.935740 (10 mV of discretisation error)
    assert abs(ens.run_info[0, 0]["V"] - 3.945410) < (1.5e-2 if min(grid[:3]) < 3 else 2e-3), ens.run_info[0, 0]["V"]


def test_unsupported_discretisations_refuse(pkg, emu_model):
    for kw in (dict(N_p=40, N_s=10, N_n=10), dict(N_r_p=9, N_r_n=9), dict(N_r_p=12, N_r_n=9), dict(N_r_p=10, N_r_n=17), dict(N_p=1), dict(temperature=True, N_p=4), dict(temperature=True, N_p=20, N_s=4, N_n=6),
               dict(temperature=True, N_a=20, N_z=20)):
        with pytest.raises((ValueError, NotImplementedError)):
            pkg.petlion(pkg.LCO, **kw)
    with pytest.raises(pkg._capi.PetlionHipError, match="plh_register_grid_library"):       # the C ABI itself: an unregistered grid is refused with the way out in the message
        pkg.petlion(pkg.LCO, N_p=11, _lib_path=emu_model._lib._name, _grid_lib=False)


# ---- r05 ----
def test_default_build_is_the_quiet_oracle_through_hold_legs(emu_model, O, pkg):
    """identical decisions and 1e-9 per cell against lco_iso_quiet, default tolerances, CC-CV / five-leg hold chain / 1C discharge (parity.check_quiet_oracle_parity)"""
    w = parity.check_quiet_oracle_parity(emu_model, O, pkg, n_cells=2, tol=1e-9, min_same=1.0)
    print("device vs quiet oracle, worst deviation over cells / protocols: %.1e" % w)


def test_default_build_is_the_quiet_oracle_thermal_cc_ct_cv(emu_model_thermal, O, pkg):
    w = parity.check_quiet_oracle_parity(emu_model_thermal, O, pkg, n_cells=2, thermal_proto=True, tol=1e-5, min_same=1.0)      # (C3's legs end on bounds: the linear back-interpolation over a knee amplifies last-bit differences; the fixed-time chain: 1e-8)
    print("thermal device vs quiet oracle, worst deviation: %.1e" % w)


@pytest.fixture(scope="module")
def emu_models_reforder(pkg):
    import build_emu
    lib = build_emu.build()
    return pkg.petlion(pkg.LCO, precision="f64_reforder", _lib_path=lib), pkg.petlion(pkg.LCO, temperature=True, precision="f64_reforder", _lib_path=lib)


def test_reference_order_variants(emu_models_reforder, O, pkg):
    """PLH_PREC_F64_REFORDER: the finite-volume rows in the generated code's operation order (matrix form, source term first)"""
    parity.check_reforder_variant(emu_models_reforder[0], O, pkg, "lco_iso")
    parity.check_reforder_variant(emu_models_reforder[1], O, pkg, "lco_thermal")


def test_reference_order_variant_follows_the_notebook_pinned_oracle_in_a_hold_leg(emu_model, emu_models_reforder, O, pkg):
    """The A/B of DESIGN.md 5 on a handful of cells (the GPU suite runs it on 256): CC 900 s -> V hold 600 s.  The default build keeps the QUIET oracle's decisions in every
    cell; the reference-order build's error against the tight solution is distributed like the plain (notebook-pinned) oracle's, whose decisions it keeps far more often
    than the default build does."""
    proto = [dict(I=2.0, tf=900.0, V_max=5.0), dict(V="hold", tf=600.0, V_max=5.0, I_min=0.0)]
    n = 8
    p0, pr = emu_model, emu_models_reforder[0]
    Th = np.ascontiguousarray(pkg.configs.sweep_theta(p0, np.arange(n), 4))
    runs = parity.runs_to_oracle(O, p0, pkg, proto)
    e0, er = pkg.simulate_ensemble(p0, Th, proto, SOC=0.0), pkg.simulate_ensemble(pr, Th, proto, SOC=0.0)
    CNT = ("n_steps", "n_res", "n_jac", "n_newton", "n_errfail", "n_convfail")
    same_q = same_r = same_0 = 0
    ratio_r = []
    for i in range(n):
        ro, rq = O.simulate("lco_iso", Th[i], 0.0, runs), O.simulate("lco_iso_quiet", Th[i], 0.0, runs)
        rt = O.simulate("lco_iso", Th[i], 0.0, runs, opts=O.default_opts(maxiters=1000000, **parity.TIGHT), max_out=200000)
        same_q += all(int(e0.counters[i][f]) == rq["counters"][f] for f in CNT)
        same_0 += int(e0.counters[i]["n_steps"]) == ro["counters"]["n_steps"]
        same_r += int(er.counters[i]["n_steps"]) == ro["counters"]["n_steps"]
        ratio_r.append(parity.state_rel_err(er.Y[i], rt["Y"]) / parity.state_rel_err(ro["Y"], rt["Y"]))
        assert parity.state_rel_err(e0.Y[i], rq["Y"]) <= 1e-9
    print("default build: quiet oracle's decisions in %d / %d cells, plain oracle's step count in %d; reference-order build: plain oracle's step count in %d, error ratio median %.3f"
          % (same_q, n, same_0, same_r, float(np.median(ratio_r))))
    assert same_q == n and same_r >= same_0 and 0.8 <= float(np.median(ratio_r)) <= 1.25


def test_stop_function(emu_model, O, pkg):
    parity.check_stop_function(emu_model, O, pkg)


def test_stop_function_thermal_node_temperature(emu_model_thermal, O, pkg):
    parity.check_stop_function(emu_model_thermal, O, pkg)


def test_default_layout_lds_bytes(emu_model):
    """LDS per cell of variant 0 on the default grid (since r06: state vectors padded to whole trips, 301 -> 320 entries, + the node-pass tables): four cells per CU need <= 40 960"""
    assert emu_model.lds_bytes == 39264


def test_initial_states(emu_model, O, pkg):
    parity.check_initial_states(emu_model, O, pkg)


def test_save_start(emu_model, pkg):
    parity.check_save_start(emu_model, pkg)

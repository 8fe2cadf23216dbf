"""The step boundary of the plain integrate kernel (csrc/dfn_integrate.h, PL_STEPB): the accepted point handed to the run logic out of ida_complete_step's registers, the
error weights formed where phi[0] is stored, no iterate after the last Newton correction -- against the separate passes it replaces, which stay compilable under
-DPL_OLD_STEP_BOUNDARY for exactly this comparison.  Both are wave-emulator builds of variant 0 (lco_iso); every output must be bit-equal on protocols that leave the
normal path each in its own way, and every case asserts from flags and counters that at least one cell did leave it that way."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CELLS = 4
ERR_OUTPUT_FULL = -14
ERR_STALL = -12

# name -> (protocol, SOC, options, max_points)
CASES = {
    "bound": ([{"I": -1.0}], 1.0, {}, None),                                                       # 1C discharge to SOC_min: back-interpolation from phi[0] - phi[1]
    "tf_inside_step": ([{"I": -1.0, "tf": 1000.0}], 1.0, {}, None),                                # the last step is clamped to tf: at_tstop, ida_get_solution
    "continuation": ([{"I": -1.0, "tf": 600.0}, {"I": "rest", "tf": 600.0}], 1.0, {}, None),      # second run: re-initialisation, the tstop 1 s after its start
    "default_h0": ([{"I": -1.0, "tf": 300.0}], 1.0, {}, None),                                     # (what "large_h0" is compared with)
    "large_h0": ([{"I": -1.0, "tf": 300.0}], 1.0, {"init_step": 100.0}, None),                     # the first attempts fail the error test: ida_restore
    "max_order_1": ([{"I": -1.0, "tf": 1500.0}], 1.0, {"max_order": 1}, None),
    "max_order_2": ([{"I": -1.0, "tf": 1500.0}], 1.0, {"max_order": 2}, None),
    "max_order_5": ([{"I": -1.0, "tf": 300.0}], 1.0, {"max_order": 5, "reltol": 1e-8, "abstol": 1e-10}, None),     # (tolerances at which the controller climbs to order 5)
    "output_full": ([{"I": -1.0}], 1.0, {}, 12),
    "stall": ([{"I": -1.0}], 0.15, {"check_bounds": False}, None),                                # no bound stops the discharge: depletion, ida_step gives up (PLH_ERR_STALL)
}

WORKER = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np, pkgload
pkg = pkgload.load()
cases = %(cases)r
p = pkg.petlion(pkg.LCO, _lib_path=sys.argv[1])
Th = pkg.configs.sweep_theta(p, np.arange(%(n)d), 4)
out = {}
for name, (proto, soc, okw, mp) in cases.items():
    o = pkg.Opts()
    for k, v in okw.items():
        setattr(o, k, v)
    e = pkg.simulate_ensemble(p, Th, proto, SOC=soc, opts=o, max_points=mp)
    npts = np.asarray(e.n_pts)
    for f in ("t", "V", "I", "SOC"):
        a = np.asarray(getattr(e, f)).copy()
        for i in range(len(npts)):
            a[i, npts[i]:] = 0.0                      # (entries beyond n_pts are never written)
        out[name + "/" + f] = a
    out[name + "/Y"] = np.asarray(e.Y); out[name + "/YP"] = np.asarray(e.YP); out[name + "/n_pts"] = npts
    ri = np.asarray(e.run_info)
    for f in ri.dtype.names:
        out[name + "/run_info/" + f] = np.ascontiguousarray(ri[f])
    cn = np.asarray(e.counters)
    for f in cn.dtype.names:
        if f != "cyc":
            out[name + "/counters/" + f] = np.ascontiguousarray(cn[f])
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """every case through the new and the old step boundary (one process per library: both export the same C symbols)"""
    import build_emu
    libs = {"new": build_emu.build(variant=0), "old": build_emu.build(variant=0, extra=["-DPL_OLD_STEP_BOUNDARY"], tag="_oldsb")}
    d = tmp_path_factory.mktemp("step_boundary")
    code = WORKER % dict(root=ROOT, cases=CASES, n=N_CELLS)
    res = {}
    for k, lib in libs.items():
        f = str(d / (k + ".npz"))
        subprocess.check_call([sys.executable, "-c", code, lib, f])
        res[k] = dict(np.load(f))
    return res


def assert_bit_equal(both, case):
    new, old = both["new"], both["old"]
    keys = sorted(k for k in old if k.startswith(case + "/"))
    assert keys and keys == sorted(k for k in new if k.startswith(case + "/"))
    for k in keys:
        a, b = new[k], old[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert a.tobytes() == b.tobytes(), (k, np.argwhere(a != b)[:4])             # (bytes: NaN-safe and sign-of-zero-exact)


def test_bound_fires_and_back_interpolates(both):
    """1C discharge to SOC_min: the end point is interpolated between the last two accepted points from the history, which must be the unscaled one"""
    r = both["new"]
    assert (r["bound/run_info/flag"][:, 0] == 3).all()
    last = r["bound/t"][np.arange(N_CELLS), r["bound/n_pts"] - 1]
    assert (r["bound/run_info/t_end"][:, 0] == last).all() and (np.abs(r["bound/SOC"][np.arange(N_CELLS), r["bound/n_pts"] - 1]) < 1e-9).all()      # ends ON the bound
    assert_bit_equal(both, "bound")


def test_tf_inside_a_step(both):
    """the run ends at tf, which no free step would hit: the step is clamped, ends on tstop, and the point comes from ida_get_solution"""
    r = both["new"]
    assert (r["tf_inside_step/run_info/flag"][:, 0] == 0).all() and (r["tf_inside_step/run_info/t_end"][:, 0] == 1000.0).all()
    free = both["new"]["bound/t"]                                                    # (the same cells without tf: no accepted point at 1000 s)
    assert not (free == 1000.0).any()
    assert_bit_equal(both, "tf_inside_step")


def test_continuation_and_reinitialisation(both):
    """[1C for 600 s, rest 600 s]: the second run starts from the first's end state, is re-initialised, and stops 1 s after its start"""
    r = both["new"]
    assert (r["continuation/run_info/flag"] == 0).all()
    t1 = np.nextafter(600.0, 1e300) + 1.0
    assert all((r["continuation/t"][i, :r["continuation/n_pts"][i]] == t1).any() for i in range(N_CELLS))        # the tstop at run-local t = 1
    assert (r["continuation/run_info/t_end"][:, 1] > 1199.0).all() and (r["continuation/counters/n_init_iters"] > 0).all()
    assert_bit_equal(both, "continuation")


def test_failed_first_steps_restore_the_history(both):
    """init_step = 100 s: the first attempts fail the error test, ida_restore undoes the rescaling and the step is retried"""
    r = both["new"]
    assert (r["large_h0/counters/n_errfail"] > r["default_h0/counters/n_errfail"]).any()
    assert (r["large_h0/run_info/flag"][:, 0] == 0).all()
    assert_bit_equal(both, "default_h0")
    assert_bit_equal(both, "large_h0")


@pytest.mark.parametrize("maxord", [1, 2, 5])
def test_max_order(both, maxord):
    """orders 4 and 5 off (1, 2) and on (5); no growth of the history at maxord.  sum_kp2 = sum over the steps of (order + 2)"""
    r = both["new"]
    case = "max_order_%d" % maxord
    steps, skp2 = r[case + "/counters/n_steps"], r[case + "/counters/sum_kp2"]
    assert (r[case + "/run_info/flag"][:, 0] == 0).all()
    if maxord == 1:
        assert (skp2 == 3 * steps).all()
    elif maxord == 2:
        assert (skp2 > 3 * steps).all() and (skp2 <= 4 * steps).all() and (skp2 > 3.5 * steps).any()       # order 2 most of the way
    else:
        assert (skp2 > 6 * steps).any()                                                                 # mean order above 4: order 5 was used
    assert_bit_equal(both, case)


def test_output_buffer_full(both):
    """max_points = 12: the run ends on PLH_ERR_OUTPUT_FULL, inside the step loop, on an accepted point"""
    r = both["new"]
    assert (r["output_full/run_info/flag"][:, 0] == ERR_OUTPUT_FULL).any() and (r["output_full/n_pts"] == 12).all()
    assert_bit_equal(both, "output_full")


def test_run_that_ends_on_a_stall(both):
    """check_bounds off, 1C from SOC 0.15: the anode runs empty after 60 - 90 accepted steps and ida_step gives up after ten failed attempts.  The run then ends on the iterate
    of the last attempt -- Y_final, YP_final, run_info -- which the new step boundary forms in cell_simulate because ida_nls no longer does"""
    r = both["new"]
    assert (r["stall/run_info/flag"][:, 0] == ERR_STALL).all() and (r["stall/counters/n_steps"] > 10).all()
    assert (r["stall/counters/n_convfail"] + r["stall/counters/n_errfail"] >= 10).all()
    assert_bit_equal(both, "stall")

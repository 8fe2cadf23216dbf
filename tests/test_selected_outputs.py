"""Selected state sections per saved point (plh_outputs.n_sel / sel / Y_sel; `sections=` of simulate_ensemble / simulate / simulate_b): the reference keeps what the user
names -- outputs = (:t, :V, :c_e) saves c_e per step and nothing else (solution_states_logic, src/outputs.jl:107-131; set_vars!, src/save_outputs.jl:11-40).  The device writes
only the named entries of every saved state vector, packed in the order given.  Here on the wave-emulator build of the device source (no GPU): Y_sel must hold the BITS of the
corresponding columns of the full state dump Y_all, and asking for it must change nothing else -- both calls run the same kernel instantiation."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# two runs from SOC 0.1: a 2C charge that ends on the SOC_max bound (exit flag 4, back-interpolated last point) after about 180 s, then 100 s of discharge that end on time
PROTO = [{"I": 2.0, "tf": 1000.0, "SOC_max": 0.2}, {"I": -1.0, "tf": 100.0}]
SOC0 = 0.1
SCALARS = ("t", "V", "I", "SOC")


def two_cells(pkg, p):
    Th = pkg.theta_matrix(p, 2)
    Th[1, p.θ_keys.index("D_sp")] *= 1.25
    Th[1, p.θ_keys.index("k_p")] *= 0.8
    return Th


def same_everything_else(a, b):
    """every output two calls share, bit for bit: the per-point scalars up to n_pts, the summaries, the final states"""
    assert np.array_equal(a.n_pts, b.n_pts)
    for c in range(a.n_cells):
        n = int(a.n_pts[c])
        for nm in SCALARS + (("T_avg",) if a.T_avg is not None else ()):
            assert np.array_equal(getattr(a, nm)[c, :n], getattr(b, nm)[c, :n]), (nm, c)
    assert (a.T_avg is None) == (b.T_avg is None)
    assert a.run_info.tobytes() == b.run_info.tobytes()
    assert a.counters.tobytes() == b.counters.tobytes()
    assert np.array_equal(a.Y, b.Y) and np.array_equal(a.YP, b.YP)


def check_sections_against_the_full_dump(pkg, p, sections):
    Th = two_cells(pkg, p)
    full = pkg.simulate_ensemble(p, Th, PROTO, SOC=SOC0, outputs="all")
    ens = pkg.simulate_ensemble(p, Th, PROTO, SOC=SOC0, sections=sections)
    assert (full.run_info["flag"][:, 0] == 4).all() and (full.run_info["flag"][:, 1] == 0).all()          # a run that ends on a bound, a run that ends on time
    assert not np.array_equal(full.t[0], full.t[1])                                                       # (the two cells are different cells)
    assert ens.Y_all is None and full.Y_sel is None
    lens = [p.ind[s].stop - p.ind[s].start for s in sections]
    assert ens.Y_sel.shape == (2, ens.t.shape[1], sum(lens))
    starts = [p.ind[s].start for s in sections]
    assert starts != sorted(starts)                                                                       # (the order asked for is not the order of the state vector)
    off = 0
    for s, ln in zip(sections, lens):
        assert ens.sel_ind[s] == slice(off, off + ln)
        for c in range(2):
            n = int(full.n_pts[c])
            assert n > 10
            assert np.array_equal(ens.Y_sel[c, :n, off:off + ln], full.Y_all[c, :n, p.ind[s]]), (s, c)
            assert np.array_equal(ens.section(s)[c, :n], full.section(s)[c, :n]), (s, c)
        off += ln
    same_everything_else(full, ens)
    # a single cell of the ensemble: sol.<name> comes from Y_sel, anything else was not saved
    s0, f0 = ens[1], full[1]
    for s in sections:
        assert np.array_equal(getattr(s0, s), getattr(f0, s))
    missing = next(k for k in p.ind if k not in sections)
    with pytest.raises(AttributeError):
        getattr(s0, missing)
    return full, ens


def test_sections_lco(emu_model, pkg):
    check_sections_against_the_full_dump(pkg, emu_model, ("Φ_s", "c_e", "j"))


def test_sections_nmc_sei(emu_model_nmc_sei, pkg):
    check_sections_against_the_full_dump(pkg, emu_model_nmc_sei, ("SOH", "film", "c_e"))


def test_sections_thermal(emu_model_thermal, pkg):
    check_sections_against_the_full_dump(pkg, emu_model_thermal, ("T", "c_e"))


def test_names_and_index_ranges_mix(emu_model, pkg):
    """a (start, len) pair next to a name; the accessor and the slice map carry the pair as its key"""
    p = emu_model
    Th = two_cells(pkg, p)
    proto = [{"I": -1.0, "tf": 60.0}]
    full = pkg.simulate_ensemble(p, Th, proto, SOC=1.0, outputs="all")
    a = p.ind["Φ_e"].start + 3
    ens = pkg.simulate_ensemble(p, Th, proto, SOC=1.0, sections=((p.N.tot - 1, 1), "c_e", (a, 5)))
    n = int(full.n_pts[0])
    assert ens.sel == ((p.N.tot - 1, 1), (p.ind["c_e"].start, 30), (a, 5)) and ens.Y_sel.shape[2] == 36
    assert np.array_equal(ens.Y_sel[0, :n, 0], full.Y_all[0, :n, -1]) and np.array_equal(ens.section((a, 5))[0, :n], full.Y_all[0, :n, a:a + 5])
    assert np.array_equal(ens.section("c_e")[0, :n], full.Y_all[0, :n, p.ind["c_e"]])
    with pytest.raises(KeyError):
        ens.section("Φ_s")
    with pytest.raises(ValueError):
        pkg.simulate_ensemble(p, Th, proto, SOC=1.0, sections=("c_e", "no_such_state"))
    with pytest.raises(ValueError):
        pkg.simulate_ensemble(p, Th, proto, SOC=1.0, sections=("c_e", "c_e"))


def _raw_call(pkg, p, Th, proto, soc, max_pts, sel, want_all=False, ysel_fill=None, n_sel=None, pass_ysel=True):
    """plh_integrate through the ctypes mirror with the caller's own (start, len) pairs: (return code, message, buffers)"""
    cap = pkg._capi
    api = sys.modules[pkg.__name__ + ".api"]
    lib, n, N = p._lib, Th.shape[0], p.N.tot
    runs, _ = pkg.make_protocol(p, proto, n)
    arr = (cap.Run * len(runs))(*runs)
    os_ = api._opts_struct(pkg.Opts(), p)
    sel = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1, 2)
    tot = max(int(np.abs(sel[:, 1]).sum()), 1)
    b = dict(t=np.full((n, max_pts), np.nan), V=np.full((n, max_pts), np.nan), n_pts=np.zeros(n, np.int32), Y=np.zeros((n, N)),
             run_info=np.zeros((n, len(runs)), cap.RUN_INFO_DTYPE), Y_sel=np.full((n, max_pts, tot), np.nan if ysel_fill is None else ysel_fill),
             Y_all=np.full((n, max_pts, N), np.nan) if want_all else None)
    out = cap.Outputs()
    out.max_pts = max_pts
    out.t, out.V, out.n_pts, out.Y_final, out.run_info = cap.ptr(b["t"]), cap.ptr(b["V"]), cap.ptr(b["n_pts"]), cap.ptr(b["Y"]), cap.ptr(b["run_info"])
    out.Y_all = cap.ptr(b["Y_all"])
    out.n_sel = len(sel) if n_sel is None else n_sel
    out.sel = sel.ctypes.data_as(C.POINTER(C.c_int)) if len(sel) else None
    out.Y_sel = cap.ptr(b["Y_sel"]) if pass_ysel else None
    soc0 = np.full(n, float(soc))
    rc = lib.plh_integrate(p._h, n, cap.ptr(np.ascontiguousarray(Th)), cap.ptr(soc0), None, None, len(runs), arr, C.byref(os_), C.byref(out), cap.PLH_HOST, None)
    return rc, lib.plh_last_error().decode("utf-8", "replace"), b


def test_c_abi_argument_rules(emu_model, pkg):
    p = emu_model
    Th, proto, N, E_ARG = two_cells(pkg, p), [{"I": -1.0, "tf": 60.0}], emu_model.N.tot, -1
    bad = {"overlap": [(0, 10), (5, 10)], "one entry twice": [(7, 1), (7, 1)], "past the end": [(N - 3, 4)], "negative start": [(-1, 4)], "start beyond N": [(N, 1)],
           "empty range": [(0, 0)], "negative length": [(4, -2)]}
    for what, sel in bad.items():
        rc, msg, b = _raw_call(pkg, p, Th, proto, 1.0, 64, sel)
        assert rc == E_ARG and "sel" in msg, (what, rc, msg)
        assert np.isnan(b["Y_sel"]).all() and (b["n_pts"] == 0).all(), what                # refused before anything ran: nothing clamped, nothing written
    seventeen = [(k, 1) for k in range(17)]
    rc, msg, _ = _raw_call(pkg, p, Th, proto, 1.0, 64, seventeen)
    assert rc == E_ARG and "n_sel" in msg, (rc, msg)
    rc, msg, _ = _raw_call(pkg, p, Th, proto, 1.0, 64, [(0, 1)], n_sel=-1)
    assert rc == E_ARG and "n_sel" in msg, (rc, msg)
    rc, msg, _ = _raw_call(pkg, p, Th, proto, 1.0, 64, [], n_sel=0)                           # Y_sel without ranges
    assert rc == E_ARG and "Y_sel" in msg, (rc, msg)
    # sixteen ranges are allowed; and so is the whole state vector in one range
    sixteen = [(2 * k, 1) for k in range(16)]
    rc, msg, b = _raw_call(pkg, p, Th, proto, 1.0, 64, sixteen, want_all=True)
    assert rc == 0, msg
    n = int(b["n_pts"][0])
    assert n > 3 and np.array_equal(b["Y_sel"][0, :n], b["Y_all"][0, :n, 0:32:2])
    rc, msg, b = _raw_call(pkg, p, Th, proto, 1.0, 64, [(0, N)], want_all=True)
    n1 = int(b["n_pts"][1])
    assert rc == 0 and n1 > 3 and np.array_equal(b["Y_sel"][1, :n1], b["Y_all"][1, :n1]), msg
    # ranges without a Y_sel pointer: checked like any others, nothing selected
    rc, msg, _ = _raw_call(pkg, p, Th, proto, 1.0, 64, [(0, 10), (5, 10)], pass_ysel=False)
    assert rc == E_ARG
    rc, msg, _ = _raw_call(pkg, p, Th, proto, 1.0, 64, [(0, 10)], pass_ysel=False)
    assert rc == 0, msg


def test_y_all_and_y_sel_together_agree(emu_model_thermal, pkg):
    p = emu_model_thermal
    sel = [(p.ind["T"].start + 5, 20), (p.ind["I"].start, 1), (p.ind["c_e"].start, 30)]
    rc, msg, b = _raw_call(pkg, p, two_cells(pkg, p), PROTO, SOC0, 256, sel, want_all=True)
    assert rc == 0, msg
    for c in range(2):
        n = int(b["n_pts"][c])
        assert n > 10
        cols = np.concatenate([np.arange(a, a + ln) for a, ln in sel])
        assert np.array_equal(b["Y_sel"][c, :n], b["Y_all"][c, :n][:, cols]), c
    assert np.isnan(b["Y_sel"][:, int(b["n_pts"].max()):]).all()                                  # rows past the longest trajectory of the call are not written
    # and the library's python face gives both when both are asked for
    ens = pkg.simulate_ensemble(p, two_cells(pkg, p), PROTO, SOC=SOC0, outputs="all", sections=("T",))
    n = int(ens.n_pts[0])
    assert np.array_equal(ens.Y_sel[0, :n], ens.Y_all[0, :n, p.ind["T"]])


def test_truncation_at_max_points(emu_model, pkg):
    p = emu_model
    Th = two_cells(pkg, p)
    sel = [(p.ind["Φ_e"].start, 30), (p.ind["c_e"].start + 10, 10)]
    rc, msg, whole = _raw_call(pkg, p, Th, PROTO, SOC0, 256, sel, ysel_fill=-777.0)
    assert rc == 0, msg
    n_whole = whole["n_pts"].copy()
    assert (whole["run_info"]["flag"][:, 1] == 0).all() and n_whole.min() > 12
    mp = 9
    # what the library reports for a short buffer today: the same call with the full state dump instead of a selection (the same kernel instantiation)
    rc, msg, plain = _raw_call(pkg, p, Th, PROTO, SOC0, mp, [], n_sel=0, pass_ysel=False, want_all=True)
    assert rc == 0, msg
    rc, msg, cut = _raw_call(pkg, p, Th, PROTO, SOC0, mp, sel, ysel_fill=-777.0)
    assert rc == 0, msg
    assert np.array_equal(cut["n_pts"], plain["n_pts"]) and cut["run_info"].tobytes() == plain["run_info"].tobytes()
    assert (cut["run_info"]["flag"][:, 0] == pkg._capi.ERR_OUTPUT_FULL).all()
    # sentinel rows around the short buffer: the array handed over is the middle of a larger one
    api = sys.modules[pkg.__name__ + ".api"]
    cap = pkg._capi
    tot = 40
    big = np.full((2 + 2, mp, tot), -777.0)
    runs, _ = pkg.make_protocol(p, PROTO, 2)
    out = cap.Outputs()
    out.max_pts = mp
    t, npts, ri = np.zeros((2, mp)), np.zeros(2, np.int32), np.zeros((2, 2), cap.RUN_INFO_DTYPE)
    sel_a = np.ascontiguousarray(sel, dtype=np.int32)
    out.t, out.n_pts, out.run_info = cap.ptr(t), cap.ptr(npts), cap.ptr(ri)
    out.n_sel, out.sel, out.Y_sel = 2, sel_a.ctypes.data_as(C.POINTER(C.c_int)), cap.ptr(big[1:3])
    os_ = api._opts_struct(pkg.Opts(), p)
    rc = p._lib.plh_integrate(p._h, 2, cap.ptr(np.ascontiguousarray(Th)), cap.ptr(np.full(2, SOC0)), None, None, 2, (cap.Run * 2)(*runs), C.byref(os_), C.byref(out), cap.PLH_HOST, None)
    assert rc == 0
    assert (big[0] == -777.0).all() and (big[3] == -777.0).all()                                 # nothing before the first cell's rows, nothing behind the last cell's
    for c in range(2):
        k = min(int(cut["n_pts"][c]), mp)
        assert k >= mp - 1
        # rows below max_pts are those of the untruncated run (the last row the truncated run wrote is a saved point of the long one too)
        assert np.array_equal(cut["Y_sel"][c, :k], whole["Y_sel"][c, :k]), c
        assert np.array_equal(big[1 + c, :k], whole["Y_sel"][c, :k]), c
        assert np.array_equal(plain["Y_all"][c, :k][:, np.r_[sel[0][0]:sel[0][0] + 30, sel[1][0]:sel[1][0] + 10]], cut["Y_sel"][c, :k]), c
    # the long buffer: rows beyond the longest trajectory of the call keep the sentinel (the way back copies whole rows up to it), the saved rows do not
    assert (whole["Y_sel"][:, int(n_whole.max()):] == -777.0).all()
    for c in range(2):
        assert not (whole["Y_sel"][c, :int(n_whole[c])] == -777.0).any()


def test_simulate_and_simulate_b(emu_model, pkg):
    p = emu_model
    kw1, kw2 = dict(I=2.0, SOC=SOC0, SOC_max=0.2), dict(I=-1.0)
    sol = pkg.simulate(p, 1000.0, sections=("c_e",), **kw1)
    n1 = len(sol.t)
    assert sol.Y_all is None and sol.Y_sel.shape == (n1, 30) and sol.c_e.shape == (n1, 30)
    pkg.simulate_b(sol, p, 100.0, **kw2)
    ref = pkg.simulate(p, 1000.0, outputs="all", **kw1)
    pkg.simulate_b(ref, p, 100.0, **kw2)
    assert len(sol.t) > n1 + 3 and len(sol.results) == 2 and sol.results[0].flag == 4
    assert np.array_equal(sol.t, ref.t) and np.array_equal(sol.V, ref.V)
    assert sol.c_e.shape == (len(sol.t), 30) and np.array_equal(sol.c_e, ref.c_e)                  # one row per saved point over both runs
    tq = [0.5 * (sol.t[2] + sol.t[3]), 0.5 * (sol.t[n1 + 1] + sol.t[n1 + 2])]
    a, b = sol(tq), ref(tq)
    assert a.c_e.shape == (2, 30) and np.array_equal(a.c_e, b.c_e) and np.array_equal(a.V, b.V)
    with pytest.raises(AttributeError):
        sol.Φ_s
    with pytest.raises(AttributeError):
        a.Φ_s
    n2 = len(sol.t)
    with pytest.raises(ValueError):
        pkg.simulate_b(sol, p, 50.0, sections=("c_e", "j"), **kw2)
    with pytest.raises(ValueError):
        pkg.simulate_b(ref, p, 50.0, sections=("c_e",), **kw2)                                     # a solution saved without a selection does not gain one
    assert len(sol.t) == n2 and len(ref.t) == n2                                                   # (a refused continuation leaves the solution as it was)
    pkg.simulate_b(sol, p, 50.0, sections=("c_e",), **kw2)                                         # naming the same selection again is fine
    assert sol.c_e.shape[0] == len(sol.t) > n2


def test_mirrors_carry_the_new_fields(pkg):
    """the last three fields of plh_outputs in the header, the ctypes struct and the Julia struct (parsed as tests/test_capi_symbols.py parses it)"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "petlion_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} plh_outputs;", hdr).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls[-3:] == ["int n_sel", "const int* sel", "double* Y_sel"]
    cap = pkg._capi
    assert [f for f, _ in cap.Outputs._fields_][-4:] == ["Y_all", "n_sel", "sel", "Y_sel"]
    assert cap.Outputs.n_sel.size == 4 and cap.Outputs.sel.size == 8 and cap.Outputs.Y_sel.size == 8
    assert cap.Outputs.sel.offset == cap.Outputs.n_sel.offset + 8 and cap.Outputs.Y_sel.offset == cap.Outputs.sel.offset + 8 and C.sizeof(cap.Outputs) == cap.Outputs.Y_sel.offset + 8
    jl = open(os.path.join(ROOT, "bindings", "julia", "PetlionHIP.jl")).read()
    jbody = re.sub(r"#.*", "", re.search(r"struct Outputs\b[^\n]*\n(.*?)\nend", jl, flags=re.S).group(1))
    fields = re.findall(r"(\w+)::\s*([A-Za-z_]+(?:\{[^;\n]*?\})?)", jbody)
    assert fields[-4:] == [("Y_all", "Ptr{Cdouble}"), ("n_sel", "Cint"), ("sel", "Ptr{Cint}"), ("Y_sel", "Ptr{Cdouble}")]
    # every place the Julia binding builds the struct passes as many values as it has fields
    for m in re.finditer(r"Ref\(Outputs\((.*?)\)\)\n", jl, flags=re.S):
        depth, n_args = 0, 1
        for ch in m.group(1):
            depth += ch in "([{"
            depth -= ch in ")]}"
            n_args += ch == "," and depth == 0
        assert n_args == len(fields), m.group(1)[:60]


def test_library_reports_the_new_fields(emu_model, pkg):
    """plh_abi_layout() of the library under test lists 15 fields for plh_outputs, the last three where the mirror has them"""
    lib = emu_model._lib
    lib.plh_abi_layout.argtypes = [C.c_void_p, C.c_int]
    n = lib.plh_abi_layout(None, 0)
    buf = (C.c_int * n)()
    assert lib.plh_abi_layout(buf, n) == n
    vals, k = list(buf), 0
    for _ in range(6):
        k += 2 + vals[k + 1]
    size, nf = vals[k], vals[k + 1]
    offs = vals[k + 2:k + 2 + nf]
    cap = pkg._capi
    assert k + 2 + nf == n and nf == 15 and size == C.sizeof(cap.Outputs)
    assert offs[-3:] == [cap.Outputs.n_sel.offset, cap.Outputs.sel.offset, cap.Outputs.Y_sel.offset]

"""The three ways the outputs of plh_integrate travel (PLH_HOST, PLH_HOST_ASYNC + plh_synchronize, PLH_DEVICE) give the same bits, for every subset of the optional
arrays -- a characterisation of the host side of the call (csrc/petlion_hip.hip: argument rules, per-stream workspaces and cached uploads, the output table, the way back
of a blocking host call).  On the wave-emulator build "device" memory is host memory: PLH_DEVICE takes numpy pointers and is the reference for the two host kinds.

What a blocking PLH_HOST call does to the caller's arrays (include/petlion_hip.h): an array that is not requested is not written; per-point entries at columns >=
max(n_pts) of the call receive no results; and the first touch of a requested array's pages may write ZERO bytes anywhere inside that array before the results arrive.
That touch is known exactly for the sizes used here: an array of less than a page (the per-point scalar arrays) has its first and last byte written, an array whose
rows are longer than a page (Y_all, Y_sel) bytes 0 and 4095 of every row.  The sentinel check below allows those bytes to hold zero and nothing else to change."""
import ctypes as C
import sys

import numpy as np
import pytest

OPTIONAL = ("t", "V", "I", "SOC", "T_avg", "n_pts", "Y_final", "YP_final", "counters", "Y_all", "Y_sel")
PER_POINT = ("t", "V", "I", "SOC", "T_avg", "Y_all", "Y_sel")
SUBSETS = dict([("everything", OPTIONAL), ("only run_info", ())] + [("no " + nm, tuple(k for k in OPTIONAL if k != nm)) for nm in OPTIONAL])
N_CELLS, MAX_PTS, SENT, GUARD = 3, 48, 0xA5, 64
PROTO = [{"I": -1.0, "tf": 20.0}]
E_ARG, E_UNSUPPORTED = -1, -2
_memo = {}


def thetas(pkg, p):
    """three different cells: their step sequences, and so their n_pts, differ"""
    Th = pkg.theta_matrix(p, N_CELLS)
    Th[1, p.θ_keys.index("D_sp")] *= 0.2
    Th[1, p.θ_keys.index("k_p")] *= 0.1
    Th[2, p.θ_keys.index("D_sn")] *= 0.05
    Th[2, p.θ_keys.index("D_e" if "D_e" in p.θ_keys else "D_s")] *= 0.3
    return np.ascontiguousarray(Th)


def sel_ranges(p):
    return [(p.ind["Φ_e"].start + 3, 7), (p.ind["c_e"].start + 2, 5)]              # two ranges, not in the order of the state vector


def call(pkg, p, kind, want, max_pts=MAX_PTS, tstops=None, proto=PROTO, mutate=None, soc=1.0):
    """one plh_integrate through the ctypes mirror.  Every output array, requested or not, lies in ONE sentinel-filled arena with guard bytes between the arrays; only
    the requested ones are handed over.  -> (return code, message, {name: array}, arena, {name: (offset, bytes)})"""
    cap, api = pkg._capi, sys.modules[pkg.__name__ + ".api"]
    lib, n, N = p._lib, N_CELLS, p.N.tot
    runs, _ = pkg.make_protocol(p, proto, n)
    arr = (cap.Run * len(runs))(*runs)
    o = pkg.Opts()
    if tstops is not None:
        o.tstops = list(tstops)
    os_ = api._opts_struct(o, p)
    sel = np.ascontiguousarray(sel_ranges(p), dtype=np.int32)
    n_selt, mp = int(sel[:, 1].sum()), max(max_pts, 1)
    shapes = dict(t=((n, mp), np.float64), V=((n, mp), np.float64), I=((n, mp), np.float64), SOC=((n, mp), np.float64), T_avg=((n, mp), np.float64),
                  n_pts=((n,), np.int32), Y_final=((n, N), np.float64), YP_final=((n, N), np.float64), run_info=((n, len(runs)), cap.RUN_INFO_DTYPE),
                  counters=((n,), cap.COUNTERS_DTYPE), Y_all=((n, mp, N), np.float64), Y_sel=((n, mp, n_selt), np.float64))
    where, off = {}, GUARD
    for nm, (shape, dt) in shapes.items():
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        where[nm] = (off, nb)
        off += (nb + GUARD + 63) // 64 * 64
    arena = np.full(off, SENT, np.uint8)
    b = {nm: arena[where[nm][0]:where[nm][0] + where[nm][1]].view(shapes[nm][1]).reshape(shapes[nm][0]) for nm in shapes}
    out = cap.Outputs()
    out.max_pts = max_pts
    for nm in want + ("run_info",):
        setattr(out, nm, cap.ptr(b[nm]))
    out.n_sel, out.sel = len(sel), sel.ctypes.data_as(C.POINTER(C.c_int))
    Th, soc0 = thetas(pkg, p), np.full(n, float(soc))
    args = dict(n=n, theta=cap.ptr(Th), soc=cap.ptr(soc0), Y_init=None, t_init=None, n_runs=len(runs), runs=arr, opts=os_, out=out, kind=kind)
    if mutate:
        mutate(args)
    rc = lib.plh_integrate(p._h, args["n"], args["theta"], args["soc"], args["Y_init"], args["t_init"], args["n_runs"], args["runs"], C.byref(args["opts"]),
                           C.byref(args["out"]), args["kind"], None)
    msg = lib.plh_last_error().decode("utf-8", "replace") if rc else ""
    if rc == 0 and kind == cap.PLH_HOST_ASYNC:
        assert lib.plh_synchronize(p._h, None) == 0
    return rc, msg, b, arena, where


def untouched_outside(arena, where, want, host_blocking):
    """guards and arrays that were not requested still hold the sentinel"""
    mask = np.ones(arena.size, bool)
    for nm in want + ("run_info",):
        mask[where[nm][0]:where[nm][0] + where[nm][1]] = False
    assert (arena[mask] == SENT).all(), "bytes outside the requested arrays were written"


def compare(pkg, ref, got, want, n_pts, what, blocking_host):
    rc, msg, b, arena, where = got
    assert rc == 0, (what, msg)
    untouched_outside(arena, where, want, blocking_host)
    rb = ref[2]
    assert b["run_info"].tobytes() == rb["run_info"].tobytes(), what
    mp = b["t"].shape[1]
    for nm in want:
        if nm in PER_POINT:
            for c in range(N_CELLS):
                k = min(int(n_pts[c]), mp)
                assert b[nm][c, :k].tobytes() == rb[nm][c, :k].tobytes(), (what, nm, c)
            if blocking_host:                                   # columns >= max(n_pts): no results; only the first touch's zero bytes
                maxn = min(int(n_pts.max()), mp)
                rows = b[nm].view(np.uint8).reshape(N_CELLS, -1)
                pitch = rows.shape[1]
                assert rows.size <= 4096 or pitch > 4096                     # (the two shapes of the first touch this file's sizes reach)
                touched = {(N_CELLS - 1, pitch - 1)} if pitch <= 4096 else {(c, 4095) for c in range(N_CELLS)}
                first = maxn * (pitch // mp)
                for c, k in np.argwhere(rows[:, first:] != SENT):
                    assert (int(c), int(k) + first) in touched and rows[c, k + first] == 0, (what, nm, c, k + first)
        else:
            assert b[nm].tobytes() == rb[nm].tobytes(), (what, nm)


def reference(pkg, p, name, **kw):
    key = (id(p), name, tuple(sorted(kw.items())))
    if key not in _memo:
        _memo[key] = call(pkg, p, pkg._capi.PLH_DEVICE, SUBSETS[name], **kw)
        assert _memo[key][0] == 0, _memo[key][1]
        untouched_outside(_memo[key][3], _memo[key][4], SUBSETS[name], False)
    return _memo[key]


def npts_of(pkg, p, **kw):
    return reference(pkg, p, "everything", **kw)[2]["n_pts"].copy()


def test_the_cells_differ(emu_model, pkg):
    n_pts = npts_of(pkg, emu_model)
    assert len(set(n_pts.tolist())) == N_CELLS and 8 <= n_pts.min() and n_pts.max() < MAX_PTS, n_pts
    b = reference(pkg, emu_model, "everything")[2]
    assert (b["run_info"]["flag"] == 0).all()
    assert not (b["Y_all"][0, :int(n_pts[0])].view(np.uint8) == SENT).all(axis=-1).any()


@pytest.mark.parametrize("name", list(SUBSETS))
def test_subsets_agree_across_pointer_kinds(emu_model, pkg, name):
    """the reference of every subset that saves states is the ONE PLH_DEVICE call with everything: what an array holds does not depend on which others are asked for
    (run_info alone runs another kernel instantiation and has a reference call of its own)"""
    p, cap, want = emu_model, pkg._capi, SUBSETS[name]
    n_pts = npts_of(pkg, p)
    ref = reference(pkg, p, "only run_info" if name == "only run_info" else "everything")
    for kind, what in ((cap.PLH_HOST, "PLH_HOST"), (cap.PLH_HOST_ASYNC, "PLH_HOST_ASYNC")):
        compare(pkg, ref, call(pkg, p, kind, want), want, n_pts, (name, what), kind == cap.PLH_HOST)
    if name == "everything":        # the same call again: cached uploads (protocol, selection map) and staging blocks are reused
        compare(pkg, ref, call(pkg, p, cap.PLH_HOST, want), want, n_pts, (name, "PLH_HOST, second call"), True)


def test_thermal_T_avg(emu_model_thermal, pkg):
    p, cap = emu_model_thermal, pkg._capi
    n_pts = npts_of(pkg, p)
    ref = reference(pkg, p, "everything")
    T = ref[2]["T_avg"]
    assert len(set(T[0, :int(n_pts[0])].tolist())) > 3                       # a temperature that moves
    for kind in (cap.PLH_HOST, cap.PLH_HOST_ASYNC):
        compare(pkg, ref, call(pkg, p, kind, OPTIONAL), OPTIONAL, n_pts, ("thermal", kind), kind == cap.PLH_HOST)


@pytest.mark.parametrize("max_pts", [0, 5])
def test_no_room_and_truncation(emu_model, pkg, max_pts):
    """max_pts = 0 with the per-point pointers given: nothing per point is written; max_pts below the longest trajectory: the rows are cut there, in every kind"""
    p, cap = emu_model, pkg._capi
    ref = reference(pkg, p, "everything", max_pts=max_pts)
    n_pts = ref[2]["n_pts"].copy()
    if max_pts:
        assert n_pts.max() >= max_pts and (ref[2]["run_info"]["flag"][:, 0] == cap.ERR_OUTPUT_FULL).all()
        whole = reference(pkg, p, "everything")[2]
        for c in range(N_CELLS):
            assert ref[2]["t"][c, :max_pts - 1].tobytes() == whole["t"][c, :max_pts - 1].tobytes()
    for kind in (cap.PLH_HOST, cap.PLH_HOST_ASYNC):
        got = call(pkg, p, kind, OPTIONAL, max_pts=max_pts)
        if max_pts == 0:
            for nm in PER_POINT:
                assert (got[2][nm].view(np.uint8) == SENT).all(), (kind, nm)
            n_pts_cmp = np.zeros(N_CELLS, np.int32)
        else:
            n_pts_cmp = n_pts
        compare(pkg, ref, got, OPTIONAL, n_pts_cmp, ("max_pts", max_pts, kind), kind == cap.PLH_HOST and max_pts > 0)


def test_tstops_change_and_return(pkg):
    """tstops A, then B, then A again on one handle: each the result of a fresh handle (the per-stream device copy follows the caller's list)"""
    import build_emu
    cap = pkg._capi
    A, B = (7.0, 19.5), (11.0, 3.0, 16.0)
    want = ("t", "V", "n_pts", "Y_final")
    fresh = {}
    for ts in (A, B):
        p = pkg.petlion(pkg.LCO, _lib_path=build_emu.build())
        fresh[ts] = call(pkg, p, cap.PLH_HOST, want, tstops=ts)
        assert fresh[ts][0] == 0, fresh[ts][1]
        k = int(fresh[ts][2]["n_pts"][0])
        assert all(t in fresh[ts][2]["t"][0, :k] for t in ts)                # the integrator stopped at the listed times
    assert fresh[A][2]["t"].tobytes() != fresh[B][2]["t"].tobytes()
    p = pkg.petlion(pkg.LCO, _lib_path=build_emu.build())
    for ts in (A, B, A):
        got = call(pkg, p, cap.PLH_HOST, want, tstops=ts)
        compare(pkg, fresh[ts], got, want, fresh[ts][2]["n_pts"], ("tstops", ts), True)


def _refused(pkg, p, mutate, proto=PROTO, **kw):
    rc, msg, b, arena, _ = call(pkg, p, pkg._capi.PLH_HOST, OPTIONAL, mutate=mutate, proto=proto, **kw)
    assert (arena == SENT).all()                                              # refused before anything ran
    return rc, msg


def test_refusals_keep_their_code_text_and_order(emu_model, pkg):
    p, cap = emu_model, pkg._capi

    def bad_sel(a):
        a["_sel"] = np.ascontiguousarray([(0, 10), (5, 10)], dtype=np.int32)
        a["out"].n_sel, a["out"].sel = 2, a["_sel"].ctypes.data_as(C.POINTER(C.c_int))

    def t_init_alone(a):
        a["_t"] = np.zeros(N_CELLS)
        a["t_init"] = cap.ptr(a["_t"])

    def bad_refine(a):
        a["opts"].refine = 5

    def both(*fs):
        return lambda a: [f(a) for f in fs]
    # the head of the call
    assert _refused(pkg, p, lambda a: a.update(kind=7)) == (E_ARG, "bad ptr_kind")
    assert _refused(pkg, p, lambda a: a.update(n=0)) == (E_ARG, "bad argument")
    # the protocol
    assert _refused(pkg, p, None, proto=[{"I": -1.0, "tf": 0.0}]) == (E_ARG, "run length tf must be positive")
    assert _refused(pkg, p, None, proto=[{"dT": -1.0, "tf": 10.0}]) == (
        E_UNSUPPORTED, "operating mode not available for this model (I, V, P, eta_p; dT with temperature = true)")
    # the outputs
    assert _refused(pkg, p, None, max_pts=-1) == (E_ARG, "max_pts")
    assert _refused(pkg, p, bad_sel) == (E_ARG, "plh_outputs.sel: ranges may not overlap")
    assert _refused(pkg, p, t_init_alone) == (E_ARG, "t_init without Y_init")
    # the options
    assert _refused(pkg, p, bad_refine) == (E_ARG, "refine must be 0 .. 4")
    assert _refused(pkg, p, None, tstops=[1.0, float("nan")]) == (E_ARG, "tstops must not contain NaN")
    # the first complaint of a call that is wrong in several ways: protocol, outputs, t_init, options
    assert _refused(pkg, p, both(bad_sel, bad_refine), proto=[{"I": -1.0, "tf": 0.0}])[1] == "run length tf must be positive"
    assert _refused(pkg, p, both(bad_sel, t_init_alone, bad_refine))[1] == "plh_outputs.sel: ranges may not overlap"
    assert _refused(pkg, p, both(t_init_alone, bad_refine))[1] == "t_init without Y_init"


def test_sensitivity_refusals(emu_model, pkg):
    p, cap, api = emu_model, pkg._capi, sys.modules[pkg.__name__ + ".api"]
    n, N = N_CELLS, p.N.tot

    def sens_call(n_sens, cols, refine=0, kind=cap.PLH_HOST):
        runs, _ = pkg.make_protocol(p, PROTO, n)
        os_ = api._opts_struct(pkg.Opts(), p)
        os_.refine = refine
        ri, dY = np.zeros((n, 1), cap.RUN_INFO_DTYPE), np.zeros((n, max(n_sens, 1), N))
        out = cap.Outputs()
        out.max_pts, out.run_info = 0, cap.ptr(ri)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        rc = p._lib.plh_integrate_sens(p._h, n, cap.ptr(thetas(pkg, p)), cap.ptr(np.ones(n)), 1, (cap.Run * 1)(*runs), C.byref(os_), C.byref(out), n_sens,
                                       cols.ctypes.data, cap.ptr(dY), None, None, kind, None)
        return rc, p._lib.plh_last_error().decode("utf-8", "replace")
    assert sens_call(0, [0]) == (E_ARG, "plh_integrate_sens: 1 <= n_sens <= 64, theta columns and at least one of dY_dtheta / dV_dtheta")
    assert sens_call(1, [len(p.θ_keys)]) == (E_ARG, "plh_integrate_sens: theta column out of range")
    assert sens_call(1, [0], refine=1) == (E_UNSUPPORTED, "plh_integrate_sens: not with refine / tdiscon / a stop function")
    assert sens_call(1, [0], refine=5) == (E_ARG, "refine must be 0 .. 4")                     # the options are checked ahead of the sensitivity request
    assert sens_call(1, [0], kind=cap.PLH_HOST_ASYNC) == (E_ARG, "plh_integrate_sens: ptr_kind must be PLH_HOST or PLH_DEVICE")

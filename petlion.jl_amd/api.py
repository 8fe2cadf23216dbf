"""Host-side mirror of the reference's user API for the hot path, over the C ABI (include/petlion_hip.h):

    p   = petlion(LCO; N_p=10, ..., temperature=false)         reference src/external.jl:2-18, src/params.jl:119-174
    sol = simulate(p, tf; I=-1, SOC=1, V_min=..., reltol=...)    reference src/model_evaluation.jl:11-85
    simulate!(sol, p, tf; V=:hold, I_min=1/20)                  reference src/model_evaluation.jl:87-97   (here: simulate_b)
    ens = simulate_ensemble(p, Theta, protocol; SOC=...)         new: the ensemble axis the MI355X path exists for

Julia spellings map as  simulate! -> simulate_b,  :hold -> "hold",  :rest -> "rest",  p.θ[:D_sp] -> p.θ["D_sp"].
Everything numerical happens in the HIP library; this file only marshals arguments (no CPU compute path).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import time
import numpy as np

from . import _capi as cap
from . import closures, grids
from .params import EXIT_REASONS, Bounds, Opts, bounds_LCO, bounds_LGM50, bounds_NMC, calc_I1C, theta_LCO, theta_LGM50, theta_NMC

LCO = "LCO"
NMC = "NMC"
NMC_LGM50 = "LGM50"


class _N:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Model:
    """The reference's `model` struct, reduced to the data contracts of the hot path (src/structures.jl:336-345)."""

    def __init__(self, cathode, N, temperature, aging, lib_path=None, precision="f64", device=-1, solid_diffusion="Fickian", thermodynamic_factor="linear", rxn="BV", waves_per_cell=1, grid_lib=None):
        if cathode not in (LCO, NMC, NMC_LGM50):
            raise NotImplementedError("chemistry %r is outside the hot-path scope (LCO, NMC and NMC_LGM50 are built)" % (cathode,))
        self.cathode = cathode
        self.N = N
        self.temperature = bool(temperature)
        if aging not in (False, None, True, "SEI"):
            raise NotImplementedError("aging=%r: the reference knows false and :SEI (src/params.jl:119-174)" % (aging,))
        aging = "SEI" if aging in (True, "SEI") else False
        self.aging = aging
        self.θ = {LCO: theta_LCO, NMC: theta_NMC, NMC_LGM50: theta_LGM50}[cathode]()
        self.θ["I1C"] = calc_I1C(self.θ)
        self.bounds = {LCO: bounds_LCO, NMC: bounds_NMC, NMC_LGM50: bounds_LGM50}[cathode]()
        self.opts = Opts()
        self._lib = cap.load(lib_path)
        self._lib_path = lib_path
        self._builtin_lib = lib_path is None          # the product library (not the tests' emulator build / an experiment build)
        if precision not in ("f64", "mixed", "f64_reforder"):
            raise ValueError("precision: 'f64', 'mixed' (fp32 storage of the Newton-matrix factors, everything else fp64) or 'f64_reforder' (fp64 with the finite-volume rows in the "
                             "reference's operation order: PLH_PREC_F64_REFORDER)")
        self.precision = precision
        desc = cap.ModelDesc({LCO: cap.CHEM_LCO, NMC: cap.CHEM_NMC, NMC_LGM50: cap.CHEM_LGM50}[cathode], N.p, N.s, N.n, N.a, N.z, N.r_p, N.r_n, int(self.temperature), int(bool(aging)), 8,
                             {"f64": cap.PREC_F64, "mixed": cap.PREC_MIXED, "f64_reforder": cap.PREC_F64_REFORDER}[precision], int(device),
                             {"Fickian": 0, "quadratic": 1, "polynomial": 2}[solid_diffusion], {"linear": 0, "nonlinear": 1}[thermodynamic_factor], {"BV": 0, "MHC": 1}[rxn], int(waves_per_cell))
        self.waves_per_cell = int(waves_per_cell)
        self.solid_diffusion, self.thermodynamic_factor, self.rxn = solid_diffusion, thermodynamic_factor, rxn
        # another discretisation than the built-in 10/10/10/10: its kernels are a library of their own, compiled on first use and cached (grids.py), registered before the
        # handle is created (`grid_lib`: a library built elsewhere -- the tests' emulator build)
        # (N_r_p != N_r_n: a 7-entry grid, the anode's N_r last -- the particle phases then run on the larger of the two as lane stride, dfn_cell.h)
        g = grids.grid_tuple(N.p, N.s, N.n, N.r_p if solid_diffusion == "Fickian" else 10, N.a if self.temperature else 10, N.z if self.temperature else 10,
                             N.r_n if solid_diffusion == "Fickian" else None)
        grids.check(g, thermal=self.temperature, sei=bool(aging))
        if grid_lib is None and g != grids.DEFAULT:
            if lib_path is not None:
                raise ValueError("a non-default discretisation with an explicit library path needs grid_lib= as well")
            vid = grids.variant_id({LCO: "LCO_LIC6", NMC: "NMC_LIC6", NMC_LGM50: "LGM50"}[cathode], bool(aging), self.temperature, {"f64": 0, "mixed": 1, "f64_reforder": 2}[precision],
                                   solid_diffusion.upper(), thermodynamic_factor.upper(), rxn, waves_per_cell == 2)
            if vid is None:
                raise NotImplementedError("this combination of model options is not instantiated on the device")
            # (a variant that failed the kernel self-test on this machine with the built-in flags -- under THIS flag table and these sources: the marker carries the build
            #  identity -- goes to its fall-back build directly, and grids.library keeps it out of every union library of the built-in flags: ADVICE r05)
            grid_lib = grids.library(g, [vid], machine_licm=True) if grids.needs_fallback(g, vid) else grids.library(g, [vid])
            self._grid_lib_built, self._grid_key = grid_lib, (g, vid)
        if grid_lib:                                     # (False: register nothing -- the tests' way to reach the C ABI's own refusal)
            cap.check(self._lib, self._lib.plh_register_grid_library(os.fsencode(grid_lib)), "plh_register_grid_library")
        h = C.c_void_p()
        cap.check(self._lib, self._lib.plh_model_create(C.byref(desc), C.byref(h)), "plh_model_create")
        self._h = h
        self.N.tot = self._lib.plh_n_states(h)
        self.N.diff = self._lib.plh_n_diff(h)
        self.N.alg = self.N.tot - self.N.diff
        self.lds_bytes = self._lib.plh_lds_bytes(h)            # LDS per cell of this variant
        self.save_start_dict = {}                              # p.cache.save_start_dict (src/structures.jl:305): opts.save_start
        self.θ_keys = [self._lib.plh_theta_key(h, i).decode("utf-8") for i in range(self._lib.plh_n_theta(h))]
        self.ind = {}                       # p.ind: state name -> slice into Y (reference state_indices, src/external.jl:275-365)
        for i in range(self._lib.plh_n_sections(h)):
            nm, a, ln = C.c_char_p(), C.c_int(), C.c_int()
            cap.check(self._lib, self._lib.plh_section(h, i, C.byref(nm), C.byref(a), C.byref(ln)), "plh_section")
            self.ind[nm.value.decode("utf-8")] = slice(a.value, a.value + ln.value)
        self.variant = "%s_%s%s%s%s%s" % (cathode.lower(), "thermal" if self.temperature else "iso", "_sei" if aging else "",          # matching oracle variant (tests)
                                          {"Fickian": "", "quadratic": "_quad", "polynomial": "_poly"}[solid_diffusion], "_nu" if thermodynamic_factor == "nonlinear" else "",
                                          "_mhc" if rxn == "MHC" else "")
        if g != grids.DEFAULT:
            self.variant += "_g%d_%d_%d_%d" % g[:4] + ("_%d_%d" % g[4:6] if self.temperature else "") + ("_rn%d" % g[6] if len(g) == 7 else "")

    theta = property(lambda self: self.θ)

    def compile_closures(self, protocol, n_cells=None, force=False, _emu_include=None, verify=True):
        """compile the input closures of `protocol` into device code and attach them to this model (closure_lib.py; hipcc, once per closure set, cached): later
        simulate_ensemble / simulate calls with the same closures run them compiled instead of interpreted; every other call is unaffected.  Returns the library path
        (None: the protocol has no closure input)."""
        from . import closure_lib
        runs, _ = make_protocol(self, protocol, n_cells)
        #  a closure library is compiled on the user's machine with the aggressive flag set of the built-in kernels, which this toolchain is known to miscompile now
        # and then (buildflags.py): it is VERIFIED before use -- compiled against interpreted on a short run of the same protocol, bit for bit (the contract of a compiled
        # closure) --, rebuilt ONCE with the conservative set when that fails, and dropped (interpreter) when that fails too.  A model whose grid library already needed the
        # conservative set starts there.
        licm = "_licm" in os.path.basename(getattr(self, "_grid_lib_built", None) or "")
        lib = closure_lib.library(self, runs, force=force, emu_include=_emu_include, machine_licm=licm)
        if not lib:
            return None
        for attempt in range(2):
            cap.check(self._lib, self._lib.plh_model_attach_closure_library(self._h, os.fsencode(lib)), "plh_model_attach_closure_library")
            self._closure_digest = closure_lib.digest(closure_lib.expr_runs(runs))
            why = self._verify_closure_library(protocol, lib) if verify else None
            if why is None:
                return lib
            if attempt == 0 and not licm:
                lib = closure_lib.library(self, runs, force=force, emu_include=_emu_include, machine_licm=True)
                licm = True
                continue
            break
        self._lib.plh_model_attach_closure_library(self._h, None)          # detach: the interpreter serves these closures
        self._closure_digest = None
        import warnings
        warnings.warn("compiled closures of this protocol do not reproduce the interpreter (%s): the library %s is not used" % (why, os.path.basename(lib)))
        return None

    def _verify_closure_library(self, protocol, lib):
        """None if a short run of `protocol` (every run cut to 30 s, 2 cells at SOC 0.5) through the attached library equals the interpreter's bit for bit, else what differs.  Verified
        libraries are remembered next to the file (<lib>.verified holds the build identity)."""
        mark = lib + ".verified"
        ident = build_info(self)
        if os.path.exists(mark) and open(mark).read() == ident:
            return None
        short = [dict(r, tf=min(float(r.get("tf", 30.0)), 30.0)) for r in protocol]
        Th = np.tile(self.theta_vector(), (2, 1))
        try:
            a = simulate_ensemble(self, Th, short, SOC=0.5)
            if not self._lib.plh_last_integrate_compiled(self._h):
                return "the attached library was not selected for its own protocol"
            self._lib.plh_model_attach_closure_library(self._h, None)
            try:
                b = simulate_ensemble(self, Th, short, SOC=0.5)
            finally:
                cap.check(self._lib, self._lib.plh_model_attach_closure_library(self._h, os.fsencode(lib)), "plh_model_attach_closure_library")
        except Exception as e:              # (a protocol that cannot run per-cell arrays cut to two cells, ...: nothing verified, nothing refused)
            return None if isinstance(e, (ValueError, TypeError)) else repr(e)
        if not np.array_equal(a.run_info["flag"], b.run_info["flag"]):
            return "exit flags %r, interpreted %r" % (a.run_info["flag"].tolist(), b.run_info["flag"].tolist())
        if not (np.array_equal(np.asarray(a.Y), np.asarray(b.Y)) and np.array_equal(a.run_info["t_end"], b.run_info["t_end"])):
            return "end states differ by %.1e" % float(np.abs(np.asarray(a.Y) - np.asarray(b.Y)).max())
        try:
            open(mark, "w").write(ident)
        except OSError:
            pass
        return None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.plh_model_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def theta_vector(self, overrides=None):
        """dense θ_tot in θ_keys order (update_θ!, src/generate_functions.jl:364-372)."""
        th = dict(self.θ)
        if overrides:
            th.update(overrides)
        return np.array([th[k] for k in self.θ_keys], dtype=np.float64)

    def jac_pattern(self, mode=cap.MODE_I):
        nnz = C.c_int(0)
        cap.check(self._lib, self._lib.plh_jac_pattern(self._h, mode, C.byref(nnz), None, None), "plh_jac_pattern")
        cp = np.zeros(self.N.tot + 1, dtype=np.int32)
        ri = np.zeros(nnz.value, dtype=np.int32)
        cap.check(self._lib, self._lib.plh_jac_pattern(self._h, mode, C.byref(nnz), cp.ctypes.data, ri.ctypes.data), "plh_jac_pattern")
        return cp, ri


def petlion(cathode=LCO, *, N_p=10, N_s=10, N_n=10, N_a=10, N_z=10, N_r_p=10, N_r_n=10, temperature=None,
            solid_diffusion="Fickian", Fickian_method="finite_difference", aging=False, jacobian="symbolic", SOC=1.0,
            thermodynamic_factor="linear", rxn_p="BV", rxn_n="BV", precision="f64", device=-1, waves_per_cell=1, _lib_path=None, _grid_lib=None):
    """petlion(cathode; kwargs...) -- reference src/params.jl:119-174.  `jacobian` is accepted and ignored (the device
    Jacobian is hand-derived); unsupported structural options raise."""
    if temperature is None:
        temperature = cathode == NMC_LGM50       # the reference's defaults: system_LGM50_NMC_LiC6 has temperature = true (src/params.jl:695), LCO / NMC false (139, 389)
    if solid_diffusion not in ("Fickian", "quadratic", "polynomial") or (solid_diffusion == "Fickian" and Fickian_method != "finite_difference"):
        raise NotImplementedError("solid diffusion: Fickian (finite_difference), quadratic and polynomial are built; the BETA spectral method is not (SURVEY.md 8f)")
    if thermodynamic_factor not in ("linear", "nonlinear") or rxn_p not in ("BV", "MHC") or rxn_n != rxn_p:
        raise NotImplementedError("thermodynamic_factor: linear / nonlinear; rxn_p = rxn_n in (BV, MHC)")
    mk = lambda: Model(cathode, _N(p=N_p, s=N_s, n=N_n, a=N_a, z=N_z, r_p=N_r_p, r_n=N_r_n), temperature, aging, _lib_path, precision, device, solid_diffusion, thermodynamic_factor, rxn_p, waves_per_cell, _grid_lib)
    p = mk()
    p.opts.SOC = SOC
    try:
        _selftest_new_grid_library(p)
    except RuntimeError as err:
        # a grid library compiled here with the built-in flags (buildflags.py) failed the kernel self-test: ONE rebuild with MachineLICM on -- the flag set every grid library of
        # r04 passed under -- is registered after it (the latest registration wins in plh_model_create) and checked the same way; the marker makes later processes go there directly
        import warnings
        lib = getattr(p, "_grid_lib_built", None)
        if not lib or lib.endswith("_licm.so"):
            raise
        warnings.warn("petlion.jl_amd: %s -- rebuilding %s with MachineLICM on (fall-back flags)" % (err, os.path.basename(lib)), RuntimeWarning)
        grids.mark_fallback(*p._grid_key, err)
        p = mk()
        p.opts.SOC = SOC
        _selftest_new_grid_library(p)
    _selftest_unvalidated_build(p)
    return p


def selftest(p, n_cells=2, tf=100.0):
    """Power-on check of the kernels of ONE model variant: every k_integrate instantiation (plain / stop times / table / closure / general control row / refinement,
    csrc/dfn_integrate.h GenFlag) runs the same 1C discharge and must reproduce the plain kernel -- flags and end times equal, SOC (exact for a constant current) to 1e-11,
    the first saved SOC equal to SOC0, voltage to 1e-9 where the input is the same number.  Raises RuntimeError naming the instantiation.  It exists because a kernel of this size
    sits at the register allocator's limits: one build was seen to start a run with a garbage SOC accumulator in one instantiation only; the built-in variants
    are checked by the GPU test suite, a grid library compiled on the user's machine at first use is checked here."""
    Th = np.tile(p.theta_vector(), (n_cells, 1))
    ps = p.ind["Φ_s"]
    base = simulate_ensemble(p, Th, [{"I": -1.0, "tf": tf}], SOC=1.0)
    o_stop, o_ref = Opts(), Opts()
    o_stop.tstops = [1e7]; o_ref.refine = 1
    cases = [("stop times", [{"I": -1.0, "tf": tf}], o_stop, 1e-12), ("table input", [{"I": ([0.0, 1e7], [-1.0, -1.0]), "tf": tf}], None, 1e-9),
             ("closure input", [{"I": lambda t: -1.0 + 0.0 * t, "tf": tf}], None, 1e-9),
             ("general control row", [{"I": lambda t, Y, q: -1.0 + 1e-12 * (Y[ps.start] - Y[ps.stop - 1]), "tf": tf}], None, 2e-3), ("refinement", [{"I": -1.0, "tf": tf}], o_ref, 2e-3)]
    bad = None
    if not ((base.run_info["flag"][:, 0] == 0).all() and np.abs(base.run_info["SOC"][:, 0] - (1.0 - tf / 3600.0)).max() < 1e-11 and np.abs(base.SOC[:, 0] - 1.0).max() == 0.0):
        bad = "plain"
    if not bad:
        # every comparison below is against the PLAIN kernel of the same build: a wrong plain kernel would pass them all.  Known answer first.
        why = known_answer_check(p)
        if why:
            raise RuntimeError("kernel self-test failed: the plain kernel of %s does not reproduce the known answer of the validated binary (%s) -- a miscompiled or modified build "
                               "(DESIGN.md 5a)" % (p.variant, why))
    for name, proto, o, vtol in cases:
        if bad:
            break
        e = simulate_ensemble(p, Th, proto, SOC=1.0, opts=o)
        if not (np.array_equal(e.run_info["flag"], base.run_info["flag"]) and np.abs(e.run_info["t_end"] - base.run_info["t_end"]).max() == 0.0
                and np.abs(e.run_info["SOC"] - base.run_info["SOC"]).max() < 1e-11 and np.abs(e.run_info["V"] - base.run_info["V"]).max() <= vtol and np.abs(e.SOC[:, 0] - 1.0).max() == 0.0):
            bad = name
    if not bad:
        # the continuation path (a second run inherits SOC, time, V / I from the first: the path of the miscompile that was seen) in the plain and the table instantiation,
        # and the sensitivity instantiation, whose states must be those of the plain kernel bit for bit
        two = [{"I": -1.0, "tf": tf / 2}, {"I": -1.0, "tf": tf / 2}]
        two_tab = [{"I": -1.0, "tf": tf / 2}, {"I": ([0.0, 1e7], [-1.0, -1.0]), "tf": tf / 2}]
        for name, proto in (("plain, two runs", two), ("table input, two runs", two_tab)):
            e = simulate_ensemble(p, Th, proto, SOC=1.0)
            if not ((e.run_info["flag"] == 0).all() and np.abs(e.run_info["SOC"][:, 1] - (1.0 - tf / 3600.0)).max() < 1e-11 and np.abs(e.run_info["t_end"][:, 1] - tf).max() < 1e-9
                    and np.abs(e.run_info["V"][:, 1] - base.run_info["V"][:, 0]).max() <= 2e-3):
                bad = name
                break
    if not bad and p.waves_per_cell != 2:
        # (compared like the other instantiations -- flags and end times equal, SOC to 1e-11, voltage and states within the tolerance the run was made at: the sensitivity kernel
        #  is another compilation of the step loop, and on a build other than the validated one its sums may be contracted differently; bit-identity is what the validated
        #  binary shows, tests/test_sensitivities.py, not what a correct build must show)
        e = simulate_ensemble(p, Th, [{"I": -1.0, "tf": tf}], SOC=1.0, sens=[p.θ_keys[0]])
        scale = np.abs(base.Y).max(axis=0) + 1e-300
        if not (np.array_equal(e.run_info["flag"], base.run_info["flag"]) and np.abs(e.run_info["t_end"] - base.run_info["t_end"]).max() == 0.0
                and np.array_equal(e.counters["n_steps"], base.counters["n_steps"]) and np.array_equal(e.counters["n_newton"], base.counters["n_newton"])
                and np.abs(e.run_info["SOC"] - base.run_info["SOC"]).max() < 1e-11 and np.abs(e.run_info["V"] - base.run_info["V"]).max() <= 1e-8
                and (np.abs(e.Y - base.Y) / scale).max() <= 1e-8 and (np.asarray(e.sens_stat)[:, 1] == 0).all()):          # (the header's guarantee -- same steps, states to ~1e-9 -- held to 1e-8, not to 10 x reltol)
            bad = "sensitivity"
    if bad:
        raise RuntimeError("kernel self-test failed: the %s instantiation of %s does not reproduce the plain kernel on a 1C discharge -- a miscompiled build "
                           "(rebuild; see DESIGN.md 5a)" % (bad, p.variant))


_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "selftest_golden.json")
KA_TOL = 2e-6        # 200 x the reltol of the known-answer protocol: two correct builds (other compiler, other contraction of a sum) agree to ~1e-7 there (tests/test_gpu_tight.py)
KA_ATOL = 1e-9       # 10 x the abstol of the known-answer protocol: the absolute floor of a state-section comparison (known_answer_check)


def known_answer_protocol(p):
    """the fixed protocol of the kernel self-test's known answer: 2 cells (default theta; D_sp x 1.3, k_n x 0.8), 3 runs (1C discharge 100 s, V hold 50 s, rest 50 s) at reltol
    1e-8 / abstol 1e-10 -- tight, so that the result does not depend on the last bits of the step selection (at the default tolerances two correct builds differ by 1e-6)"""
    Th = np.tile(p.theta_vector(), (2, 1))
    Th[1, p.θ_keys.index("D_sp")] *= 1.3
    Th[1, p.θ_keys.index("k_n")] *= 0.8
    o = Opts()
    o.reltol, o.abstol, o.reltol_init, o.abstol_init, o.maxiters = 1e-8, 1e-10, 1e-8, 1e-10, 100000
    return Th, [{"I": -1.0, "tf": 100.0}, {"V": "hold", "tf": 50.0}, {"I": "rest", "tf": 50.0}], o


def known_answer_digest(p):
    """what is compared: per run (t_end, V, I, SOC), per state section of the end state (max |Y|, sum Y)"""
    Th, proto, o = known_answer_protocol(p)
    e = simulate_ensemble(p, Th, proto, SOC=1.0, opts=o, max_points=20000)
    d = {"flags": e.run_info["flag"].tolist(), "t_end": e.run_info["t_end"].tolist(), "V": e.run_info["V"].tolist(), "I": e.run_info["I"].tolist(), "SOC": e.run_info["SOC"].tolist(),
         "sections": {nm: [[float(np.abs(e.Y[c, sl]).max()), float(e.Y[c, sl].sum())] for c in range(2)] for nm, sl in p.ind.items()}}
    return d


def _golden_key(p):
    return "%s|%s" % (p.variant, p.precision)


def known_answer_check(p):
    """None if the plain kernel reproduces the committed known answer of this variant / grid (selftest_golden.json: produced by tools/make_selftest_golden.py on the binary that
    profiles/validated_build.json names), else a description of the first disagreement.  A discretisation without a committed answer (a grid library for a grid of the user's
    own) is checked against the built-in default-grid kernel of the same model instead -- two discretisations of the same cell agree to their truncation error, which catches a
    broken equation, not a last-digit one."""
    import json
    try:
        gold = json.load(open(_GOLDEN))["digests"]
    except (OSError, ValueError, KeyError):
        gold = {}
    g = gold.get(_golden_key(p))
    d = known_answer_digest(p)
    if g is None:
        return _cross_grid_check(p, d)
    if d["flags"] != g["flags"]:
        return "exit flags %r, known %r" % (d["flags"], g["flags"])
    for k in ("t_end", "V", "I", "SOC"):
        a, b = np.asarray(d[k]), np.asarray(g[k])
        if not np.all(np.abs(a - b) <= KA_TOL * np.maximum(1.0, np.abs(b))):
            return "%s of the runs %r, known %r" % (k, a.tolist(), b.tolist())
    for nm, rows in g["sections"].items():
        for c in range(2):
            mx, sm = d["sections"][nm][c]
            gmx, gsm = rows[c]
            n = p.ind[nm].stop - p.ind[nm].start
            # (absolute floor: ten times the ABSOLUTE tolerance the protocol is integrated with -- a field that has relaxed to ~1e-5 of its scale, Phi_e at the end of the rest, is
            #  only determined to abstol, and two correct builds whose step sequences differ in one step differ there by that much: r06, 1.1e-10 in max |Phi_e| = 2.08e-5 V)
            if abs(mx - gmx) > KA_TOL * max(gmx, 1e-300) + KA_ATOL or abs(sm - gsm) > KA_TOL * n * max(gmx, 1e-300) + n * KA_ATOL:
                return "state section %s of cell %d: max |Y| %.12g (known %.12g), sum %.12g (known %.12g)" % (nm, c, mx, gmx, sm, gsm)
    return None


def _cross_grid_check(p, d):
    """no committed answer for this discretisation: the same model on the built-in default grid (whose own answer IS committed) must give the same cell voltage, current and
    SOC at the run ends to the truncation error of a coarse grid"""
    if getattr(p, "_lib_path", None) is not None or not getattr(p, "_grid_lib_built", None):
        return None
    try:
        ref = Model(p.cathode, _N(p=10, s=10, n=10, a=10, z=10, r_p=10, r_n=10), p.temperature, p.aging, None, p.precision, -1, p.solid_diffusion, p.thermodynamic_factor, p.rxn, p.waves_per_cell, None)
    except Exception:
        return None
    g = known_answer_digest(ref)
    if d["flags"] != g["flags"]:
        return "exit flags %r, default grid %r" % (d["flags"], g["flags"])
    # (a coarse grid -- 2 control volumes per section -- is tens of mV from the default one: this catches a broken equation, not a discretisation)
    if np.abs(np.asarray(d["V"]) - np.asarray(g["V"])).max() > 0.15 or np.abs(np.asarray(d["SOC"]) - np.asarray(g["SOC"])).max() > 5e-3 or np.abs(np.asarray(d["t_end"]) - np.asarray(g["t_end"])).max() > 1e-6:
        return "run-end V / SOC / t_end %r / %r / %r, default grid %r / %r / %r" % (d["V"], d["SOC"], d["t_end"], g["V"], g["SOC"], g["t_end"])
    return None


def _gpu_visible(p):
    """the library's own device count (no second GPU runtime in the process, no dependence on torch)"""
    try:
        return p._lib.plh_device_count() > 0
    except AttributeError:
        return False


def _guarded_selftest(p, marker, identity, what):
    """run selftest(p) once per (marker file, identity string); warn -- never skip silently -- when no GPU is visible"""
    import warnings
    try:
        if os.path.exists(marker) and open(marker).read().strip() == identity:
            return
    except OSError:
        pass
    if not _gpu_visible(p):
        warnings.warn("petlion.jl_amd: kernel self-test of %s skipped (no GPU visible to the library); it runs on the first machine with a GPU" % what, RuntimeWarning)
        return
    selftest(p)
    try:
        with open(marker, "w") as f:
            f.write(identity + "\n")
    except OSError:
        pass


def _selftest_new_grid_library(p):
    """a grid library compiled at first use (petlion.jl_amd/grids.py) is checked once per (library, variant, compiler / host build identity) on the first machine with a GPU
    that loads it (a cache copied from another machine carries the identity it was checked under; a different compiler or host library checks again)"""
    lib = getattr(p, "_grid_lib_built", None)
    if not lib:
        return
    _guarded_selftest(p, "%s.%s.selftest" % (lib, p.variant), build_info(p), "the grid library %s" % os.path.basename(lib))


def build_info(p=None):
    """plh_build_info(): compiler versions, flag hash and source hash of the loaded library"""
    lib = p._lib if p is not None else cap.load()
    try:
        return lib.plh_build_info().decode("utf-8", "replace")
    except AttributeError:
        return "unknown"


_VALIDATED = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "validated_build.json")


def _selftest_unvalidated_build(p):
    """the built-in kernels are validated by the GPU test suite, and profiles/validated_build.json records the identity of the binary that run validated.  A
    library whose plh_build_info() differs -- another hipcc, other flags, edited sources -- has not been through that run: the first petlion() of each variant then runs the
    kernel self-test (every k_integrate instantiation against the plain one, including a two-run continuation) once per build and machine."""
    if not getattr(p, "_builtin_lib", False) or getattr(p, "_grid_lib_built", None):
        return
    info = build_info(p)
    try:
        import json
        if json.load(open(_VALIDATED)).get("build_info") == info:
            return
    except (OSError, ValueError):
        pass
    _guarded_selftest(p, "%s.%s.selftest" % (cap.LIB_PATH, p.variant), info, "this build of libpetlion_hip.so (%s: not the validated binary)" % info)


# ---------------------------------------------------------------------------------------------------------------------
_INPUTS = ("I", "V", "dT", "P", "η_p", "res") + tuple(cap.DSTATE)
_MODE = {"I": cap.MODE_I, "V": cap.MODE_V, "dT": cap.MODE_DT, "P": cap.MODE_P, "η_p": cap.MODE_ETA_P, "res": cap.MODE_RES}
_MODE.update({k: cap.MODE_DSTATE for k in cap.DSTATE})       # dc_s_p_max, ..., dc_e_min (input_methods.jl:190-247): the rate of one differential state, chosen per cell at the start of the run
_BOUND_KW = Bounds.FIELDS


def _make_run(p, name, inp, tf, bounds):
    r = cap.Run()
    r.mode = _MODE[name]
    res_x = 0.0
    if name in cap.DSTATE:
        r.dstate = cap.DSTATE[name]
        if callable(inp) or isinstance(inp, (tuple, list)):
            raise ValueError("%s takes a number or :hold" % name)
    if name == "res":
        # user-defined control residual (reference input_methods.jl:155-175, custom_res!, model_evaluation.jl:155-172): res = f  ->  0 - f = 0;  res = (x, f)  ->  x - f = 0
        if isinstance(inp, (tuple, list)) and len(inp) == 2 and callable(inp[1]) and not callable(inp[0]):
            res_x, inp = float(inp[0]), inp[1]
        if not callable(inp):
            raise ValueError("res = f or res = (x, f) with a closure f(t, Y, p)")
    if isinstance(inp, str):
        if inp == "hold":
            r.value_kind, r.value = cap.VAL_HOLD, 0.0
        elif inp == "rest":
            if name not in ("I", "P"):
                raise ValueError("Unsupported input symbol.")       # input_methods.jl:24,97
            r.value_kind, r.value = cap.VAL_REST, 0.0
        else:
            raise ValueError("Unsupported input symbol.")
    elif callable(inp):
        # a closure cannot cross the C ABI, its expression can: traced once into a postfix program (closures.py; PLH_VAL_EXPR).  A closure that branches on t or Y in Python
        # cannot be traced (closures.TraceError says how to rewrite it); a piecewise-linear table (t, values) + opts.tdiscon remains the other way in.
        if name == "dT":
            raise ValueError("function inputs for dT are not defined by the reference")
        (ops, args), tree = closures.trace(inp, p, with_tree=True)
        r.value_kind, r.value = cap.VAL_EXPR, 0.0
        r.n_tab = ops.size
        # a closure of Y: the entries d f / d Y[c] of the control row, as the reference's symbolic differentiation builds them (scalar_residual.jl:276-416); the programs ride
        # behind the main one in the same arrays (plh_run.dcol / dofs)
        der = closures.row_derivatives(tree, p.N.tot, p.N.diff)
        keep = []
        if der is not None:
            dcol = np.ascontiguousarray(der[0], dtype=np.int32)
            dofs = np.ascontiguousarray(np.cumsum([ops.size] + [q[0].size for q in der[1]]), dtype=np.int32)
            ops = np.concatenate([ops] + [q[0] for q in der[1]]); args = np.concatenate([args] + [q[1] for q in der[1]])
            r.n_dcol = dcol.size
            r.dcol = dcol.ctypes.data_as(C.POINTER(C.c_int)); r.dofs = dofs.ctypes.data_as(C.POINTER(C.c_int))
            keep = [dcol, dofs]
        r.tab_t = ops.ctypes.data_as(C.POINTER(C.c_double)); r.tab_v = args.ctypes.data_as(C.POINTER(C.c_double))
        r._keep = (ops, args, *keep)
        if name == "res":
            if der is None:
                raise ValueError("res: the closure must read the state (Y, or YP of differential states)")
            r.value = res_x
    elif isinstance(inp, (tuple, list)) and len(inp) == 2 and np.ndim(inp[0]) == 1:
        if name == "dT":
            raise ValueError("time-dependent dT inputs are not defined by the reference")
        tt = np.ascontiguousarray(inp[0], dtype=np.float64); vv = np.ascontiguousarray(inp[1], dtype=np.float64)
        if tt.shape != vv.shape or tt.size < 1 or (np.diff(tt) < 0).any():
            raise ValueError("table input: (t, v) arrays of equal length with non-decreasing times")
        r.value_kind, r.value = cap.VAL_TABLE, float(vv[0])
        r.n_tab = tt.size
        r.tab_t = tt.ctypes.data_as(C.POINTER(C.c_double)); r.tab_v = vv.ctypes.data_as(C.POINTER(C.c_double))
        r._keep = (tt, vv)                              # keep the arrays alive as long as the run descriptor
    elif isinstance(inp, np.ndarray) and inp.ndim == 1:                       # one constant input per cell (ensemble axis of the protocol)
        vv = np.ascontiguousarray(inp, dtype=np.float64)
        r.value_kind, r.value = cap.VAL_CONST, float(vv[0])
        r.value_cell = vv.ctypes.data_as(C.POINTER(C.c_double))
        r._keep = (vv,)
    else:
        r.value_kind, r.value = cap.VAL_CONST, float(inp)
    if isinstance(tf, np.ndarray):                                            # one run length per cell
        tt_ = np.ascontiguousarray(tf, dtype=np.float64)
        r.tf = float(tt_[0]); r.tf_cell = tt_.ctypes.data_as(C.POINTER(C.c_double)); r._keep_tf = tt_
    else:
        r.tf = float(tf)
    for f in cap.BOUND_FIELDS:
        setattr(r.bounds, f, getattr(bounds, "η_plating_min" if f == "eta_plating_min" else f))
    return r


def _opts_struct(o, p=None):
    s = cap.Opts(o.abstol, o.reltol, o.abstol if o.abstol_init is None else o.abstol_init,
                 o.reltol if o.reltol_init is None else o.reltol_init, int(o.maxiters), int(bool(o.check_bounds)),
                 int(bool(o.interp_final)), int(o.max_order), int(bool(o.jac_every_step)), float(o.init_step))
    td = np.ascontiguousarray(list(getattr(o, "tdiscon", []) or []), dtype=np.float64)
    s.n_tdiscon = td.size
    s.tdiscon = td.ctypes.data_as(C.POINTER(C.c_double)) if td.size else None
    s.refine = int(getattr(o, "refine", 0))
    ts = np.ascontiguousarray(list(getattr(o, "tstops", []) or []), dtype=np.float64)      # opts.tstops (run-local times; model_evaluation.jl:292-294)
    s.n_tstops = ts.size
    s.tstops = ts.ctypes.data_as(C.POINTER(C.c_double)) if ts.size else None
    s._keep = (td, ts)                               # the arrays must outlive the struct
    s.yp_alg_zero = int(bool(getattr(o, "yp_alg_zero", False)))
    # opts.stop_function (src/structures.jl:283, src/checks.jl:26): a closure g(t, Y, YP, p) traced into a postfix program like an input closure (closures.py); the run ends
    # when g > 0, exit flag 12, with the same linear back-interpolation as the built-in bounds (plh_opts.stop_ops)
    sf = getattr(o, "stop_function", None)
    s.n_stop, s.stop_ops, s.stop_args = 0, None, None
    if sf is not None:
        if p is None:
            raise ValueError("opts.stop_function needs the model it is traced for")
        ops, args = sf if isinstance(sf, tuple) else closures.trace(sf, p)
        ops, args = np.ascontiguousarray(ops, dtype=np.float64), np.ascontiguousarray(args, dtype=np.float64)
        s.n_stop = ops.size
        s.stop_ops, s.stop_args = ops.ctypes.data_as(C.POINTER(C.c_double)), args.ctypes.data_as(C.POINTER(C.c_double))
        s._keep = s._keep + (ops, args)
    return s


class RunResult:
    def __init__(self, name, tspan, flag, iterations, info):
        self.name = name
        self.tspan = tspan
        self.flag = int(flag)
        self.exit_reason = EXIT_REASONS.get(int(flag), "error %d" % flag)
        self.iterations = int(iterations)
        self.info = info


class Solution:
    """reference `solution` (src/outputs.jl:78-105), for the outputs the device records per step."""

    def __init__(self):
        self.t = np.zeros(0)
        self.V = np.zeros(0)
        self.I = np.zeros(0)
        self.SOC = np.zeros(0)
        self.P = np.zeros(0)
        self.Y = None          # last state vector (sol.Y[end])
        self.YP = None
        self.T_avg = None      # [points] with temperature = true
        self.Y_all = None      # [points, N] when the run was made with outputs = "all" / a state name (sol.Y of the reference)
        self.Y_sel = None      # [points, n_sel_total] when the run was made with sections = (...): only the selected state entries, packed in the order given
        self._sel = None       # the selection as ((start, len), ...) and each of its keys as a slice into a row of Y_sel
        self._sel_ind = None
        self._ind = None
        self.results = []
        self.counters = None

    def __len__(self):
        return len(self.t)

    def __getattr__(self, name):
        # sol.c_e, sol.T, sol.j, sol.Φ_e ... : per-step state sections, available when the states were kept (outputs = "all")
        ind = self.__dict__.get("_ind")
        if ind and name in ind:
            if self.__dict__.get("Y_all") is None:
                sel_ind = self.__dict__.get("_sel_ind")
                if sel_ind and name in sel_ind and self.__dict__.get("Y_sel") is not None:      # saved as a selected section (sections = (name, ...))
                    return self.Y_sel[:, sel_ind[name]]
                raise AttributeError("%s was not saved: run with sections=(%r,) or outputs='all'" % (name, name))
            return self.Y_all[:, ind[name]]
        raise AttributeError(name)

    def isempty(self):
        return len(self.results) == 0

    def __call__(self, t, interp_bc="interpolate", k=3):
        """sol(t): the reference's post-interpolation of a solution (src/save_outputs.jl:74-133).  Every requested time is assigned to the run whose
        tspan contains it (first match; before the first run -> run 1, otherwise the last run), each run's saved points get an interpolating spline
        of degree min(k, points) -- Dierckx `Spline1D(t, x; k, bc)` with s = 0, i.e. FITPACK curfit/splev, which is exactly what
        scipy.interpolate.splrep/splev call -- evaluated with bc = "nearest" (interp_bc = "interpolate") or "extrapolate"."""
        from scipy.interpolate import splev, splrep
        if interp_bc not in ("interpolate", "extrapolate"):
            raise ValueError("Invalid interp_bc method.")
        tq = np.atleast_1d(np.asarray(t, dtype=np.float64))
        spans = [r.tspan for r in self.results]
        which = np.full(tq.shape, len(spans) - 1)
        for q, tv in enumerate(tq):
            if tv < spans[0][0]:
                which[q] = 0
                continue
            for i, (a, b) in enumerate(spans):
                if a <= tv <= b:
                    which[q] = i
                    break
        out = Solution()
        out.t = tq
        out.results = [self.results[i] for i in sorted(set(which.tolist()))]
        out.Y, out.YP, out.counters = self.Y, self.YP, self.counters
        out._ind, out._sel, out._sel_ind = self._ind, self._sel, self._sel_ind
        start = np.concatenate([[0], np.cumsum([r.iterations for r in self.results])])
        names = ["V", "I", "SOC", "P"] + (["T_avg"] if self.T_avg is not None else []) + (["Y_all"] if self.Y_all is not None else []) + (["Y_sel"] if self.Y_sel is not None else [])
        for name in names:
            x = getattr(self, name)
            y = np.zeros(tq.shape + x.shape[1:])
            for i in set(which.tolist()):
                pts = slice(int(start[i]), int(start[i + 1]))
                n = int(start[i + 1] - start[i])
                kk = min(k, n)
                if kk >= n:
                    kk = max(1, n - 1)          # FITPACK needs more points than the degree
                sel = which == i
                if n < 2:
                    y[sel] = x[pts][0]
                    continue
                ext = 3 if interp_bc == "interpolate" else 0
                if x.ndim == 1:
                    y[sel] = splev(tq[sel], splrep(self.t[pts], x[pts], k=kk, s=0), ext=ext)
                else:                           # VectorOfArray fields: one spline per state (save_outputs.jl:104-119)
                    for c in range(x.shape[1]):
                        y[sel, c] = splev(tq[sel], splrep(self.t[pts], x[pts, c], k=kk, s=0), ext=ext)
            setattr(out, name, y)
        return out

    def __repr__(self):
        if self.isempty():
            return "PETLION simulation (empty)"
        r = self.results[-1]
        runs = " → ".join(x.name for x in self.results)
        return ("PETLION simulation\n  --------\n  Runs:    %s\n  Time:    %.2f s\n  Current: %.4gC\n  Voltage: %.4f V\n"
                "  Power:   %.4f W/m²\n  SOC:     %.4f\n  Exit:    %s" % (runs, self.t[-1], self.I[-1], self.V[-1], self.P[-1], self.SOC[-1], r.exit_reason))


def exit_reasons(sol):
    return [r.exit_reason for r in sol.results]


def final_exit_reason(sol):
    return sol.results[-1].exit_reason


def _split_kwargs(p, kw):
    inputs = {k: kw.pop(k) for k in list(kw) if k in _INPUTS}
    if len(inputs) != 1:
        raise ValueError("exactly one input (I, V or dT) must be selected")     # check_input_arguments, checks.jl:270-282
    bounds = p.bounds.copy(**{k: kw.pop(k) for k in list(kw) if k in _BOUND_KW})
    return inputs, bounds, kw


_STATE_OUTPUTS = ("Y", "c_e", "c_s_avg", "T", "film", "SOH", "j", "j_s", "Φ_e", "Φ_s")


def _wants_states(p, outputs):
    """outputs = :all or any per-node state asks for the state vector of every step (solution_states_logic, src/outputs.jl:107-131)."""
    outs = (outputs,) if isinstance(outputs, str) else tuple(outputs or ())
    return "all" in outs or any(x in _STATE_OUTPUTS for x in outs)


def _resolve_sections(p, sections):
    """sections = names of p.ind and / or (start, len) pairs -> (the selection as a tuple of (start, len), {key: slice into the packed row of Y_sel}); the order given is kept.
    Only the spelling is checked here: bounds, overlaps and the number of ranges are the library's to refuse (plh_outputs.sel)."""
    if sections is None:
        return None, None
    items = (sections,) if isinstance(sections, str) else tuple(sections)
    if len(items) == 2 and all(isinstance(x, (int, np.integer)) for x in items):
        items = (items,)                                               # one bare (start, len) pair
    if not items:
        raise ValueError("sections: name at least one state section or (start, len) range")
    sel, sel_ind, off = [], {}, 0
    for x in items:
        if isinstance(x, str):
            if x not in p.ind:
                raise ValueError("sections: %r is not a state section of this model (%s)" % (x, ", ".join(p.ind)))
            a, ln = p.ind[x].start, p.ind[x].stop - p.ind[x].start
        else:
            a, ln = (int(v) for v in x)
            x = (a, ln)
        if x in sel_ind:
            raise ValueError("sections: %r is named twice" % (x,))
        sel.append((a, ln))
        sel_ind[x] = slice(off, off + ln)
        off += ln
    return tuple(sel), sel_ind


def calc_SOC(p, Y):
    """calc_SOC(Y, p) (reference src/physics_equations/scalar_residual.jl:95-102): the anode's mean c_s_avg as a fraction of its stoichiometry window"""
    Y = np.asarray(Y, dtype=np.float64)
    cs = p.ind["c_s_avg"]
    n_p = p.N.p * p.N.r_p if p.solid_diffusion == "Fickian" else p.N.p
    return (Y[..., cs.start + n_p:cs.stop].mean(axis=-1) / p.θ["c_max_n"] - p.θ["θ_min_n"]) / (p.θ["θ_max_n"] - p.θ["θ_min_n"])


def simulate(p, tf=1e6, *, sol=None, SOC=None, initial_states=None, sections=None, **kw):
    """simulate(p, tf; I=..|V=..|dT=.., SOC, abstol, reltol, ..., V_max, V_min, ...) for ONE cell (n_cells = 1 ensemble).
    sections = ("c_e", "T", (start, len), ...): keep only these entries of the state vector per saved point (sol.Y_sel, sol.c_e, sol(t).c_e) instead of the whole vector that
    outputs = "all" keeps; a continued solution keeps its selection, and continuing it with another one is refused.
    initial_states = Y (reference src/model_evaluation.jl:15, 102-110, 193-199): a new solution that starts from this state vector instead of initial_guess!; its SOC is
    calc_SOC(Y)."""
    inputs, bounds, rest = _split_kwargs(p, kw)
    if initial_states is not None:
        if sol is not None and not sol.isempty():
            raise ValueError("Cannot set `initial_states` and continue a previous run.")         # model_evaluation.jl:105-108
        initial_states = np.ascontiguousarray(initial_states, dtype=np.float64)
        if initial_states.shape != (p.N.tot,):
            raise ValueError("initial_states must have length N.tot")
    o = Opts()
    o.__dict__.update(p.opts.__dict__)
    for k, v in rest.items():
        if not hasattr(o, k):
            raise TypeError("unknown keyword %r" % k)
        setattr(o, k, v)
    (name, inp), = inputs.items()
    # simulate(p, tf::Vector): run to tf[end], then post-interpolate onto tf (model_evaluation.jl:79-80, 148-149)
    tf_interp = None
    if isinstance(tf, (list, tuple, np.ndarray)):
        tf_interp = np.asarray(tf, dtype=np.float64)
        if tf_interp.ndim != 1 or tf_interp.size == 0:
            raise ValueError("tf must be a number or a non-empty vector of times")
        tf = float(tf_interp[-1])
    new = sol is None or sol.isempty()
    sol = Solution() if sol is None else sol
    keep_Y = _wants_states(p, o.outputs) or sol.Y_all is not None
    sel, sel_ind = _resolve_sections(p, sections)
    if not new:
        if sections is not None and sel != sol._sel:
            raise ValueError("the solution being continued was saved with sections=%r: a continuation keeps that selection" % (sol._sel,))
        sel, sel_ind = sol._sel, sol._sel_ind
    soc0 = (p.opts.SOC if SOC is None else SOC) if new else sol.SOC[-1]
    if initial_states is not None:
        soc0 = float(calc_SOC(p, initial_states))                      # (starting_from_initial_state: the estimated SOC, model_evaluation.jl:197-199)
    # opts.save_start (src/structures.jl:281, model_evaluation.jl:384-411): the algebraic states a consistent initialisation ended with, kept per (method, SOC rounded to 4
    # digits, input value rounded to 4 digits) in the model's cache and used as the first guess of the next initialisation with the same key.  The reference looks the key up for
    # every run; here it is the warm start of a NEW solution with a numeric input (a continued run already starts from the previous run's states).
    ss_key, ss_hit = None, False
    if getattr(o, "save_start", False) and new and initial_states is None and isinstance(inp, (int, float)) and not isinstance(inp, bool):
        ss_key = (name, round(float(soc0), 4), round(float(inp), 4))
        ss_hit = ss_key in p.save_start_dict
        if ss_hit:
            th1 = p.theta_vector()[None, :]
            Y0 = np.zeros((1, p.N.tot)); s1 = np.array([float(soc0)])
            cap.check(p._lib, p._lib.plh_initial_guess(p._h, 1, th1.ctypes.data, s1.ctypes.data, Y0.ctypes.data, cap.PLH_HOST, None), "plh_initial_guess")
            Y0[0, p.N.diff:] = p.save_start_dict[ss_key]
            initial_states = Y0[0]
    want_Y0 = ss_key is not None and not ss_hit                        # (a miss: the initialised algebraic states are the first saved state vector)
    ens = _integrate(p, p.theta_vector()[None, :], np.array([soc0]), [_make_run(p, name, inp, tf, bounds)], o,
                     Y_init=(None if initial_states is None else initial_states[None, :]) if new else sol.Y[None, :], t_init=None if new else np.array([sol.t[-1]]), keep_Y=keep_Y or want_Y0, sections=sel)
    if want_Y0 and int(ens["run_info"][0, 0]["flag"]) >= 0:
        p.save_start_dict[ss_key] = ens["Y_all"][0, 0, p.N.diff:].copy()
    n = int(ens["n_pts"][0])
    ri = ens["run_info"][0, 0]
    if ri["flag"] < 0:                                                # the reference's error() paths: `sol` is left untouched
        raise RuntimeError(EXIT_REASONS.get(int(ri["flag"]), "error"))
    I1C = calc_I1C(p.θ)
    for fld in ("t", "V", "I", "SOC"):
        setattr(sol, fld, np.concatenate([getattr(sol, fld), ens[fld][0, :n]]))
    sol.P = sol.I * I1C * sol.V                                   # calc_P, scalar_residual.jl:87
    sol._ind = p.ind
    if "T_avg" in ens:
        sol.T_avg = np.concatenate([sol.T_avg if sol.T_avg is not None else np.zeros(0), ens["T_avg"][0, :n]])
    if keep_Y:
        prev = sol.Y_all if sol.Y_all is not None else np.zeros((0, p.N.tot))
        if prev.shape[0] != len(sol.t) - n:
            raise ValueError("the solution being continued was not saved with outputs='all'")
        sol.Y_all = np.concatenate([prev, ens["Y_all"][0, :n]])
    if sel is not None:
        prev = sol.Y_sel if sol.Y_sel is not None else np.zeros((0, ens["Y_sel"].shape[2]))
        sol.Y_sel = np.concatenate([prev, ens["Y_sel"][0, :n]])
        sol._sel, sol._sel_ind = sel, sel_ind
    sol.Y, sol.YP = ens["Y"][0].copy(), ens["YP"][0].copy()
    t_start = ens["t"][0, 0]
    sol.results.append(RunResult(name, (t_start, ri["t_end"]), ri["flag"], ri["iterations"], ri))
    sol.counters = ens["counters"][0]
    if tf_interp is not None:
        return sol(tf_interp, interp_bc=o.interp_bc)
    return sol


def simulate_b(sol, p, tf=1e6, **kw):
    """simulate!(sol, p, tf; kw...) -- continue `sol` (reference src/model_evaluation.jl:87-97)."""
    return simulate(p, tf, sol=sol, **kw)


# the per-point channels a sensitivity run can differentiate (simulate_ensemble(sens_outputs=...)) and a fit can use (EnsembleSolution.lsq): name -> the ensemble's array of
# its sensitivities; the curve itself is the attribute of that name
SENS_CHANNELS = {"V": "dV_dtheta", "I": "dI_dtheta", "T_avg": "dT_avg_dtheta"}


def _sens_channels(sens_outputs):
    names = [sens_outputs] if isinstance(sens_outputs, str) else list(sens_outputs)
    for c in names:
        if c not in SENS_CHANNELS:
            raise ValueError("sens_outputs: %r is not one of %s" % (c, ", ".join(SENS_CHANNELS)))
    return [c for c in SENS_CHANNELS if c in names]


def _integrate(p, theta, SOC0, runs, o, Y_init=None, t_init=None, device=False, stream=None, max_points=None, keep_Y=False, keep_YP=True, sens=None, sections=None, sens_outputs=("V",)):
    """one plh_integrate call; numpy in / numpy out (host pointers) or torch device tensors (device=True).
    keep_YP = False: YP_final is not requested (the reference keeps YP only with var_keep.YP; the kernel then does not store the previous point's YP per step).
    sections: ((start, len), ...) -> bufs["Y_sel"][cell, point, k]: only those entries of every saved state vector, packed in the order given (plh_outputs.sel / Y_sel).
    sens: list of theta keys -> plh_integrate_sens, bufs["dY_dtheta"][cell, k, state], bufs["dV_dtheta"][cell, k, point], bufs["sens_stat"][cell, 3].
    sens_outputs: the per-point channels differentiated, of "V", "I", "T_avg" -> bufs["dV_dtheta"], bufs["dI_dtheta"], bufs["dT_avg_dtheta"] (plh_integrate_sens_out; ("V",) is
    plh_integrate_sens itself)."""
    lib, h = p._lib, p._h
    n = theta.shape[0]
    N = p.N.tot
    arr = (cap.Run * len(runs))(*runs)
    os_ = _opts_struct(o, p)
    mp = int(max_points or o.max_points)
    out = cap.Outputs()
    out.max_pts = mp
    if device:
        import torch
        dev = theta.device
        mk = lambda *shape, dt=torch.float64: torch.empty(*shape, dtype=dt, device=dev)
        bufs = dict(t=mk(n, mp), V=mk(n, mp), I=mk(n, mp), SOC=mk(n, mp), n_pts=mk(n, dt=torch.int32), Y=mk(n, N), YP=mk(n, N),
                    run_info=torch.empty(n * len(runs) * cap.RUN_INFO_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                    counters=torch.empty(n * cap.COUNTERS_DTYPE.itemsize, dtype=torch.uint8, device=dev))
        kind = cap.PLH_DEVICE
    else:
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        SOC0 = np.ascontiguousarray(SOC0, dtype=np.float64)
        # (np.empty: the library overwrites every array in full; only the first n_pts[i] entries of a per-point row are meaningful)
        bufs = dict(t=np.empty((n, mp)), V=np.empty((n, mp)), I=np.empty((n, mp)), SOC=np.empty((n, mp)), n_pts=np.zeros(n, np.int32),
                    Y=np.empty((n, N)), YP=np.empty((n, N)), run_info=np.zeros((n, len(runs)), cap.RUN_INFO_DTYPE),
                    counters=np.zeros(n, cap.COUNTERS_DTYPE))
        if Y_init is not None:
            Y_init = np.ascontiguousarray(Y_init, dtype=np.float64)
            t_init = None if t_init is None else np.ascontiguousarray(t_init, dtype=np.float64)      # (None: initial_states -- a new solution from these states)
        kind = cap.PLH_HOST
    out.t, out.V, out.I, out.SOC = cap.ptr(bufs["t"]), cap.ptr(bufs["V"]), cap.ptr(bufs["I"]), cap.ptr(bufs["SOC"])
    out.T_avg = None
    out.Y_all = None
    if p.temperature:                   # per-step average temperature (calc_T_avg) only exists with temperature = true
        bufs["T_avg"] = mk(n, mp) if device else np.empty((n, mp))
        out.T_avg = cap.ptr(bufs["T_avg"])
    if keep_Y:                          # outputs = :all : every saved state vector
        bufs["Y_all"] = mk(n, mp, N) if device else np.empty((n, mp, N))
        out.Y_all = cap.ptr(bufs["Y_all"])
    out.n_sel, out.sel, out.Y_sel = 0, None, None
    if sections is not None:            # selected state entries per saved point
        sel_arr = np.ascontiguousarray(sections, dtype=np.int32).reshape(-1, 2)
        n_selt = max(int(sel_arr[:, 1].clip(0).sum()), 1)               # (a selection the library refuses is refused there: the buffer only has to exist)
        bufs["Y_sel"] = mk(n, mp, n_selt) if device else np.empty((n, mp, n_selt))
        out.n_sel, out.sel, out.Y_sel = len(sel_arr), sel_arr.ctypes.data_as(C.POINTER(C.c_int)), cap.ptr(bufs["Y_sel"])
    out.n_pts, out.Y_final, out.YP_final = cap.ptr(bufs["n_pts"]), cap.ptr(bufs["Y"]), cap.ptr(bufs["YP"]) if keep_YP else None
    out.run_info, out.counters = cap.ptr(bufs["run_info"]), cap.ptr(bufs["counters"])
    if sens:
        cols = np.ascontiguousarray([p.θ_keys.index(k) for k in sens], dtype=np.int32)
        ns = len(cols)
        chans = _sens_channels(sens_outputs)
        if device:
            bufs["dY_dtheta"], bufs["sens_stat"] = mk(n, ns, N), mk(n, 3, dt=torch.int32)
        else:
            bufs["dY_dtheta"], bufs["sens_stat"] = np.empty((n, ns, N)), np.zeros((n, 3), np.int32)
        for c in chans:
            bufs[SENS_CHANNELS[c]] = mk(n, ns, mp) if device else np.empty((n, ns, mp))
        if Y_init is not None:
            raise ValueError("sensitivities are integrated for new solutions only")
        bufs["sens_keys"] = list(sens)
        if chans == ["V"]:
            cap.check(lib, lib.plh_integrate_sens(h, n, cap.ptr(theta), cap.ptr(SOC0), len(runs), arr, C.byref(os_), C.byref(out), ns, cols.ctypes.data,
                                                  cap.ptr(bufs["dY_dtheta"]), cap.ptr(bufs["dV_dtheta"]), cap.ptr(bufs["sens_stat"]), kind, stream), "plh_integrate_sens")
        else:
            so = cap.SensOutputs(cap.ptr(bufs["dY_dtheta"]), cap.ptr(bufs.get("dV_dtheta")), cap.ptr(bufs.get("dI_dtheta")), cap.ptr(bufs.get("dT_avg_dtheta")), cap.ptr(bufs["sens_stat"]))
            cap.check(lib, lib.plh_integrate_sens_out(h, n, cap.ptr(theta), cap.ptr(SOC0), len(runs), arr, C.byref(os_), C.byref(out), ns, cols.ctypes.data, C.byref(so), kind, stream),
                      "plh_integrate_sens_out")
    else:
        t_call = time.perf_counter()
        rc = lib.plh_integrate(h, n, cap.ptr(theta), cap.ptr(SOC0), cap.ptr(Y_init), cap.ptr(t_init), len(runs), arr, C.byref(os_), C.byref(out), kind, stream)
        bufs["call_ms"] = 1e3 * (time.perf_counter() - t_call)          # wall time inside plh_integrate (a blocking PLH_HOST call: staging, kernel, the way back)
        cap.check(lib, rc, "plh_integrate")
    if device:
        if stream is not None and int(stream) != torch.cuda.current_stream(dev).cuda_stream:
            # the buffers were allocated on torch's current stream but the kernel runs on `stream`: tell the caching allocator, or it may hand the
            # memory out again while the kernel still writes it
            ext = torch.cuda.ExternalStream(int(stream), device=dev)
            for v in list(bufs.values()) + [theta, SOC0]:
                if hasattr(v, "record_stream"):
                    v.record_stream(ext)
        bufs["kernel_ms"] = lambda: lib.plh_last_kernel_ms(h)     # evaluated on access: the launch is asynchronous on `stream`
        bufs["stream"] = stream                                   # (what works on these buffers later -- ens(t) -- is queued behind the launch)
    else:
        bufs["kernel_ms"] = lib.plh_last_kernel_ms(h)
    return bufs


class ResampledEnsemble:
    """ens(t): an ensemble's per-point arrays on one time grid (EnsembleSolution.__call__).  t [n_q]; V, I, SOC, T_avg [cell, n_q]; Y_all [cell, n_q, state];
    Y_sel [cell, n_q, n_sel_total] -- those the ensemble holds and that were asked for, None otherwise; status [cell]."""

    def __init__(self, p, t, sel, sel_ind):
        self.p, self.t, self.sel, self.sel_ind = p, t, sel, sel_ind
        self.V = self.I = self.SOC = self.T_avg = self.Y_all = self.Y_sel = self.status = None

    def section(self, name):
        """[cell, n_q, len] of one state section, as EnsembleSolution.section"""
        if self.Y_sel is not None and name in self.sel_ind:
            return self.Y_sel[:, :, self.sel_ind[name]]
        if self.Y_all is not None and name in self.p.ind:
            return self.Y_all[:, :, self.p.ind[name]]
        raise KeyError("%r was not resampled: the ensemble needs sections=(%r,) or outputs='all', and ens(t, fields=...) must include it" % (name, name))


class EnsembleFit:
    """ens.lsq(t, V_data): the least-squares misfit of every cell's measured curves against data (EnsembleSolution.lsq).  cost [cell]; grad [cell, k] and JtJ [cell, k, k] with
    respect to the ensemble's `sens` keys (.keys), None for an ensemble run without them; resid (the voltage channel), resid_I, resid_T_avg [cell, n_q] when asked for and
    the channel was given, else None; channels: the names of the channels summed, in the order of the sums; status [cell]."""

    def __init__(self, keys, channels=("V",)):
        self.keys = list(keys)
        self.channels = list(channels)
        self.cost = self.grad = self.JtJ = self.resid = self.resid_I = self.resid_T_avg = self.status = None
        self._p = self._stream = None                                    # the model and the launch stream of the ensemble (ens.lsq sets them: by_group needs them)

    def by_group(self, groups):
        """The fits of consecutive cells that share their parameters, summed into one fit per group (plh_lsq_group; csrc/plh_group.h): groups [n_cells], the label of every
        cell's group (group_offsets).  Returns an EnsembleFit with one row per group: .cost [n_groups], .grad [n_groups, k], .JtJ [n_groups, k, k] -- every entry the sum of
        the members' entries, taken sequentially in ascending cell order from the first member's value (a group of one has its member's bits) --, .status [n_groups] (1: a
        member's status is not 0); resid* are None.  A fit in HBM stays there, queued on the ensemble's launch stream."""
        off = group_offsets(groups, self.cost.shape[0])
        ng, ns = len(off) - 1, len(self.keys)
        out = EnsembleFit(self.keys, self.channels)
        out._p, out._stream = self._p, self._stream
        device = not isinstance(self.cost, np.ndarray)
        if device:
            import torch
            dev = self.cost.device
            mk = lambda *shape, dt=torch.float64: torch.empty(*shape, dtype=dt, device=dev)
        else:
            mk = lambda *shape, dt=np.float64: np.empty(shape, dt)
        out.cost, out.status = mk(ng), mk(ng, dt=torch.int32 if device else np.int32)
        if ns:
            out.grad, out.JtJ = mk(ng, ns), mk(ng, ns, ns)
        ext = None
        if device and self._stream is not None and int(self._stream) != torch.cuda.current_stream(dev).cuda_stream:
            ext = torch.cuda.ExternalStream(int(self._stream), device=dev)      # (allocated on torch's current stream, written on the launch stream: as in ens.lsq)
            ext.wait_stream(torch.cuda.current_stream(dev))
        _lsq_group(self._p, off, self, out, self._stream)
        if ext is not None:
            for v in (out.cost, out.grad, out.JtJ, out.status):
                if v is not None:
                    v.record_stream(ext)
        return out


def group_offsets(groups, n_cells):
    """groups [n_cells]: the integer label of every cell's group, non-decreasing from 0 without gaps (the members of a group are consecutive cells).  Returns the offsets
    [n_groups + 1] (int32) the C ABI takes: group g owns the cells off[g] .. off[g + 1] - 1."""
    g = np.asarray(groups.cpu() if hasattr(groups, "cpu") else groups)
    if g.ndim != 1 or g.shape[0] != n_cells or g.shape[0] < 1:
        raise ValueError("groups must be a 1-D array of n_cells = %d labels" % n_cells)
    if not np.issubdtype(g.dtype, np.integer):
        raise ValueError("groups must be an integer array")
    g = g.astype(np.int64)
    d = np.diff(g)
    if g[0] != 0 or ((d != 0) & (d != 1)).any():
        raise ValueError("groups: the labels must start at 0 and be non-decreasing without gaps (the members of a group are consecutive cells)")
    return np.ascontiguousarray(np.concatenate([[0], np.flatnonzero(d) + 1, [n_cells]]), dtype=np.int32)


def _lsq_group(p, off, fit, out, stream):
    """plh_lsq_group: the per-cell EnsembleFit `fit` summed by groups into the arrays of `out` (host arrays or tensors in HBM, like fit's)"""
    kind = cap.PLH_HOST if isinstance(fit.cost, np.ndarray) else cap.PLH_DEVICE
    cap.check(p._lib, p._lib.plh_lsq_group(p._h, fit.cost.shape[0], len(off) - 1, off.ctypes.data, len(fit.keys), cap.ptr(fit.cost), cap.ptr(fit.grad), cap.ptr(fit.JtJ), cap.ptr(fit.status),
                                           cap.ptr(out.cost), cap.ptr(out.grad), cap.ptr(out.JtJ), cap.ptr(out.status), kind, stream if kind == cap.PLH_DEVICE else None), "plh_lsq_group")


class EnsemblePrediction:
    """ens.predict(t, cov): an ensemble's measured curves, their sensitivities and their prediction bands on one time grid (EnsembleSolution.predict).  t [n_q]; keys; channels:
    the names of the channels evaluated; per channel c of them V / I / T_avg [cell, n_q] (the resampled curve), dV_dtheta / dI_dtheta / dT_avg_dtheta [cell, k, n_q] (the
    resampled sensitivities), V_var / I_var / T_avg_var [cell, n_q] (the delta-method variance s' cov s of the curve, as computed: a tiny negative value from cancellation
    stays visible) and V_sd / I_sd / T_avg_sd = sqrt(max(var, 0)) -- var and sd are None without a covariance, and everything of a channel that was not evaluated is None;
    status [cell] (1: the cell failed or was cut at max_points -- its rows are NaN).  The band of the CURVE: a prediction interval for a new observation adds the
    measurement's sigma^2 to var."""

    def __init__(self, t, keys, channels):
        self.t, self.keys, self.channels = t, list(keys), list(channels)
        self.status = None
        for c in SENS_CHANNELS:
            for nm in (c, SENS_CHANNELS[c], c + "_var", c + "_sd"):
                setattr(self, nm, None)


def _group_offsets_or_labels(groups, n_cells):
    """the offsets [n_groups + 1] of `groups`, given as labels [n_cells] (group_offsets) or as the offsets themselves (an integer array that ends at n_cells: no array of
    labels does)"""
    g = np.asarray(groups.cpu() if hasattr(groups, "cpu") else groups)
    if g.ndim == 1 and g.size >= 2 and np.issubdtype(g.dtype, np.integer) and int(g[-1]) == n_cells:
        if g[0] != 0 or (np.diff(g.astype(np.int64)) < 1).any():
            raise ValueError("groups: offsets must start at 0, end at n_cells and be strictly ascending (every group has a member)")
        return np.ascontiguousarray(g, dtype=np.int32)
    return group_offsets(g, n_cells)


class EnsembleSolution:
    """Per-cell results of an ensemble run (arrays indexed [cell, point]); sol[i] gives a single-cell Solution."""

    def __init__(self, p, bufs, run_names, sel=None, sel_ind=None):
        self.p = p
        self.t, self.V, self.I, self.SOC = bufs["t"], bufs["V"], bufs["I"], bufs["SOC"]
        self.n_pts = bufs["n_pts"]
        self.Y, self.YP = bufs["Y"], bufs["YP"]
        self.T_avg = bufs.get("T_avg")          # [cell, point] with temperature = true
        self.Y_all = bufs.get("Y_all")          # [cell, point, state] with outputs = "all"
        self.Y_sel = bufs.get("Y_sel")          # [cell, point, n_sel_total] with sections = (...): the selected state entries, packed in the order given
        self.sel, self.sel_ind = sel, sel_ind   # ((start, len), ...) and {name or (start, len): slice into a row of Y_sel}
        self._run_info = bufs["run_info"]
        self._run_info_raw = bufs["run_info"]   # as the library wrote it (device=True: stays in HBM, ens(t) hands it back to the library)
        self._stream = bufs.get("stream")       # device=True: the launch stream
        self._counters = bufs["counters"]
        self.run_names = run_names
        self._kernel_ms = bufs.get("kernel_ms", -1.0)
        self.call_ms = bufs.get("call_ms")      # wall time of the plh_integrate call itself (host pointers: includes the copies back)
        # forward parameter sensitivities (simulate_ensemble(..., sens=[keys])): [cell, k, state] at the end of the protocol, [cell, k, point] for the voltage
        self.dY_dtheta, self.dV_dtheta, self.sens_stat = bufs.get("dY_dtheta"), bufs.get("dV_dtheta"), bufs.get("sens_stat")
        # the further per-point channels (sens_outputs=("V", "I", "T_avg")): [cell, k, point], None when not asked for
        self.dI_dtheta, self.dT_avg_dtheta = bufs.get("dI_dtheta"), bufs.get("dT_avg_dtheta")
        self.keys = list(bufs.get("sens_keys") or [])      # the `sens` names, in the order of the k axis

    # With device=True the launch is asynchronous: the per-cell summaries stay in HBM until they are looked at (the first access synchronises),
    # so a host loop can enqueue launches back to back.
    @property
    def run_info(self):
        if not isinstance(self._run_info, np.ndarray):
            self._run_info = self._run_info.cpu().numpy().view(cap.RUN_INFO_DTYPE).reshape(self.t.shape[0], len(self.run_names))
        return self._run_info

    @property
    def counters(self):
        if not isinstance(self._counters, np.ndarray):
            self._counters = self._counters.cpu().numpy().view(cap.COUNTERS_DTYPE).reshape(self.t.shape[0])
        return self._counters

    @property
    def kernel_ms(self):
        """duration of the integrate kernel of the handle's LAST launch (HIP events on the launch stream)"""
        if callable(self._kernel_ms):
            self._kernel_ms = self._kernel_ms()
        return self._kernel_ms

    @property
    def n_cells(self):
        return self.t.shape[0]

    def flags(self):
        return self.run_info["flag"]

    def section(self, name):
        """[cell, point, len] of one saved state section: from Y_sel when it was selected (sections=), else from Y_all when every state was kept (outputs = "all")"""
        if self.Y_sel is not None and name in self.sel_ind:
            return self.Y_sel[:, :, self.sel_ind[name]]
        if self.Y_all is not None and name in self.p.ind:
            return self.Y_all[:, :, self.p.ind[name]]
        raise KeyError("%r was not saved: run with sections=(%r,) or outputs='all'" % (name, name))

    def __call__(self, t, interp_bc="interpolate", fields=None, k=3):
        """ens(t): every per-point array of the ensemble (V, I, SOC, T_avg, Y_all, Y_sel -- or only the names in `fields`) on the time grid `t` shared by all cells: the
        reference's sol(t) (src/save_outputs.jl:74-133) for the whole ensemble, on the device (plh_resample, one call per array; csrc/plh_resample.h).  Per run the interpolating
        cubic spline through its saved points, the same function as ens[i](t) builds with scipy's splrep to rounding; interp_bc as there.  A device=True ensemble stays in HBM
        (torch tensors, queued on the launch stream), a host ensemble gives numpy arrays.  Returns a ResampledEnsemble: .t [n_q], the arrays as [cell, n_q(, width)],
        .status [cell] (1: the cell failed or was cut at max_points -- its rows are NaN), .section(name), .sel_ind."""
        if k != 3:
            raise ValueError("ens(t) offers the cubic spline (k = 3) only; another degree: ens[i](t, k=%r), one cell at a time on the host" % (k,))
        if interp_bc not in ("interpolate", "extrapolate"):
            raise ValueError("Invalid interp_bc method.")
        have = [f for f in ("V", "I", "SOC", "T_avg", "Y_all", "Y_sel") if getattr(self, f, None) is not None]
        names = have if fields is None else [fields] if isinstance(fields, str) else list(fields)
        for f in names:
            if f not in have:
                raise KeyError("%r is not a per-point array of this ensemble (it holds %s)" % (f, ", ".join(have)))
        tq = np.ascontiguousarray(np.atleast_1d(np.asarray(t, dtype=np.float64)))
        if tq.ndim != 1 or tq.size < 1:
            raise ValueError("t must be a time or a 1-D array of times")
        lib, h = self.p._lib, self.p._h
        n, mp = self.t.shape
        device = not isinstance(self.t, np.ndarray)
        out = ResampledEnsemble(self.p, tq, self.sel, self.sel_ind)
        if device:
            import torch
            dev = self.t.device
            mk = lambda *shape, dt=torch.float64: torch.empty(*shape, dtype=dt, device=dev)
            kind, stream, rinfo = cap.PLH_DEVICE, self._stream, self._run_info_raw
        else:
            mk = lambda *shape, dt=np.float64: np.empty(shape, dt)
            kind, stream, rinfo = cap.PLH_HOST, None, np.ascontiguousarray(self.run_info)
        out.status = mk(n, dt=torch.int32) if device else mk(n, dt=np.int32)
        made = [out.status]
        for f in names:
            x = getattr(self, f)
            width = 1 if x.ndim == 2 else x.shape[2]
            y = mk(n, tq.size) if x.ndim == 2 else mk(n, tq.size, width)
            cap.check(lib, lib.plh_resample(h, n, len(self.run_names), mp, cap.ptr(self.t), cap.ptr(self.n_pts), cap.ptr(rinfo), width, cap.ptr(x), tq.size, tq.ctypes.data,
                                            1 if interp_bc == "extrapolate" else 0, cap.ptr(y), cap.ptr(out.status), kind, stream), "plh_resample")
            setattr(out, f, y)
            made.append(y)
        if device and stream is not None and int(stream) != torch.cuda.current_stream(dev).cuda_stream:
            ext = torch.cuda.ExternalStream(int(stream), device=dev)      # (allocated on torch's current stream, written on the launch stream: as in _integrate)
            for v in made:
                v.record_stream(ext)
        return out

    def lsq(self, t, V_data=None, weights=None, interp_bc="interpolate", resid=False, I_data=None, I_weights=None, T_avg_data=None, T_avg_weights=None):
        """The weighted least-squares misfit of every cell's measured curves against data on the device (plh_lsq_multi; csrc/plh_lsq.h), and -- for an ensemble run with
        sens=[keys] -- its gradient and Gauss-Newton matrix with respect to those keys.  Channels: the voltage (V_data, weights), the current (I_data, I_weights: what a
        constant-voltage leg measures) and the average temperature (T_avg_data, T_avg_weights); at least one.  With S_c = ens(t).<channel> and S_ck the same spline through
        row k of the channel's sensitivities (dV_dtheta, dI_dtheta, dT_avg_dtheta: simulate_ensemble(sens_outputs=...)), r_c = w_c (S_c(t) - data_c), J_c[:, k] = w_c S_ck(t):
        cost = sum_c r_c.r_c / 2, grad = sum_c J_c'r_c, JtJ = sum_c J_c'J_c per cell (J at fixed knots: the saved times' dependence on the parameters is ignored, as for every
        post-interpolated output).  t [n_q], shared by the channels (a channel without a datum at a time gets weight 0 there); data and weights [n_q] (shared by all cells) or
        [n_cells, n_q]; weights None: ones.  A point with weight 0 is left out of its channel (a NaN time or datum there is harmless).  interp_bc as ens(t).  A device=True
        ensemble takes and returns torch tensors in HBM, queued on the launch stream; a host ensemble numpy arrays.  Returns an EnsembleFit: .cost [n], .grad [n, k],
        .JtJ [n, k, k] (None without sens), .resid / .resid_I / .resid_T_avg [n, n_q] (resid=True, per channel given) or None, .channels, .status [n] (1: the cell failed or
        was cut at max_points -- its rows are NaN), .keys."""
        if interp_bc not in ("interpolate", "extrapolate"):
            raise ValueError("Invalid interp_bc method.")
        tq = np.ascontiguousarray(np.asarray(t.cpu() if hasattr(t, "cpu") else t, dtype=np.float64))
        if tq.ndim != 1 or tq.size < 1:
            raise ValueError("t must be a 1-D array of measurement times")
        given = [(c, d, w_) for c, d, w_ in (("V", V_data, weights), ("I", I_data, I_weights), ("T_avg", T_avg_data, T_avg_weights)) if d is not None]
        if not given:
            raise ValueError("ens.lsq needs the data of at least one channel: V_data, I_data or T_avg_data")
        n, mp = self.t.shape
        ns = len(self.keys)
        if ns > cap.LSQ_MAX_SENS:
            raise ValueError("ens.lsq takes at most %d sens keys per call (this ensemble has %d)" % (cap.LSQ_MAX_SENS, ns))
        for c, _, _ in given:
            if getattr(self, c, None) is None:
                raise ValueError("this ensemble has no per-point %s" % c)
            if ns and getattr(self, SENS_CHANNELS[c]) is None:
                raise ValueError("%s_data: this ensemble was run without the sensitivities of %s; ask for them with simulate_ensemble(..., sens_outputs=(..., %r))" % (c, c, c))
        device = not isinstance(self.t, np.ndarray)
        if device:
            import torch
            dev = self.t.device
            conv = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()      # (numpy 2 arrays have .device too)
            mk = lambda *shape, dt=torch.float64: torch.empty(*shape, dtype=dt, device=dev)
            kind, stream, rinfo = cap.PLH_DEVICE, self._stream, self._run_info_raw
        else:
            conv = lambda a: np.ascontiguousarray(a, dtype=np.float64)
            mk = lambda *shape, dt=np.float64: np.empty(shape, dt)
            kind, stream, rinfo = cap.PLH_HOST, None, np.ascontiguousarray(self.run_info)
        ext = None
        if device and stream is not None and int(stream) != torch.cuda.current_stream(dev).cuda_stream:
            # data made or converted on torch's current stream are read on the launch stream: that stream waits for them, and the allocator learns of their use there
            ext = torch.cuda.ExternalStream(int(stream), device=dev)
        data = [[c, conv(d), None if w_ is None else conv(w_)] for c, d, w_ in given]
        wname = {"V": "weights", "I": "I_weights", "T_avg": "T_avg_weights"}
        for c, y, w in data:
            for what, a in ((c + "_data", y), (wname[c], w)):
                if a is not None and tuple(a.shape) not in ((tq.size,), (n, tq.size)):
                    raise ValueError("%s must be [n_q] or [n_cells, n_q] = [%d] or [%d, %d], not %s" % (what, tq.size, n, tq.size, list(a.shape)))
        per_cell = 1 if any(a is not None and a.ndim == 2 for _, y, w in data for a in (y, w)) else 0
        if per_cell:                                            # (one form for every array of every channel)
            full = lambda a: a if a is None or a.ndim == 2 else conv(a.expand(n, tq.size) if device else np.broadcast_to(a, (n, tq.size)))
            data = [[c, full(y), full(w)] for c, y, w in data]
        if ext is not None:
            ext.wait_stream(torch.cuda.current_stream(dev))
        out = EnsembleFit(self.keys, [c for c, _, _ in data])
        out._p, out._stream = self.p, stream
        out.cost, out.status = mk(n), mk(n, dt=torch.int32 if device else np.int32)
        if ns:
            out.grad, out.JtJ = mk(n, ns), mk(n, ns, ns)
        rname = {"V": "resid", "I": "resid_I", "T_avg": "resid_T_avg"}
        ch = (cap.LsqChannel * len(data))()
        for q, (c, y, w) in enumerate(data):
            if resid:
                setattr(out, rname[c], mk(n, tq.size))
            ch[q] = cap.LsqChannel(cap.ptr(getattr(self, c)), cap.ptr(getattr(self, SENS_CHANNELS[c])) if ns else None, cap.ptr(y), cap.ptr(w), cap.ptr(getattr(out, rname[c])))
        lib, h = self.p._lib, self.p._h
        cap.check(lib, lib.plh_lsq_multi(h, n, len(self.run_names), mp, cap.ptr(self.t), cap.ptr(self.n_pts), cap.ptr(rinfo), len(data), ch, ns,
                                         tq.size, tq.ctypes.data, per_cell, 1 if interp_bc == "extrapolate" else 0,
                                         cap.ptr(out.cost), cap.ptr(out.grad), cap.ptr(out.JtJ), cap.ptr(out.status), kind, stream), "plh_lsq_multi")
        if ext is not None:
            for v in [a for _, y, w in data for a in (y, w)] + [out.cost, out.grad, out.JtJ, out.resid, out.resid_I, out.resid_T_avg, out.status]:
                if v is not None:
                    v.record_stream(ext)
        return out

    def predict(self, t, cov=None, groups=None, channels=None, interp_bc="interpolate"):
        """Prediction bands on the device (plh_predict; csrc/plh_predict.h; include/petlion_hip.h states the definition): the measured curves of an ensemble run with
        sens=[keys] and the rows of their sensitivities on the time grid t [n_q] -- the functions ens(t) and ens.lsq evaluate -- and, with a covariance of the keys, the
        delta-method variance s' cov s of every curve at every time.  channels: of "V", "I", "T_avg"; default: every channel whose sensitivities the ensemble carries
        (simulate_ensemble(sens_outputs=...)).  cov: None (no variance), a FitCovariance (fit_covariance, res.covariance()) or an [n_prob, k, k] array / tensor in the units
        of theta; n_prob = n_cells, or with groups (labels [n_cells] as fit_ensemble takes them, or offsets [n_groups + 1]) n_groups: every member of a group takes its
        group's matrix.  interp_bc as ens(t).  A device=True ensemble gets tensors in HBM, queued on the launch stream; a host ensemble numpy arrays.  Returns an
        EnsemblePrediction."""
        if interp_bc not in ("interpolate", "extrapolate"):
            raise ValueError("Invalid interp_bc method.")
        tq = np.ascontiguousarray(np.atleast_1d(np.asarray(t.cpu() if hasattr(t, "cpu") else t, dtype=np.float64)))
        if tq.ndim != 1 or tq.size < 1:
            raise ValueError("t must be a time or a 1-D array of times")
        n, mp = self.t.shape
        ns = len(self.keys)
        if ns < 1:
            raise ValueError("ens.predict needs an ensemble run with sens=[keys]; without sensitivities ens(t) resamples the curves")
        if ns > cap.LSQ_MAX_SENS:
            raise ValueError("ens.predict takes at most %d sens keys per call (this ensemble has %d)" % (cap.LSQ_MAX_SENS, ns))
        have = [c for c in SENS_CHANNELS if getattr(self, c, None) is not None and getattr(self, SENS_CHANNELS[c], None) is not None]
        names = have if channels is None else [channels] if isinstance(channels, str) else list(channels)
        for c in names:
            if c not in SENS_CHANNELS:
                raise ValueError("channels: %r is not one of %s" % (c, ", ".join(SENS_CHANNELS)))
            if c not in have:
                raise ValueError("this ensemble was run without the sensitivities of %s; ask for them with simulate_ensemble(..., sens_outputs=(..., %r))" % (c, c))
        names = [c for c in SENS_CHANNELS if c in names]
        if not names:
            raise ValueError("ens.predict: this ensemble carries no channel with its sensitivities (simulate_ensemble(sens=[keys], sens_outputs=...))")
        if groups is not None and cov is None:
            raise ValueError("ens.predict: groups say which covariance a cell takes; give cov")
        off = None if groups is None else _group_offsets_or_labels(groups, n)
        n_prob = n if off is None else len(off) - 1
        cv = cov.cov if isinstance(cov, FitCovariance) else cov
        if cv is not None and tuple(cv.shape) != (n_prob, ns, ns):
            raise ValueError("cov must be [%s, k, k] = [%d, %d, %d], not %s" % ("n_cells" if off is None else "n_groups", n_prob, ns, ns, list(cv.shape)))
        device = not isinstance(self.t, np.ndarray)
        if device:
            import torch
            dev = self.t.device
            conv = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()
            mk = lambda *shape, dt=torch.float64: torch.empty(*shape, dtype=dt, device=dev)
            kind, stream, rinfo = cap.PLH_DEVICE, self._stream, self._run_info_raw
        else:
            conv = lambda a: np.ascontiguousarray(a.cpu() if hasattr(a, "cpu") else a, dtype=np.float64)
            mk = lambda *shape, dt=np.float64: np.empty(shape, dt)
            kind, stream, rinfo = cap.PLH_HOST, None, np.ascontiguousarray(self.run_info)
        cv = None if cv is None else conv(cv)
        ext = None
        if device and stream is not None and int(stream) != torch.cuda.current_stream(dev).cuda_stream:
            ext = torch.cuda.ExternalStream(int(stream), device=dev)      # (made or converted on torch's current stream, used on the launch stream: as in fit_covariance)
            ext.wait_stream(torch.cuda.current_stream(dev))
        out = EnsemblePrediction(tq, self.keys, names)
        out.status = mk(n, dt=torch.int32 if device else np.int32)
        ch = (cap.PredictChannel * len(names))()
        for q, c in enumerate(names):
            setattr(out, c, mk(n, tq.size))
            setattr(out, SENS_CHANNELS[c], mk(n, ns, tq.size))
            if cv is not None:
                setattr(out, c + "_var", mk(n, tq.size))
            ch[q] = cap.PredictChannel(cap.ptr(getattr(self, c)), cap.ptr(getattr(self, SENS_CHANNELS[c])), cap.ptr(getattr(out, c)), cap.ptr(getattr(out, SENS_CHANNELS[c])),
                                       cap.ptr(getattr(out, c + "_var")))
        lib, h = self.p._lib, self.p._h
        cap.check(lib, lib.plh_predict(h, n, len(self.run_names), mp, cap.ptr(self.t), cap.ptr(self.n_pts), cap.ptr(rinfo), len(names), ch, ns, tq.size, tq.ctypes.data,
                                       1 if interp_bc == "extrapolate" else 0, cap.ptr(cv), 0 if off is None else len(off) - 1, None if off is None else off.ctypes.data,
                                       cap.ptr(out.status), kind, stream), "plh_predict")
        if cv is not None:                                               # sd = sqrt(max(var, 0)) (NaN stays NaN), behind the kernel on its stream
            for c in names:
                var = getattr(out, c + "_var")
                if not device:
                    sd = np.sqrt(np.maximum(var, 0.0))
                elif ext is None:
                    sd = torch.sqrt(torch.clamp(var, min=0.0))
                else:
                    with torch.cuda.stream(ext):
                        sd = torch.sqrt(torch.clamp(var, min=0.0))
                    sd.record_stream(torch.cuda.current_stream(dev))
                setattr(out, c + "_sd", sd)
        if ext is not None:
            for v in [cv, out.status] + [getattr(out, nm) for c in names for nm in (c, SENS_CHANNELS[c], c + "_var")]:
                if v is not None:
                    v.record_stream(ext)
        return out

    def __getitem__(self, i):
        host = lambda x: (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)).copy()      # device=True results are torch tensors in HBM
        s = Solution()
        n = int(self.n_pts[i])
        s.t, s.V, s.I, s.SOC = host(self.t[i, :n]), host(self.V[i, :n]), host(self.I[i, :n]), host(self.SOC[i, :n])
        s.P = s.I * calc_I1C(self.p.θ) * s.V
        s.Y, s.YP = host(self.Y[i]), host(self.YP[i])
        s._ind = self.p.ind
        if self.T_avg is not None:
            s.T_avg = host(self.T_avg[i, :n])
        if self.Y_all is not None:
            s.Y_all = host(self.Y_all[i, :n])
        if self.Y_sel is not None:
            s.Y_sel, s._sel, s._sel_ind = host(self.Y_sel[i, :n]), self.sel, self.sel_ind
        t0 = 0.0
        for k, nm in enumerate(self.run_names):
            ri = self.run_info[i, k]
            s.results.append(RunResult(nm, (t0, ri["t_end"]), ri["flag"], ri["iterations"], ri))
            t0 = ri["t_end"]
        s.counters = self.counters[i]
        return s


def make_protocol(p, protocol, n_cells=None):
    """protocol: list of dicts like {"I": 2, "tf": 1800, "V_max": 4.1} / {"V": "hold", "I_min": 1/20} -- each dict is the
    keyword set of one simulate()/simulate!() call.  An input value or `tf` given as a 1-D numpy array of length n_cells is applied cell by cell
    (a C-rate sweep is `{"I": -np.linspace(0.5, 3, n)}`)."""
    runs, names = [], []
    for step in protocol:
        step = dict(step)
        tf = step.pop("tf", 1e6)
        inputs, bounds, rest = _split_kwargs(p, step)
        if rest:
            raise TypeError("unknown protocol keys %r" % list(rest))
        (name, inp), = inputs.items()
        for what, arr in (("input", inp), ("tf", tf)):
            if isinstance(arr, np.ndarray) and (n_cells is None or arr.shape != (n_cells,)):
                raise ValueError("per-cell %s: expected a 1-D array of length n_cells" % what)
        runs.append(_make_run(p, name, inp, tf, bounds))
        names.append(name)
    return runs, names


def simulate_ensemble(p, Theta, protocol, *, SOC=None, opts=None, device=False, stream=None, max_points=None, outputs=None, YP=True, sens=None, initial_states=None, sections=None, sens_outputs=("V",)):
    """Integrate an ensemble of independent cells on this process's GPU.

    Theta: [n_cells, n_theta] array in `p.θ_keys` order (numpy = host memory; torch CUDA tensor with device=True = already in HBM).
    protocol: list of run dicts (see make_protocol) shared by all cells.  SOC: scalar or [n_cells] initial SOC.
    outputs: "all" (or any state name) also returns every saved state vector as ens.Y_all [cell, point, state] -- 8 N bytes per point.
    sections: ("c_e", "T", (start, len), ...) -- state names of p.ind and / or index ranges: ens.Y_sel [cell, point, n_sel_total] holds only those entries of every saved
    state vector, packed in the order given (8 n_sel_total bytes per point instead of 8 N); ens.sel_ind[name] is the slice of a section in that row, ens.section(name) the
    section itself.  Independent of `outputs`: with both, Y_sel repeats the columns of Y_all.
    YP = False: do not return YP of the final point (the reference's default: var_keep.YP is off unless :YP is among the outputs).
    sens = ["D_sp", "k_n", ...]: forward sensitivities with respect to these entries of θ next to the states (plh_integrate_sens): ens.dY_dtheta[cell, k, state] at the
    end of the protocol, ens.dV_dtheta[cell, k, point] at every saved point; the states and saved points are those of the call without `sens`.
    sens_outputs = ("V", "I", "T_avg"): the per-point channels differentiated (default: the voltage only) -- "I" adds ens.dI_dtheta[cell, k, point], what a constant-voltage
    leg measures; "T_avg" (thermal models) adds ens.dT_avg_dtheta[cell, k, point]; a channel not named is None.  ens.lsq fits against any of them.
    """
    n = Theta.shape[0]
    runs, names = make_protocol(p, protocol, n)
    o = opts or p.opts
    soc = p.opts.SOC if SOC is None else SOC
    if device:
        import torch
        soc0 = soc if hasattr(soc, "device") else torch.full((n,), float(soc), dtype=torch.float64, device=Theta.device)
    else:
        soc0 = np.full(n, float(soc)) if np.isscalar(soc) else np.asarray(soc, dtype=np.float64)
    Y0 = None
    if initial_states is not None:          # [n_cells, N.tot] (host array): every cell starts a NEW solution from its own state vector; SOC = calc_SOC of it unless given
        if device:
            raise ValueError("initial_states: host arrays (device = False)")
        Y0 = np.ascontiguousarray(initial_states, dtype=np.float64)
        if Y0.shape != (n, p.N.tot):
            raise ValueError("initial_states must be [n_cells, N.tot]")
        if SOC is None:
            # (with the theta the run is made with -- a sweep over c_max_n / the anode's stoichiometry window changes every cell's SOC of the same state vector)
            th = np.asarray(Theta if not hasattr(Theta, "cpu") else Theta.cpu(), dtype=np.float64)
            col = lambda k: th[:, p.θ_keys.index(k)] if k in p.θ_keys else np.full(n, p.θ[k])
            cs = p.ind["c_s_avg"]
            n_p = p.N.p * p.N.r_p if p.solid_diffusion == "Fickian" else p.N.p
            soc0 = np.ascontiguousarray((Y0[:, cs.start + n_p:cs.stop].mean(axis=1) / col("c_max_n") - col("θ_min_n")) / (col("θ_max_n") - col("θ_min_n")))
    sel, sel_ind = _resolve_sections(p, sections)
    bufs = _integrate(p, Theta, soc0, runs, o, Y_init=Y0, device=device, stream=stream, max_points=max_points,
                      keep_Y=_wants_states(p, o.outputs if outputs is None else outputs), keep_YP=YP, sens=sens, sections=sel, sens_outputs=sens_outputs)
    return EnsembleSolution(p, bufs, names, sel, sel_ind)


class EnsembleFitResult:
    """fit_ensemble's result.  theta [n, n_theta]: every cell's best point; cost [n], grad [n, k], JtJ [n, k, k]: the fit at that point (NaN for a cell whose start could not
    be used); state [n] (cap.LM_*: CONV_F / CONV_X / CONV_G / MAXIT / STALLED / FAILED_START, names in cap.LM_STATE_NAMES), lam [n], n_accept [n], n_reject [n]; n_iter: the
    number of integrations; keys; history: None, or per iteration a dict of host copies (phase, theta_before / theta_after, cost, grad, JtJ, status, before / after: the
    per-cell state arrays, n_running).
    A grouped fit (fit_ensemble(groups=...)): group_off [n_groups + 1] (else None); theta stays [n, n_theta], every member holding its group's best point; every other array
    has one row per GROUP, and so has the history (theta_before / theta_after are the [n_groups, n_theta] matrix of the groups' rows), which additionally records
    member = dict(cost, grad, JtJ, status), the per-cell fits that were summed, and Theta, the per-cell matrix after the scatter."""

    def __init__(self, keys):
        self.keys = list(keys)
        self.theta = self.cost = self.grad = self.JtJ = self.state = self.lam = self.n_accept = self.n_reject = self.history = self.group_off = None
        self.theta_cur = self.n_data = None                              # [n, k]: the keys' values at the best point; [n] int32: the data of every problem (covariance)
        self.n_iter = 0
        self._p = self._tf = self._lo = self._hi = self._stream = None   # what covariance() needs of the fit: the model, transform, the bounds as plh_lm_step took them, the launch stream
        self._protocol = self._SOC = self._opts = self._max_points = self._device = self._sens_outputs = self._interp_bc = None      # what predict() needs to integrate once more

    def covariance(self, absolute_sigma=False):
        """Parameter covariances and identifiability at the best point of every problem (plh_fit_cov; csrc/plh_cov.h; include/petlion_hip.h states the definition), with the
        fit's own transform and bounds: one row per cell, or per group for a grouped fit.  absolute_sigma=False: the residual variance is estimated, sigma2 =
        2 cost / (n_data - n_free); True: the weights are taken as 1 / sigma of the data, sigma2 = 1 (scipy's absolute_sigma).  A fit in HBM stays there, queued on the fit's
        launch stream.  Returns a FitCovariance."""
        return fit_covariance(self._p, self.theta_cur, self.cost, self.grad, self.JtJ, n_data=None if absolute_sigma else self.n_data, transform=self._tf, lo=self._lo, hi=self._hi,
                              stream=self._stream, keys=self.keys)

    def predict(self, t, absolute_sigma=False, channels=None):
        """Prediction bands of the fitted curves at the times t [n_q]: one sensitivity integration at the best point self.theta (the last integration of the fit was that of
        the last TRIAL, not of the best point), then ens.predict(t, self.covariance(absolute_sigma)) with the fit's grouping, channels and interp_bc.  channels: of the
        channels the fit had data of (default: all of them).  A fit in HBM stays there.  Returns an EnsemblePrediction; every member of a group is banded with its group's
        covariance."""
        ens = simulate_ensemble(self._p, self.theta, self._protocol, SOC=self._SOC, opts=self._opts, device=self._device, stream=self._stream, max_points=self._max_points,
                                YP=False, sens=self.keys, sens_outputs=self._sens_outputs)
        return ens.predict(t, cov=self.covariance(absolute_sigma), groups=self.group_off, channels=channels, interp_bc=self._interp_bc)


class FitCovariance:
    """fit_covariance's result, one row per problem; numpy arrays, or tensors in HBM.  sigma2 [n]: the residual variance; cov [n, k, k] and stderr [n, k] in the units of
    theta (0 for a key held at a bound, NaN / +inf for a key the data do not see); corr [n, k, k]; eval [n, k] ascending and evec [n, k, k] (evec[:, j] is eigenvector j over
    the keys): the eigen-decomposition of the normalised information matrix over the analysed keys -- the eigenvector of the smallest eigenvalue is the direction the data see
    least; collinearity [n] = 1 / sqrt(eval[:, 0]) (Brun et al.); free [n]: bit i is set for a key that is not held; status [n]: 0, or bits cap.COV_* (names in
    cap.COV_STATUS_NAMES; bits 8 .. 15: the keys the data do not see); keys."""

    def __init__(self, keys):
        self.keys = None if keys is None else list(keys)
        self.sigma2 = self.cov = self.stderr = self.corr = self.eval = self.evec = self.collinearity = self.free = self.status = None


def fit_covariance(p, theta_k, cost, grad, JtJ, *, n_data=None, transform=None, lo=None, hi=None, stream=None, keys=None):
    """plh_fit_cov on the arrays a fit left behind: theta_k [n, k] (the keys' values), cost [n], grad [n, k], JtJ [n, k, k] -- fit_ensemble's result, or ens.lsq(...)'s arrays
    (and .by_group's) with the keys' columns of Theta.  n_data [n] (int): the number of data of every problem, None: sigma2 = 1.  transform [k]: "log" / "linear" (or
    cap.LM_LOG / cap.LM_LINEAR) per key, None: linear.  lo, hi: None, [k] (host) or [n, k] (where the inputs live), as fit_ensemble's bounds reach plh_lm_step.  numpy inputs
    give numpy arrays; tensors in HBM give tensors in HBM, queued on `stream`.  Returns a FitCovariance."""
    device = not isinstance(cost, np.ndarray)
    n, k = grad.shape[0], grad.shape[1]
    tf = np.zeros(k, np.int32) if transform is None else np.ascontiguousarray([{"linear": cap.LM_LINEAR, "log": cap.LM_LOG}.get(v, v) if isinstance(v, str) else int(v) for v in transform], dtype=np.int32)
    if tf.shape != (k,):
        raise ValueError("fit_covariance: transform must have one entry per key (%d)" % k)
    if device:
        import torch
        dev = cost.device
        conv = lambda a, dt=torch.float64: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).to(device=dev, dtype=dt).contiguous()
        mk = lambda *shape, dt=torch.float64: torch.empty(*shape, dtype=dt, device=dev)
        kind, it = cap.PLH_DEVICE, torch.int32
    else:
        conv = lambda a, dt=np.float64: None if a is None else np.ascontiguousarray(a, dtype=dt)
        mk = lambda *shape, dt=np.float64: np.empty(shape, dt)
        kind, it, stream = cap.PLH_HOST, np.int32, None
    bdim = lambda b: 0 if b is None else (b.dim() if hasattr(b, "dim") else np.ndim(b))
    per_cell = any(bdim(b) == 2 for b in (lo, hi))
    if per_cell:                                                         # (one form for both sides: [n, k] where the inputs live)
        full = lambda b, dflt: conv(np.full((n, k), dflt)) if b is None else (conv(b) if bdim(b) == 2 else conv(np.broadcast_to(np.asarray(b.cpu() if hasattr(b, "cpu") else b, dtype=np.float64), (n, k))))
        lo_a, hi_a = full(lo, -np.inf), full(hi, np.inf)
    else:                                                                # [k] on the host
        lo_a, hi_a = (None if b is None else np.ascontiguousarray(b.cpu() if hasattr(b, "cpu") else b, dtype=np.float64) for b in (lo, hi))
    ins = [conv(theta_k), conv(cost), conv(grad), conv(JtJ), conv(n_data, it)]
    out = FitCovariance(keys)
    out.sigma2, out.cov, out.stderr, out.corr, out.eval, out.evec, out.collinearity = mk(n), mk(n, k, k), mk(n, k), mk(n, k, k), mk(n, k), mk(n, k, k), mk(n)
    out.free, out.status = mk(n, dt=it), mk(n, dt=it)
    outs = [out.sigma2, out.cov, out.stderr, out.corr, out.eval, out.evec, out.collinearity, out.free, out.status]
    ext = None
    if device and stream is not None and int(stream) != torch.cuda.current_stream(dev).cuda_stream:
        ext = torch.cuda.ExternalStream(int(stream), device=dev)         # (made or converted on torch's current stream, used on the launch stream: as in by_group)
        ext.wait_stream(torch.cuda.current_stream(dev))
    cap.check(p._lib, p._lib.plh_fit_cov(p._h, n, k, tf.ctypes.data, cap.ptr(ins[0]), cap.ptr(lo_a), cap.ptr(hi_a), 1 if per_cell else 0, cap.ptr(ins[1]), cap.ptr(ins[2]), cap.ptr(ins[3]),
                                         cap.ptr(ins[4]), *[cap.ptr(v) for v in outs], kind, stream), "plh_fit_cov")
    if ext is not None:
        for v in ins + outs + [lo_a, hi_a]:
            if hasattr(v, "record_stream"):
                v.record_stream(ext)
    return out


LM_STATE_ARRAYS = ("theta_cur", "cost_cur", "grad_cur", "JtJ_cur", "lam", "pred", "state", "n_accept", "n_reject")


def fit_ensemble(p, Theta0, protocol, keys, t, V_data=None, weights=None, I_data=None, I_weights=None, T_avg_data=None, T_avg_weights=None, *, bounds=None, transform=None,
                 max_iter=30, check_every=1, SOC=None, opts=None, lm=None, device=False, stream=None, max_points=None, interp_bc="interpolate", history=False, groups=None):
    """Levenberg-Marquardt fit of every cell's `keys` to measured curves, the loop on the device: per iteration one sensitivity integration (simulate_ensemble(sens=keys)),
    ens.lsq(t, ...) and one plh_lm_step (csrc/plh_lm.h; include/petlion_hip.h states what a step does), which judges the trial, updates the damping, tests convergence, solves
    the damped, scaled, bounded normal equations and writes the next trial into Theta -- all in HBM with device=True, where the 4-byte read of the number of running cells every
    `check_every` iterations is the loop's only synchronisation.
    Theta0 [n, n_theta] (not modified); protocol, SOC, opts, max_points, device, stream as simulate_ensemble; t and the data / weights of the channels as ens.lsq (the channels
    given data are the ones differentiated).  bounds = {key: (lo, hi)}, scalars or [n_cells] arrays, None = unbounded on that side; transform = {key: "log" | "linear"} (default
    linear; log: the step is taken in ln theta, the parameter must be positive); lm = {option: value} over cap.LM_OPT_DEFAULTS.  At most max_iter + 1 integrations: the first
    point, up to max_iter - 1 steps, and one last judgement.  Cells that are done keep being integrated at their best point (the ensemble is not compacted).
    groups [n_cells] (labels, see group_offsets): consecutive cells form a group, one experiment per member, and the members of a group SHARE the keys -- one group is one
    least-squares problem (several C-rates, a discharge and a rest, many starts at once).  Every other column of Theta0, the protocol's per-cell inputs / tf, SOC and per-cell
    data and weights stay per cell: that is how members differ.  A group starts at its FIRST member's values of the keys (scattered to all members before the first
    integration).  Per iteration: the integration, ens.lsq, plh_lsq_group (the members' fits summed), plh_lm_step on the [n_groups, n_theta] matrix of the first members' rows,
    plh_group_scatter into Theta.  A trial is judged for the group as a whole: one member whose integration failed rejects it.  Bounds are then scalars or [n_groups] arrays,
    and every array of the result but theta has n_groups rows (EnsembleFitResult).
    Returns an EnsembleFitResult."""
    keys = list(keys)
    if len(keys) < 1 or len(keys) > cap.LSQ_MAX_SENS:
        raise ValueError("fit_ensemble fits 1 .. %d keys per call (%d given)" % (cap.LSQ_MAX_SENS, len(keys)))
    for kname in keys:
        if kname not in p.θ_keys:
            raise ValueError("fit_ensemble: %r is not a parameter of this model's theta" % (kname,))
    if len(set(keys)) != len(keys):
        raise ValueError("fit_ensemble: a key given twice")
    given = [c for c, d in (("V", V_data), ("I", I_data), ("T_avg", T_avg_data)) if d is not None]
    if not given:
        raise ValueError("fit_ensemble needs the data of at least one channel: V_data, I_data or T_avg_data")
    for what, dct in (("bounds", bounds), ("transform", transform)):
        for kname in (dct or {}):
            if kname not in keys:
                raise ValueError("fit_ensemble: %s names %r, which is not among the keys" % (what, kname))
    tf = np.zeros(len(keys), np.int32)
    for kname, v in (transform or {}).items():
        if v not in ("log", "linear"):
            raise ValueError("fit_ensemble: transform of %r must be 'log' or 'linear', not %r" % (kname, v))
        tf[keys.index(kname)] = cap.LM_LOG if v == "log" else cap.LM_LINEAR
    if max_iter < 1 or check_every < 1:
        raise ValueError("fit_ensemble: max_iter and check_every must be >= 1")
    lmo = cap.LMOpts(**(lm or {}))
    n, nth, k = Theta0.shape[0], Theta0.shape[1], len(keys)
    cols = np.ascontiguousarray([p.θ_keys.index(kname) for kname in keys], dtype=np.int32)
    off = None if groups is None else group_offsets(groups, n)
    nf = n if off is None else len(off) - 1                              # the number of least-squares problems: cells, or groups
    if device:
        import torch
        dev = Theta0.device
        Theta = Theta0.to(dtype=torch.float64).contiguous().clone()
        mk = lambda shape, dt=torch.float64, fill=float("nan"): torch.full(shape, fill, dtype=dt, device=dev)
        mki = lambda shape: torch.zeros(shape, dtype=torch.int32, device=dev)

        def host(a):                                                     # (the launch stream need not be torch's current one: it is waited for, then the copy is plain)
            cap.check(p._lib, p._lib.plh_synchronize(p._h, stream), "plh_synchronize")
            return a.cpu().numpy().copy()
        kind = cap.PLH_DEVICE
    else:
        Theta = np.array(Theta0, dtype=np.float64, order="C", copy=True)
        mk = lambda shape, dt=np.float64, fill=np.nan: np.full(shape, fill, dt)
        mki = lambda shape: np.zeros(shape, np.int32)
        host = lambda a: np.array(a, copy=True)
        kind = cap.PLH_HOST
    # bounds: [k] on the host when every one is a scalar, else [n, k] where Theta lives
    blo, bhi = np.full(k, -np.inf), np.full(k, np.inf)
    per_cell = any(b is not None and np.ndim(b.cpu() if hasattr(b, "cpu") else b) > 0 for pair in (bounds or {}).values() for b in pair)
    if per_cell:
        blo, bhi = np.full((nf, k), -np.inf), np.full((nf, k), np.inf)
    for kname, pair in (bounds or {}).items():
        if len(pair) != 2:
            raise ValueError("fit_ensemble: bounds[%r] must be (lo, hi)" % (kname,))
        for dst, b in zip((blo, bhi), pair):
            if b is None:
                continue
            b = np.asarray(b.cpu() if hasattr(b, "cpu") else b, dtype=np.float64)
            if b.ndim and b.shape != (nf,):
                raise ValueError("fit_ensemble: a bound of %r must be a scalar or [%s]" % (kname, "n_cells" if off is None else "n_groups"))
            dst[..., keys.index(kname)] = b
    if per_cell and device:
        lo_a, hi_a = torch.as_tensor(blo).to(dev), torch.as_tensor(bhi).to(dev)
    else:
        lo_a, hi_a = np.ascontiguousarray(blo), np.ascontiguousarray(bhi)
    # the number of data of every problem, for the residual variance of covariance(): the (channel, time) pairs whose weight is not 0 (a channel without weights: every
    # time), summed over the members of a group; counted once, where the weights live
    n_q = int(np.asarray(t.cpu() if hasattr(t, "cpu") else t).size)
    xp = torch if device else np
    n_data = mki((n,))
    for d, w_ in ((V_data, weights), (I_data, I_weights), (T_avg_data, T_avg_weights)):
        if d is None:
            continue
        if w_ is None:
            n_data = n_data + n_q
            continue
        if device:
            w_ = (w_ if isinstance(w_, torch.Tensor) else torch.as_tensor(np.asarray(w_, dtype=np.float64))).to(dev)
        else:
            w_ = np.asarray(w_, dtype=np.float64)
        n_data = n_data + (w_ != 0).sum(-1).to(torch.int32) if device else n_data + (w_ != 0).sum(-1).astype(np.int32)
    if off is not None:
        cs = xp.cumsum(n_data, 0)
        first_, last_ = (torch.as_tensor(off[:-1].astype(np.int64)).to(dev), torch.as_tensor(off[1:].astype(np.int64) - 1).to(dev)) if device else (off[:-1], off[1:] - 1)
        n_data = cs[last_] - cs[first_] + n_data[first_]
    n_data = n_data.to(torch.int32).contiguous() if device else np.ascontiguousarray(n_data, dtype=np.int32)
    st = dict(theta_cur=mk((nf, k)), cost_cur=mk((nf,)), grad_cur=mk((nf, k)), JtJ_cur=mk((nf, k, k)), lam=mk((nf,)), pred=mk((nf,)), state=mki((nf,)), n_accept=mki((nf,)), n_reject=mki((nf,)))
    n_running = mki((1,))
    LTheta, gfit = Theta, None                                           # the matrix plh_lm_step works on: one row per problem
    if off is not None:                                                  # the groups' rows (their first members') and the groups' fit: allocated once, before the loop
        first = off[:-1].astype(np.int64)
        LTheta = Theta[torch.as_tensor(first).to(dev)].contiguous() if device else np.ascontiguousarray(Theta[first])
        gfit = EnsembleFit(keys, given)
        gfit.cost, gfit.grad, gfit.JtJ, gfit.status = mk((nf,)), mk((nf, k)), mk((nf, k, k)), mki((nf,))
    ext = None
    if device and stream is not None and int(stream) != torch.cuda.current_stream(dev).cuda_stream:
        ext = torch.cuda.ExternalStream(int(stream), device=dev)         # (made on torch's current stream, used on the launch stream: as in _integrate)
        ext.wait_stream(torch.cuda.current_stream(dev))
        for v in [Theta, n_running, lo_a, hi_a, n_data] + list(st.values()) + ([] if off is None else [LTheta, gfit.cost, gfit.grad, gfit.JtJ, gfit.status]):
            if hasattr(v, "record_stream"):
                v.record_stream(ext)
    res = EnsembleFitResult(keys)
    res.history = [] if history else None
    lib, h = p._lib, p._h

    def scatter():                                                       # the keys of every group's row into the rows of its members
        cap.check(lib, lib.plh_group_scatter(h, n, nf, off.ctypes.data, nth, k, cols.ctypes.data, cap.ptr(LTheta), cap.ptr(Theta), kind, stream), "plh_group_scatter")

    if off is not None:
        res.group_off = off
        scatter()                                                        # (the start is consistent by construction)

    def iteration(phase):
        ens = simulate_ensemble(p, Theta, protocol, SOC=SOC, opts=opts, device=device, stream=stream, max_points=max_points, YP=False, sens=keys, sens_outputs=tuple(given))
        fit = ens.lsq(t, V_data, weights, interp_bc=interp_bc, I_data=I_data, I_weights=I_weights, T_avg_data=T_avg_data, T_avg_weights=T_avg_weights)
        if off is not None:
            member = fit
            _lsq_group(p, off, member, gfit, stream)
            fit = gfit
        if history:
            rec = dict(phase=phase, theta_before=host(LTheta), cost=host(fit.cost), grad=host(fit.grad), JtJ=host(fit.JtJ), status=host(fit.status), before={a: host(v) for a, v in st.items()})
            if off is not None:
                rec["member"] = dict(cost=host(member.cost), grad=host(member.grad), JtJ=host(member.JtJ), status=host(member.status))
        cap.check(lib, lib.plh_lm_step(h, nf, nth, cap.ptr(LTheta), k, cols.ctypes.data, tf.ctypes.data, cap.ptr(lo_a), cap.ptr(hi_a), 1 if per_cell else 0,
                                       cap.ptr(fit.cost), cap.ptr(fit.grad), cap.ptr(fit.JtJ), cap.ptr(fit.status),
                                       cap.ptr(st["theta_cur"]), cap.ptr(st["cost_cur"]), cap.ptr(st["grad_cur"]), cap.ptr(st["JtJ_cur"]), cap.ptr(st["lam"]), cap.ptr(st["pred"]),
                                       cap.ptr(st["state"]), cap.ptr(st["n_accept"]), cap.ptr(st["n_reject"]), C.byref(lmo), phase, cap.ptr(n_running), kind, stream), "plh_lm_step")
        res.n_iter += 1
        if off is not None:
            scatter()
        if history:
            rec.update(theta_after=host(LTheta), after={a: host(v) for a, v in st.items()}, n_running=int(host(n_running)[0]))
            if off is not None:
                rec["Theta"] = host(Theta)
            res.history.append(rec)

    read_running = lambda: int(host(n_running)[0])                       # (device=True: the loop's only synchronisation)
    iteration(cap.LM_FIRST)
    running = read_running() if check_every == 1 else 1
    for it in range(1, max_iter):
        if running == 0:
            break
        iteration(cap.LM_STEP)
        if it % check_every == 0:
            running = read_running()
    if running != 0 and read_running() != 0:
        iteration(cap.LM_LAST)
    res.theta, res.cost, res.grad, res.JtJ = Theta, st["cost_cur"], st["grad_cur"], st["JtJ_cur"]
    res.state, res.lam, res.n_accept, res.n_reject = st["state"], st["lam"], st["n_accept"], st["n_reject"]
    res.theta_cur, res.n_data = st["theta_cur"], n_data
    res._p, res._tf, res._lo, res._hi, res._stream = p, tf, lo_a, hi_a, stream
    res._protocol, res._SOC, res._opts, res._max_points, res._device, res._sens_outputs, res._interp_bc = protocol, SOC, opts, max_points, device, tuple(given), interp_bc
    return res


def theta_matrix(p, n_cells, overrides=None):
    """[n_cells, n_theta] matrix of the model's current θ, with per-cell overrides {key: array[n_cells]}."""
    Th = np.tile(p.theta_vector(), (n_cells, 1))
    if overrides:
        for k, v in overrides.items():
            Th[:, p.θ_keys.index(k)] = v
    return Th


class HostPipeline:
    """Host-inclusive ensemble calls at kernel rate: `depth` in-flight calls over pinned host buffers (plh_host_alloc) and one HIP stream each
    (PLH_HOST_ASYNC): call k+1's parameter upload and kernel overlap call k's device-to-host copies.  This is SURVEY.md 8(d)'s measurement shape --
    parameters start in host memory, per-cell summaries and sampled outputs end in host memory -- without paying the copies serially.

        pipe = HostPipeline(p, n_cells, protocol, max_points=256)
        for k, Theta in enumerate(batches):
            slot = k % pipe.depth
            if k >= pipe.depth: consume(pipe.wait(slot))          # results of call k - depth
            pipe.submit(slot, Theta)
    """

    def __init__(self, p, n_cells, protocol, SOC=1.0, opts=None, max_points=256, depth=2, streams=None, sections=None):
        import torch                                                   # streams only (plumbing)
        self.p, self.n, self.depth = p, int(n_cells), int(depth)
        self.runs, self.names = make_protocol(p, protocol, n_cells)
        self.arr = (cap.Run * len(self.runs))(*self.runs)
        self.opts = _opts_struct(opts or p.opts, p)
        self.mp = int(max_points)
        self._torch_streams = streams or [torch.cuda.Stream() for _ in range(self.depth)]
        self.streams = [s.cuda_stream for s in self._torch_streams]
        lib = p._lib
        N, P, nr = p.N.tot, len(p.θ_keys), len(self.runs)
        self._blocks = []

        def pinned(shape, dtype):
            dt = np.dtype(dtype); nbytes = int(np.prod(shape)) * dt.itemsize
            ptr = C.c_void_p()
            cap.check(lib, lib.plh_host_alloc(C.byref(ptr), nbytes), "plh_host_alloc")
            self._blocks.append(ptr)
            return np.frombuffer((C.c_char * nbytes).from_address(ptr.value), dtype=dt).reshape(shape)
        # sections = (...): every slot also carries Y_sel [cell, point, n_sel_total] (pinned), see simulate_ensemble; self.sel_ind[name] is a section's slice of the row
        self.sel, self.sel_ind = _resolve_sections(p, sections)
        self._sel_arr = None if self.sel is None else np.ascontiguousarray(self.sel, dtype=np.int32).reshape(-1, 2)
        self.slots = []
        for _ in range(self.depth):
            b = dict(theta=pinned((self.n, P), np.float64), soc=pinned((self.n,), np.float64), t=pinned((self.n, self.mp), np.float64), V=pinned((self.n, self.mp), np.float64),
                     n_pts=pinned((self.n,), np.int32), run_info=pinned((self.n, nr), cap.RUN_INFO_DTYPE), counters=pinned((self.n,), cap.COUNTERS_DTYPE))
            b["soc"][:] = float(SOC)
            out = cap.Outputs()
            out.max_pts = self.mp
            out.t, out.V, out.n_pts = cap.ptr(b["t"]), cap.ptr(b["V"]), cap.ptr(b["n_pts"])
            out.run_info, out.counters = cap.ptr(b["run_info"]), cap.ptr(b["counters"])
            if self.sel is not None:
                b["Y_sel"] = pinned((self.n, self.mp, max(int(self._sel_arr[:, 1].clip(0).sum()), 1)), np.float64)
                out.n_sel, out.sel, out.Y_sel = len(self._sel_arr), self._sel_arr.ctypes.data_as(C.POINTER(C.c_int)), cap.ptr(b["Y_sel"])
            b["out"] = out
            self.slots.append(b)

    def submit(self, slot, Theta):
        b = self.slots[slot]
        np.copyto(b["theta"], Theta)                                   # the caller's parameters into the pinned block (what a Julia host would own directly)
        lib, h = self.p._lib, self.p._h
        cap.check(lib, lib.plh_integrate(h, self.n, cap.ptr(b["theta"]), cap.ptr(b["soc"]), None, None, len(self.runs), self.arr, C.byref(self.opts),
                                         C.byref(b["out"]), cap.PLH_HOST_ASYNC, self.streams[slot]), "plh_integrate")

    def wait(self, slot):
        cap.check(self.p._lib, self.p._lib.plh_synchronize(self.p._h, self.streams[slot]), "plh_synchronize")
        return self.slots[slot]

    def close(self):
        for s in range(self.depth):
            self.p._lib.plh_synchronize(self.p._h, self.streams[s])
        for ptr in self._blocks:
            self.p._lib.plh_host_free(ptr)
        self._blocks = []
        self.slots = []

/*
 * petlion_hip.h -- C ABI of the MI355X-native DFN/P2D time-stepping path (libpetlion_hip.so).
 *
 * This is the drop-in boundary a Julia host binds with `ccall` (bindings/julia/PetlionHIP.jl).
 * Every entry point names the reference interface it replaces; citations are relative to the reference repository
 * (MarcBerliner/PETLION.jl @ v1.0.6).  Plain C, caller-owned arrays, no callbacks, no exceptions across the boundary.
 *
 * Conventions
 *   - all reals are IEEE fp64 (the reference is Float64 everywhere, src/structures.jl:337).
 *   - batched arrays are cell-major: X[cell*stride + k]  (one cell's vector is contiguous, like the reference's Vector).
 *   - `ptr_kind`: PLH_HOST  = the arrays are host memory (the library stages them through the device);
 *                 PLH_DEVICE = the arrays already live in this GPU's HBM (no copies; asynchronous on `stream`).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - return value: 0 ok; <0 API misuse / HIP failure (PLH_E_*).  Per-cell outcomes are reported in `status`/`flag` arrays
 *     using the reference's exit flags 0..11 (src/checks.jl:6,40,47,66,73,90,97,116,152,175,194,217) and negative codes
 *     for the reference's error() paths.
 *   - a handle is used by one host thread at a time (the reference model object is not re-entrant either,
 *     src/external.jl:135-139); different handles / GPUs may be used concurrently.  One handle may have launches in flight on several
 *     streams: the per-launch device workspaces (previous-point scratch, protocol copy, staging blocks) are kept per stream.
 *   - a handle is bound to one HIP device (plh_model_desc.device); every call switches to it and restores the caller's device.
 */
#ifndef PETLION_HIP_H
#define PETLION_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PLH_HOST 0
#define PLH_DEVICE 1
#define PLH_HOST_ASYNC 2   /* plh_integrate only: the arrays are PINNED host memory from plh_host_alloc; the call enqueues the host-to-device copies, the kernel and
                              the device-to-host copies on `stream` and returns -- the outputs are valid after plh_synchronize(m, stream).  Two streams and two
                              buffer sets overlap one call's copies with the next call's kernel (the host-inclusive pipeline of bench.py). */

#define PLH_E_ARG (-1)          /* invalid argument */
#define PLH_E_UNSUPPORTED (-2)  /* model option outside the hot-path scope */
#define PLH_E_HIP (-3)          /* HIP runtime failure (no GPU, out of memory, launch failure) */

/* chemistries: reference src/params.jl:5-289 (LCO + LiC6), 295-507 (NMC + LiC6_NMC), 514-849 (NMC_LGM50 + LiC6_LGM50) */
#define PLH_CHEM_LCO_LIC6 0
#define PLH_CHEM_NMC_LIC6 1
#define PLH_CHEM_LGM50 2      /* NMC_LGM50 + LiC6_LGM50 (Chen et al. 2020), reference src/params.jl:514-849: own OCVs, D_eff(c_e), K_eff(c_e) */

/* operating modes = the control row of the DAE (reference src/physics_equations/input_methods.jl:9,40,182-189,
 * src/physics_equations/scalar_residual.jl:167-172) */
#define PLH_MODE_I 0   /* current, C-rate:      Y[I] - value                      */
#define PLH_MODE_V 1   /* voltage, V:           Phi_s[1] - Phi_s[end] - value     */
#define PLH_MODE_DT 2  /* dT_avg/dt, K/s:       value - sum_i w_i YP[T_i] / L     (temperature models only) */
#define PLH_MODE_P 3   /* power, W/m^2:         Y[I] I1C (Phi_s[1] - Phi_s[end]) - value   (method_P, input_methods.jl:80-111) */
#define PLH_MODE_ETA_P 4 /* plating overpotential, V: Phi_s.n[1] - Phi_e.n[1] - value     (method_η_p, input_methods.jl:113-152) */
#define PLH_N_MODES 5   /* the modes above: the ones with an exported Jacobian pattern (plh_jac_pattern, plh_residual, ...) */
#define PLH_MODE_DSTATE 6 /* rate of change of ONE differential state held at value: value - YP[index] = 0 (reference dc_s_p_max / dc_s_p_min / dc_s_n_max / dc_s_n_min / dc_e_max /
                            dc_e_min, input_methods.jl:190-247: state_deriv_func(ind) as a run_residual).  plh_run.dstate (PLH_DSTATE_*) says which state: chosen per cell from the
                            state at the START of the run (the extreme surface concentration of an electrode / electrolyte concentration at the end of the previous run), so the run
                            must continue a solution (not the first run of a protocol unless Y_init is given).  PLH_VAL_CONST or PLH_VAL_HOLD (= 0).  The consistent initialisation
                            uses the row with YP[index] replaced by its differential equation (scalar_residual.jl:335-362).  plh_integrate / plh_ensemble_run only. */
#define PLH_DSTATE_CS_P_MAX 1
#define PLH_DSTATE_CS_P_MIN 2
#define PLH_DSTATE_CS_N_MAX 3
#define PLH_DSTATE_CS_N_MIN 4
#define PLH_DSTATE_CE_MAX 5
#define PLH_DSTATE_CE_MIN 6
#define PLH_MODE_RES 5 /* user-defined control residual (reference method_res, input_methods.jl:155-175; run_residual, scalar_residual.jl:172):  value - f(t, Y, theta) = 0 with
                          the closure f as PLH_VAL_EXPR and its derivative programs (n_dcol >= 1: the reference always differentiates this row, scalar_residual.jl:262-274);
                          plh_integrate / plh_ensemble_run only.  Closures of YP (the dc_s_*, dc_e_* modes are such) are not supported. */

/* plh_model_desc.solid_diffusion / thermodynamic_factor / rxn: the model options of petlion(...; solid_diffusion, thermodynamic_factor, rxn_p, rxn_n)
 * (reference src/params.jl:140-172; equations: residuals.jl:108-127,237-258, aux...jl:193-248, custom_functions.jl:177-203, 212-298) */
#define PLH_SD_FICKIAN 0     /* :Fickian with Fickian_method = :finite_difference (N_r radial nodes per particle) */
#define PLH_SD_QUADRATIC 1   /* :quadratic  -- one volume-averaged concentration per particle, c_s* = c_avg - Rp/(5 D_s) j */
#define PLH_SD_POLYNOMIAL 2  /* :polynomial -- c_avg and the flux moment Q per particle (Subramanian et al.) */
#define PLH_TF_LINEAR 0      /* thermodynamic_factor_linear: nu = 1 */
#define PLH_TF_NONLINEAR 1   /* thermodynamic_factor: nu(c_e, T) = 0.601 - 0.24 (c_e/1000)^0.5 + 0.982 (1 - 0.0052 (T - 293)) (c_e/1000)^1.5 */
#define PLH_RXN_BV 0         /* rxn_BV in both electrodes */
#define PLH_RXN_MHC 1        /* rxn_MHC in both electrodes (Marcus-Hush-Chidsey; theta gains λ_MHC_p, λ_MHC_n) */

/* plh_model_desc.precision */
#define PLH_PREC_F64 0    /* everything fp64 (default; the parity configuration) */
#define PLH_PREC_MIXED 1  /* block-Thomas factors and particle resolvents stored in fp32 in LDS; states, residuals, Jacobian entries, time, error control fp64 */
#define PLH_PREC_F64_REFORDER 2 /* everything fp64, and the finite-volume rows (c_e, Phi_e, heat conduction) evaluated in the reference's OPERATION ORDER: matrix form A x - f with
                                   every product rounded before the sum (src/physics_equations/residuals.jl:6-106, 554-654, 299-489) instead of the default build's
                                   conservative edge-flux / difference form.  Same equations and Jacobian; the rows carry the reference's evaluation rounding, so the
                                   integrator's step / order decisions in :hold legs follow the reference's more closely.  LCO isothermal and LCO with
                                   temperature. */

/* how `value` is obtained (reference input_methods.jl:11-30,53-63; model_evaluation.jl:165-170) */
#define PLH_VAL_CONST 0
#define PLH_VAL_HOLD 1  /* :hold  -- the value reached at the end of the previous run */
#define PLH_VAL_REST 2  /* :rest  -- I = 0, all bound checks skipped (src/checks.jl:12,388) */
#define PLH_VAL_TABLE 3   /* time-dependent input from plh_run.tab_t / tab_v */
#define PLH_VAL_EXPR 4    /* input = a closure f(t, Y, YP, theta) given as a postfix program (PLH_OP_*) in plh_run.tab_t (opcodes) / tab_v (operands) */
/* Postfix programs for PLH_VAL_EXPR: the form in which a reference input closure `I = (t, Y, YP, p) -> ...` (scalar_residual.jl:169-170, input_methods.jl:159-176) crosses the
   C ABI.  Instruction k is (opcode tab_t[k], operand tab_v[k]); the machine is a stack of at most 16 doubles, the program must leave exactly one value.  Operands: the constant
   for CONST, a 0-based state index for Y / YP, a 0-based position in the model's theta_keys for THETA; unused otherwise.  The closure is evaluated with the current iterate inside
   every residual evaluation of the run (also during the consistent initialisation), like run.func in scalar_residual!.
   Derivatives (plh_run.n_dcol / dcol / dofs): the reference differentiates a closure of the state symbolically and puts the row d(method - f)/dY into the Newton matrix
   (differentiate_residual_func, scalar_residual.jl:276-416).  The caller does the same differentiation (it holds the expression) and passes, for each state column dcol[k]
   the closure reads, a program for d f / d Y[dcol[k]]: instructions [dofs[k], dofs[k+1]) of the SAME tab_t / tab_v arrays (dofs[0] >= n_tab).  A column dcol[k] = N + i
   (N = n_states, i a DIFFERENTIAL state) is d f / d YP[i]: it enters the integration row times cj, and the consistent-initialisation row through the differential equation of
   state i (YP[i] -> rhs_i(Y), as the reference substitutes there, scalar_residual.jl:335-362; the closure itself is then evaluated with YP = rhs(Y)).  The device evaluates the
   programs at every Jacobian refresh and solves with the general control row (one extra structured solve per factorisation, two dot products per solve).  n_dcol = 0 is the
   reference's own fallback for closures it cannot differentiate (scalar_residual.jl:248-274, _get_method_funcs_no_differentiation): same converged states, other Newton steps. */
#define PLH_OP_CONST 0
#define PLH_OP_T 1
#define PLH_OP_Y 2
#define PLH_OP_YP 3
#define PLH_OP_THETA 4
#define PLH_OP_ADD 5
#define PLH_OP_SUB 6
#define PLH_OP_MUL 7
#define PLH_OP_DIV 8
#define PLH_OP_NEG 9
#define PLH_OP_SIN 10
#define PLH_OP_COS 11
#define PLH_OP_EXP 12
#define PLH_OP_LOG 13
#define PLH_OP_SQRT 14
#define PLH_OP_POW 15
#define PLH_OP_ABS 16
#define PLH_OP_MIN 17
#define PLH_OP_MAX 18
#define PLH_OP_LT 19      /* a b -> (a < b) as 1.0 / 0.0 ; LE, GT, GE alike */
#define PLH_OP_LE 20
#define PLH_OP_GT 21
#define PLH_OP_GE 22
#define PLH_OP_SELECT 23  /* c a b -> (c != 0 ? a : b)   (ifelse) */
#define PLH_OP_TANH 24
#define PLH_N_OPS 25
#define PLH_EXPR_STACK 16
#define PLH_MAX_DCOL 60     /* most state columns a closure's derivative programs may name (plh_run.n_dcol) */

/* per-cell status beyond the reference's exit flags */
#define PLH_FLAG_RUNNING (-1)
#define PLH_ERR_INIT (-11)      /* "Could not initialize DAE in 100 iterations", src/model_evaluation.jl:456 */
#define PLH_ERR_STALL (-12)     /* "Model failed to converge at t = ...", src/checks.jl:233,236 */
#define PLH_ERR_MAXITERS (-13)  /* "Reached max iterations", src/checks.jl:239 */
#define PLH_ERR_OUTPUT_FULL (-14)
#define PLH_FLAG_STOP_FUNCTION 12   /* the run ended on the caller's stop function (plh_opts.stop_ops): the reference's opts.stop_function hook, src/checks.jl:26 */

typedef struct plh_model_s* plh_model_t;

/* mirrors the structural keyword arguments of petlion(cathode; N_p, ..., temperature, aging)
 * (reference src/params.jl:119-174, src/external.jl:2-18) */
typedef struct {
  int chemistry;                                  /* PLH_CHEM_* */
  int N_p, N_s, N_n, N_a, N_z, N_r_p, N_r_n;      /* reference defaults: 10 each */
  int temperature;                                /* 0/1 */
  int aging_SEI;                                  /* 0/1 */
  int real_bytes;                                 /* 8: states, residuals, time and tolerances are fp64 (the reference is Float64 everywhere) */
  int precision;                                  /* PLH_PREC_* : storage precision of the LDS-resident Newton-matrix factors (config C5's fp32 leg) */
  int device;                                     /* HIP device ordinal the handle binds to (every call of the handle runs there); -1 = the device that is
                                                     current when plh_model_create is called */
  int solid_diffusion;                            /* PLH_SD_* */
  int thermodynamic_factor;                       /* PLH_TF_* */
  int rxn;                                        /* PLH_RXN_* */
  int waves_per_cell;                             /* 0 or 1: one wavefront integrates one cell (every variant); 2: two wavefronts per cell -- wave 1 owns the particle rows and
                                                     runs next to wave 0's finite-volume work (LCO isothermal Fickian fp64 only).  Same algorithm, same results to rounding. */
} plh_model_desc;

/* reference boundary_stop_conditions (src/structures.jl:237-250); NaN disables a bound */
typedef struct {
  double V_max, V_min, SOC_max, SOC_min, T_max, c_s_n_max, I_max, I_min, eta_plating_min, c_e_min, dfilm_max;
} plh_bounds;

/* one run of a protocol == one simulate()/simulate!() call (src/model_evaluation.jl:11-97) */
typedef struct {
  int mode;        /* PLH_MODE_* */
  int value_kind;  /* PLH_VAL_*  */
  double value;
  double tf;       /* run length in run-local time; reference default 1e6 (model_evaluation.jl:13) */
  plh_bounds bounds;
  /* PLH_VAL_TABLE: the input is a function of the run-local time (reference run_function: I = t -> ..., scalar_residual.jl:169-170) given as a
     piecewise-linear table; a repeated knot time is a jump (right-continuous), the last value holds beyond the last knot.  The arrays are HOST
     memory like the protocol itself (plh_integrate stages them).  List jump times in plh_opts.tdiscon as with the reference's `tdiscon`. */
  /* PLH_VAL_EXPR: n_tab instructions, tab_t[k] = opcode (PLH_OP_*, stored as a double), tab_v[k] = operand (see above); HOST arrays, staged like a table. */
  int n_tab;
  int closure_id;  /* written by the library (the caller's value is ignored): which compiled closure of an attached closure library this run uses, -1 = interpreted
                      (plh_model_attach_closure_library).  Sits in what was padding: no other field moved. */
  const double* tab_t; const double* tab_v;
  /* ensemble axis of the protocol itself: per-cell input value (PLH_VAL_CONST only, e.g. a C-rate sweep) and per-cell run length, [n_cells] HOST
     arrays staged by plh_integrate; NULL = every cell uses `value` / `tf`.  (New: the reference runs one cell per simulate() call.) */
  const double* value_cell; const double* tf_cell;
  /* PLH_VAL_EXPR of the state: derivative programs of the control row (see PLH_VAL_EXPR above); HOST arrays, dcol[n_dcol] 0-based columns in ascending order (Y columns, then
     N + i for YP of differential states), dofs[n_dcol + 1] instruction offsets into tab_t / tab_v.  n_dcol = 0: no differentiation. */
  int n_dcol;
  int dstate;      /* PLH_MODE_DSTATE: PLH_DSTATE_* ; 0 otherwise */
  const int* dcol; const int* dofs;
} plh_run;

/* reference options_simulation (src/structures.jl:266-285), the numerical subset */
typedef struct {
  double abstol, reltol, abstol_init, reltol_init;   /* reference defaults 1e-6, 1e-3, =abstol, =reltol */
  int maxiters;                                      /* 10000 */
  int check_bounds, interp_final;                    /* 1, 1 */
  int max_order;                                     /* BDF order cap, 5 */
  int jac_every_step;                                /* 0: IDA's Jacobian-reuse policy */
  double init_step;                                  /* 0: IDA's automatic h0 = 0.5/||y'||_wrms; >0: IDASetInitStep (src/checks.jl:231) */
  int n_tdiscon; const double* tdiscon;              /* opts.tdiscon (src/structures.jl:279), any length, HOST array like the protocol (staged by
                                                        plh_integrate): tstops at tdiscon - reltol/2 (model_evaluation.jl:295-297) */
  int refine;                                        /* 0 (default): plain structured solves.  n > 0: n steps of iterative refinement of every linear solve
                                                        (init Newton and corrector) against the factored matrix -- the parity mode: the solution no longer
                                                        depends on the elimination order (structured here, KLU's in the reference) beyond ~1e-13 */
  int n_tstops; const double* tstops;                /* opts.tstops (src/structures.jl:278, model_evaluation.jl:292-294): times, in run-local time, the integrator must hit
                                                        exactly (a saved point lands on each); any length, HOST array staged like tdiscon; applies to every run of the protocol */
  int yp_alg_zero;                                   /* 0 (default): newtons_method! hands the integrator its finite-difference estimate of the algebraic derivatives
                                                        (src/model_evaluation.jl:462-477).  1: the integrator starts with YP_alg = 0, as the package version that produced the
                                                        reference's example notebooks did -- with it the printed step history of examples/model_inputs_and_outputs.ipynb
                                                        (121 saved points, sol.V[1:13], sol.c_e[1:5]) is reproduced to 1e-8 (tests/golden/notebook_kats.json) */
  /* opts.stop_function (src/structures.jl:283, called after the eleven built-in checks at every accepted step, src/checks.jl:26; simulate(...; stop_function), src/model_evaluation.jl:32).
     A Julia closure cannot cross the C ABI; its expression can: ONE postfix program g(t, Y, YP, theta) in the PLH_OP_* vocabulary of PLH_VAL_EXPR (n_stop instructions, opcodes in
     stop_ops stored as doubles, operands in stop_args; HOST arrays staged like tdiscon; t = run-local time).  The run ends when g > 0 (g - 0 > eps with the eps of the built-in checks:
     reltol while t < 1 s, else 0), exit flag PLH_FLAG_STOP_FUNCTION, with the interpolation fraction g_prev / (g_prev - g) entering the same linear back-interpolation as the
     built-in bounds (interp_final_points!, src/model_evaluation.jl:369-382; the smallest fraction of all checks that fired wins, as in the reference).  Skipped in :rest runs and
     with check_bounds = 0, like every other check.  n_stop = 0: none. */
  int n_stop; const double* stop_ops; const double* stop_args;
} plh_opts;

/* per-cell, per-run summary == run_info + the printed summary (src/structures.jl:40-44, 678-746) */
typedef struct {
  int flag;          /* exit flag 0..11 or PLH_ERR_* */
  int iterations;    /* run.info.iterations */
  double t_end, V, I, SOC, T_avg;
} plh_run_info;

/* per-cell device counters: the roofline contract of SURVEY.md 8(d) */
typedef struct {
  long long n_steps, n_res, n_jac, n_fact, n_solve, n_newton, n_errfail, n_convfail, sum_kp2, n_init_iters;
  long long cyc[8];   /* shader cycles per phase (residual, jacobian+factor, solve, newton vector ops, step control, init, output, total);
                         filled only by the profiling build (-DPL_PHASE_TIMERS), zero otherwise */
} plh_counters;

/* outputs of plh_integrate; any pointer may be NULL.  Saved points are the reference's per-step pushes of
 * set_vars! (src/save_outputs.jl:11-40): t = 0 of every run + every accepted step; the last point of a run that ended on
 * a bound is the back-interpolated one (src/model_evaluation.jl:369-382).
 * What a blocking PLH_HOST call does to the caller's arrays: an array that is not requested (NULL) is not written.  The per-point arrays (t ... T_avg, Y_all, Y_sel)
 * receive results only up to the longest trajectory of the call: entries at columns >= max over the cells of n_pts -- like the entries beyond n_pts[cell] of any row,
 * which no pointer kind defines -- are not copied back.  But the pages of a requested array are touched for the first time while the kernel runs, and that touch may
 * write ZERO bytes anywhere inside the array before the results arrive: a caller must not expect values it stored in a requested array to survive the call, beyond
 * the results or not.  (PLH_DEVICE and PLH_HOST_ASYNC write exactly what the kernel writes / copy every requested array back whole.) */
typedef struct {
  int max_pts;                      /* row stride of the per-point arrays */
  double *t, *V, *I, *SOC, *T_avg;   /* [n_cells][max_pts] */
  int* n_pts;                        /* [n_cells] */
  double *Y_final, *YP_final;        /* [n_cells][n_states] */
  plh_run_info* run_info;            /* [n_cells][n_runs] */
  plh_counters* counters;            /* [n_cells] */
  double* Y_all;                     /* [n_cells][max_pts][N] or NULL: every saved state vector (reference outputs = :all / sol.Y; 2.4 kB per point) */
  /* Selected state entries per saved point (reference outputs = (:t, :V, :c_e): solution_states_logic, src/outputs.jl:107-131; set_vars!, src/save_outputs.jl:11-40 keep
     the named states and nothing else).  sel holds n_sel pairs (start, len) of 0-based ranges of the state vector (plh_section gives the named ones), HOST memory like the
     protocol; the device writes, at exactly the saved points of t / V / ... / Y_all and with the same truncation at max_pts, only those entries, packed in the order
     given: Y_sel[cell][point][k], n_sel_total = sum of len entries per point, and the row of range i starts at the sum of the lengths before it.  Rules: 0 <= n_sel <= 16;
     every range has len >= 1 and lies inside [0, N); ranges may come in any order but may not overlap; Y_sel != NULL needs n_sel >= 1.  A violation is PLH_E_ARG (nothing is
     clamped).  Y_sel and Y_all may both be set: Y_sel then holds the bits of the corresponding columns of Y_all.  These fields are the last of the struct: a caller that
     zero-initialises plh_outputs gets the behaviour of a library without them.
     plh_integrate_sens carries Y_sel exactly as it carries Y_all (same saved points).  plh_ensemble_run takes no plh_outputs and returns no per-point array, neither Y_all
     nor Y_sel. */
  int n_sel;
  const int* sel;                    /* [n_sel][2] = (start, len), host memory */
  double* Y_sel;                     /* [n_cells][max_pts][n_sel_total] or NULL */
} plh_outputs;

/* ---- model handle: replaces petlion()'s generated-function bundle p.funcs (src/structures.jl:315-334) ---- */
int plh_model_create(const plh_model_desc* desc, plh_model_t* out);
void plh_model_destroy(plh_model_t m);
/* Other discretisations (reference src/params.jl:119-136: petlion(...; N_p, N_s, N_n, N_r_p, N_r_n, N_a, N_z)).  The kernels are compiled per grid, like the reference
   generates and caches its functions per model (generate_functions.jl:44-94): the built-in ones for the default 10 / 10 / 10 / 10, any other grid with 2 <= N_p, N_s, N_n,
   N_p + N_s + N_n <= 48, 10 <= N_r_p, N_r_n <= 16 (the two particle grids may differ) as a library built from csrc/variant_tu.hip (petlion.jl_amd/grids.py) and registered here BEFORE
   plh_model_create is called with those dimensions.  Registering the same path twice is a no-op; the library stays loaded for the life of the process. */
int plh_register_grid_library(const char* path);
int plh_n_states(plh_model_t m);     /* p.N.tot  */
int plh_n_diff(plh_model_t m);       /* p.N.diff */
int plh_n_theta(plh_model_t m);      /* length(θ_keys), src/generate_functions.jl:327-363 */
const char* plh_theta_key(plh_model_t m, int i);   /* UTF-8 names identical to the reference Symbols, sorted like θ_keys */
double plh_theta_default(plh_model_t m, int i);    /* chemistry defaults, src/params.jl */
int plh_lds_bytes(plh_model_t m);    /* LDS held by one cell (= one workgroup) of this variant: 160 kB / this = resident cells per CU */
/* p.ind (reference state_indices, src/external.jl:275-365): the named sections of the state vector in storage order, differential states
 * first.  Names are the reference's Symbols (c_e, c_s_avg, T, film, SOH, j, Φ_e, Φ_s, j_s, I); start is 0-based. */
int plh_n_sections(plh_model_t m);
int plh_section(plh_model_t m, int i, const char** name, int* start, int* len);
/* CSC pattern (0-based) of the full N x N Jacobian for a mode == [J_y_sp ; scalar row] of
 * _get_jacobian_combined (src/physics_equations/scalar_residual.jl:500-522).  colptr/rowval may be NULL to query nnz. */
int plh_jac_pattern(plh_model_t m, int mode, int* nnz, int* colptr, int* rowval);
/* CSC pattern (0-based, rows/columns relative to the block) of J_y_alg = J[N_diff : N-1, N_diff : N] at gamma = 0, the generated-function
 * J_y_alg! of seam 1 (src/generate_functions.jl:318-325): N_alg columns, N_alg - 1 rows (the control row is not generated). */
int plh_jac_alg_pattern(plh_model_t m, int mode, int* nnz, int* colptr, int* rowval);
const char* plh_last_error(void);
/* "hipcc=...;clang=...;flags=<hash>;src=<hash>" of this binary (the miscompile guard keys on it), and the number of HIP devices the library can see
 * (0: no GPU or no driver -- hosts use it to decide whether the kernel self-test can run, without a second GPU runtime in the process) */
const char* plh_build_info(void);
int plh_device_count(void);
/* sizeof / offsetof of every struct of this header as the library was compiled, for bindings that mirror them by hand (bindings/julia/PetlionHIP.jl,
 * the ctypes mirror of the tests): out[] receives, per struct in declaration order (plh_model_desc, plh_bounds, plh_run, plh_opts, plh_run_info,
 * plh_counters, plh_outputs): sizeof, number of fields, then the offset of each field.  Returns the number of ints written (or needed, if cap is short). */
int plh_abi_layout(int* out, int cap);

/* ---- batched evaluators (single-cell seam = n_cells 1, PLH_HOST) ---- */
/* initial_guess!(out, SOC, θ, X_applied)  (src/states_definition.jl:80-121): Y[cell][N], Y[I] = 0 */
int plh_initial_guess(plh_model_t m, int n_cells, const double* theta, const double* SOC, double* Y, int ptr_kind, void* stream);
/* R_full(res,t,Y,YP,p,run) = f_diff! ++ f_alg! ++ scalar_residual!  (scalar_residual.jl:558-583) */
int plh_residual(plh_model_t m, int n_cells, const double* theta, const double* Y, const double* YP, int mode, double value,
                 double* F, int ptr_kind, void* stream);
/* J_full(J,t,Y,YP,γ,p,run): nzval[cell][nnz] in the CSC order of plh_jac_pattern  (scalar_residual.jl:588-602) */
int plh_jacobian(plh_model_t m, int n_cells, const double* theta, const double* Y, const double* YP, double cj, int mode,
                 double* nzval, int ptr_kind, void* stream);
/* x = J_full \ b  with the structured (particle-resolvent + block-Thomas + border) solver that replaces KLU
 * (src/model_evaluation.jl:271, 417-428): b[cell][N] in, x out in place */
int plh_linear_solve(plh_model_t m, int n_cells, const double* theta, const double* Y, const double* YP, double cj, int mode,
                     double* b, int ptr_kind, void* stream);
/* the same with n_refine steps of iterative refinement against the factored matrix (plh_opts.refine of the integrator as a stand-alone evaluator) */
int plh_linear_solve_refined(plh_model_t m, int n_cells, const double* theta, const double* Y, const double* YP, double cj, int mode,
                             double* b, int n_refine, int ptr_kind, void* stream);
/* seam 1's split evaluators, with the argument lists of the five generated functions (src/generate_functions.jl:44-94, callers
 * scalar_residual.jl:558-602): f_diff!(out[N_diff], t, Y, YP, θ), f_alg!(out[N_alg - 1], t, Y, YP, θ) (no control row, generate_functions.jl:254),
 * J_y_alg!(nzval[nnz_alg], t, Y, YP, γ, θ) in the CSC order of plh_jac_alg_pattern.  J_y! is plh_jacobian minus the control row's entries
 * (a stub gathers them through the pattern, bindings/julia/SavedModelWriter.jl). */
int plh_residual_diff(plh_model_t m, int n_cells, const double* theta, const double* Y, const double* YP, double* out, int ptr_kind, void* stream);
int plh_residual_alg(plh_model_t m, int n_cells, const double* theta, const double* Y, const double* YP, double* out, int ptr_kind, void* stream);
int plh_jacobian_alg(plh_model_t m, int n_cells, const double* theta, const double* Y, const double* YP, int mode, double* nzval,
                     int ptr_kind, void* stream);
/* newtons_method! (src/model_evaluation.jl:430-480): Y in/out, YP out, status[cell] 0 or PLH_ERR_INIT, iters[cell] */
int plh_init_consistent(plh_model_t m, int n_cells, const double* theta, int mode, double value, double reltol_init,
                        double* Y, double* YP, int* status, int* iters, int ptr_kind, void* stream);

/* ---- the hot path: ensemble integrate == simulate()/simulate!() chains over independent cells ----
 * theta[cell][n_theta]; SOC0[cell]; one protocol (runs[n_runs], host memory) shared by all cells.
 * Y_init / t_init (both NULL for a new solution): continue a previous solution like simulate!(sol, p, ...)
 * (src/model_evaluation.jl:87-97, 206-209): Y_init[cell][n_states] = sol.Y[end], t_init[cell] = sol.t[end],
 * SOC0[cell] = sol.SOC[end]; the first run is then a continuation run (t0 = nextfloat(t_init), tstop at 1 s, :hold works).
 * Y_init WITHOUT t_init (t_init = NULL): simulate(p, ...; initial_states = Y) (src/model_evaluation.jl:15, 102-110, 193-199) -- a NEW solution (t0 = 0) that starts from
 * the caller's state vectors instead of initial_guess!; the algebraic states are re-solved by the consistent initialisation as always; SOC0[cell] = calc_SOC(Y)
 * (src/physics_equations/scalar_residual.jl:95-102: the anode's mean c_s_avg as a stoichiometry fraction), which the caller computes.
 * One wavefront integrates one cell for the whole protocol inside a single kernel launch. */
int plh_integrate(plh_model_t m, int n_cells, const double* theta, const double* SOC0, const double* Y_init, const double* t_init,
                  int n_runs, const plh_run* runs, const plh_opts* opts, const plh_outputs* out, int ptr_kind, void* stream);

/* ---- forward parameter sensitivities next to the states ("parameter-sensitivity (forward) outputs for estimation workflows").  The reference has no such
 * output: its users difference whole simulate() calls (one more simulate() per parameter and direction, with the adaptive step control's noise in the quotient).  Here
 * s_k(t) = dY(t)/d theta[sens_cols[k]] is integrated with the same steps and orders as Y by the staggered-direct method (one linear solve per parameter and accepted step with
 * the factorisation the integrator already holds; csrc/dfn_sens.h).  The guarantee on the states: the integrator takes THE SAME STEPS as plh_integrate -- every counter and
 * exit flag equal in every cell -- and Y, the saved points and run_info agree with it to ~1e-9 relative (measured: bit-identical in all but a few cells per thousand, those at
 * 1e-13 ... 1e-11: the sensitivity instantiation is another compilation of the step loop and may contract a sum differently).  The power-on self-test holds it to 1e-8.
 *   dY_dtheta[cell][k][n_states]  at the end of the last completed run (NaN for a cell whose protocol failed); may be NULL
 *   dV_dtheta[cell][k][max_pts]   at every saved point (the Jacobian of the voltage curve a least-squares fit needs); may be NULL
 *   sens_stat[cell][3]            corrector iterations spent; solves that did not reach the tolerance; steps whose corrector factored the step's own matrix because the
 *                                 integrator's (stale) one did not contract (the integrator's factorisation is saved and copied back: the states do not notice); may be NULL
 * Derivatives are with respect to the absolute value of the parameter.  Saved points at accepted steps / stop times: partial derivatives at fixed time.  The last point of a run
 * that ended on a bound is the reference's linear back-interpolation between the last two accepted points (model_evaluation.jl:369-382), whose fraction depends on theta through
 * the bounded quantity: its derivative -- and what the next run continues from -- includes that shift, i.e. it is the derivative of the end state as simulate() returns it
 * (dV/dtheta = 0 at a voltage bound).  Bounds on V, I, T_avg, eta_plating, c_s_n, c_e, and SOC under a constant current; an SOC bound in another mode or the dfilm bound
 * (a bound on YP) gives NaN from there on.  Protocols: constant or :rest inputs in the modes
 * I, V, P, eta_p, dT, any number of runs, new solutions only; everything else is PLH_E_UNSUPPORTED.  ptr_kind PLH_HOST or PLH_DEVICE (the call is synchronous). */
int plh_integrate_sens(plh_model_t m, int n_cells, const double* theta, const double* SOC0, int n_runs, const plh_run* runs, const plh_opts* opts,
                       const plh_outputs* out, int n_sens, const int* sens_cols, double* dY_dtheta, double* dV_dtheta, int* sens_stat, int ptr_kind, void* stream);
/* The same call with every per-point sensitivity channel the step loop can write.  A constant-voltage or V = :hold run has the voltage as its INPUT (dV/dtheta is 0 or a
 * constant there): the measured quantity of such a leg is the current; a thermocouple measures T_avg.
 *   dI_dtheta[cell][k][max_pts]      d I / d theta_k (I in C-rate, as plh_outputs.I) at every saved point; 0 in a run whose input is a constant current or :rest, and at the
 *                                    last point of a run that ended on a current bound (the derivative of the end state as simulate() returns it, like dV at a voltage bound)
 *   dT_avg_dtheta[cell][k][max_pts]  d T_avg / d theta_k (K) at every saved point: the temperature weighting of plh_outputs.T_avg applied to s_k.  Thermal models only:
 *                                    PLH_E_UNSUPPORTED on an isothermal model (T_avg is a constant of theta there; nothing is clamped or zero-filled)
 * Layout, NaN cases (a cell whose protocol failed, the unknown bound cases from there on; rows past n_pts stay NaN) and the definition at saved / interpolated end points are
 * dV_dtheta's.  Any member may be NULL, at least one of the four derivative arrays must be given.  Which channels are asked for does not change a bit of any other output:
 * one kernel serves every combination.  plh_integrate_sens(..., dY, dV, stat, ...) is this call with {dY, dV, NULL, NULL, stat}. */
typedef struct {
  double* dY_dtheta;
  double* dV_dtheta;
  double* dI_dtheta;
  double* dT_avg_dtheta;
  int* sens_stat;
} plh_sens_outputs;
int plh_integrate_sens_out(plh_model_t m, int n_cells, const double* theta, const double* SOC0, int n_runs, const plh_run* runs, const plh_opts* opts,
                           const plh_outputs* out, int n_sens, const int* sens_cols, const plh_sens_outputs* sens_out, int ptr_kind, void* stream);

/* ---- compiled input closures.  The reference compiles the user's closure and its symbolic derivatives into its generated control-row functions
 * (differentiate_residual_func, scalar_residual.jl:231-416); the built-in kernels interpret the PLH_VAL_EXPR programs instead.  A closure library is csrc/variant_tu.hip compiled once
 * more for this model's variant and grid with the programs of ONE protocol written out as straight-line device code (petlion.jl_amd/closure_lib.py writes the header and runs
 * hipcc; the library exports its variant table like a grid library, plus plh_closure_digest()).  After it is attached, plh_integrate uses its kernels for every call whose
 * PLH_VAL_EXPR programs (opcodes, operands, derivative columns, in protocol order) hash to the digest the library was built for, and the interpreter for every other call --
 * same arguments, same results (the expression is evaluated with the same operations in the same order).  One library per handle; attaching another replaces it;
 * path = NULL detaches (every closure is interpreted again: the host side verifies a freshly compiled library that way before it relies on it). */
int plh_model_attach_closure_library(plh_model_t m, const char* path);
/* 1 if the handle's last plh_integrate ran the attached closure library's kernels, 0 if it interpreted (or had no closure input) */
int plh_last_integrate_compiled(plh_model_t m);
/* the digest plh_integrate computes for a protocol (0 if it has no PLH_VAL_EXPR run): what a builder embeds in the library */
unsigned long long plh_closure_digest(int n_runs, const plh_run* runs);

/* ---- the saved points of an ensemble on ONE time grid shared by all cells: the reference's sol(t) / simulate(p, tf::Vector) (src/save_outputs.jl:74-133), which puts an
 * interpolating spline through each run's saved points (Dierckx Spline1D, s = 0) -- post-interpolation of what plh_integrate wrote, not dense output of the integrator.
 * Every cell takes its own adaptive steps, so t[cell] differs from cell to cell; this call resamples ONE per-point field per call:
 *   src[cell][max_pts][width] on the time axis t[cell][max_pts] (V: width 1, Y_all: width N, Y_sel: width n_sel_total), with n_pts / run_info / max_pts as plh_integrate wrote them.
 * Runs: the saved points of run r of a cell are the rows [start_r, start_r + run_info[cell][r].iterations), start = the running sum of the iterations; run r spans
 * (t_end of run r-1, t_end of run r), span 0 starts at the cell's first saved time.  A query goes to run 0 when it lies before the first span, else to the first run whose
 * span holds it (ends included), else to the last run.  A run with n >= 4 points gets the interpolating cubic spline with not-a-knot ends (FITPACK curfit with k = 3, s = 0:
 * what the reference's Spline1D and scipy's splrep build; equal to it to rounding), n = 3 the parabola, n = 2 the line, n = 1 the constant.
 * extrapolate = 0 (the reference's interp_bc = :interpolate, bc = "nearest"): a query is clamped to the first / last saved time of its run; 1: the end pieces continue.
 * What is written: dst[cell][n_q][width], every entry; status[cell] (may be NULL) = 0, or 1 for a cell that cannot be resampled: a run with flag < 0 (PLH_ERR_*,
 * PLH_ERR_OUTPUT_FULL among them) or without a saved point, or n_pts[cell] != the sum of the runs' iterations (a trajectory cut at max_pts).  Such a cell's dst row is NaN
 * and none of its points is read.  A NaN query time gives NaN in every cell.  A query at a saved time returns the saved value.
 * tq[n_q]: solution time, shared by all cells, any order; HOST memory for every ptr_kind (staged like plh_opts.tdiscon).  All other arrays follow ptr_kind: PLH_HOST blocks,
 * PLH_DEVICE is asynchronous on `stream`.  The slopes live in a per-stream workspace of the handle (max_pts x width doubles per cell) bounded by processing the cells in
 * chunks: PLH_RESAMPLE_WS_BYTES in the environment (default 256 MiB, read at every call) caps it; the result does not depend on the chunking.
 * PLH_E_ARG: n_cells, n_runs, max_pts, width or n_q < 1, extrapolate not 0 / 1, a NULL array other than status.  Nothing is clamped. */
int plh_resample(plh_model_t m, int n_cells, int n_runs, int max_pts, const double* t, const int* n_pts, const plh_run_info* run_info,
                 int width, const double* src, int n_q, const double* tq, int extrapolate,
                 double* dst /* [n_cells][n_q][width] */, int* status /* [n_cells] or NULL */, int ptr_kind, void* stream);

/* ---- the weighted least-squares misfit of every cell's voltage curve against measured data, with its gradient and Gauss-Newton matrix when the ensemble was integrated by
 * plh_integrate_sens: what a fit needs per cell and iteration (1 + n_sens + n_sens^2 numbers) instead of the curves and their Jacobian.
 * S_V and S_k are exactly plh_resample's functions of V[cell] and of row k of dV_dtheta[cell]: the same run-assignment rule, the same not-a-knot cubic with the same
 * n = 3 / 2 / 1 fall-backs, the same clamping (extrapolate = 0) or continuation (1).  With measurement times tq_q, data y_q and weights w_q:
 *   r_q    = w_q (S_V(tq_q) - y_q)
 *   J_qk   = w_q S_k(tq_q)
 *   cost   = 1/2 sum_q r_q^2
 *   grad_k = sum_q J_qk r_q
 *   JtJ_kl = sum_q J_qk J_ql
 *   resid[q] = r_q
 * J is the derivative of the resampled curve AT FIXED KNOTS: the dependence of the saved times on theta is ignored, as it is for every post-interpolated output.
 * Points left out: a point with w_q == 0 is not evaluated -- it contributes nothing, its resid is 0, and a NaN tq_q or y_q there is harmless.  A point with w_q != 0 and a
 * NaN tq_q or y_q makes cost NaN, and the sums it enters.
 * Cells that cannot be resampled (plh_resample's rule, status[cell] = 1): cost, grad, JtJ and resid rows are NaN, none of the cell's points is read, other cells do not
 * notice.  NaN in a cell's dV_dtheta (the documented NaN cases of the sensitivities) reaches grad and JtJ of that cell only; cost and resid stay finite.
 * n_sens == 0 is the misfit-only call (ensembles run without sensitivities): dV_dtheta, grad and JtJ are then NULL -- and only then.
 * tq[n_q]: HOST memory for every ptr_kind (staged like plh_resample's tq).  y and w follow ptr_kind; w may be NULL (= 1); per_cell = 0: y[n_q], w[n_q] shared by all cells,
 * 1: y[n_cells][n_q], w[n_cells][n_q].  PLH_HOST blocks, PLH_DEVICE is asynchronous on `stream`.  The slopes of the 1 + n_sens columns live in plh_resample's per-stream
 * workspace, bounded the same way (PLH_RESAMPLE_WS_BYTES); the result does not depend on the chunking and is bit-identical between the two pointer kinds.
 * PLH_E_ARG, nothing clamped: n_cells, n_runs, max_pts or n_q < 1; n_sens outside 0 .. PLH_LSQ_MAX_SENS; per_cell or extrapolate not 0 / 1; a NULL among t, n_pts, run_info,
 * V, tq, y, cost; dV_dtheta / grad / JtJ NULL-ness that does not match n_sens. */
#define PLH_LSQ_MAX_SENS 8
int plh_lsq(plh_model_t m, int n_cells, int n_runs, int max_pts, const double* t, const int* n_pts, const plh_run_info* run_info,
            const double* V /* [n_cells][max_pts] */, int n_sens, const double* dV_dtheta /* [n_cells][n_sens][max_pts] */,
            int n_q, const double* tq, const double* y, const double* w, int per_cell, int extrapolate,
            double* cost /* [n_cells] */, double* grad /* [n_cells][n_sens] */, double* JtJ /* [n_cells][n_sens][n_sens], full symmetric */,
            double* resid /* [n_cells][n_q] or NULL */, int* status /* [n_cells] or NULL */, int ptr_kind, void* stream);

/* ---- the same objective over several measured channels in one pass: V in a current-controlled leg, I in a constant-voltage leg, T_avg from a thermocouple.  Channel c is a
 * per-point curve and the rows of its per-point sensitivities (plh_integrate_sens_out: V / dV_dtheta, I / dI_dtheta, T_avg / dT_avg_dtheta), with data and weights of its own.
 * With S_c and S_ck the resampled functions of channel c's curve and of row k of its dcurve, r_cq = w_cq (S_c(tq_q) - y_cq) and J_cqk = w_cq S_ck(tq_q):
 *   cost   = 1/2 sum_c sum_q r_cq^2
 *   grad_k = sum_c sum_q J_cqk r_cq
 *   JtJ_kl = sum_c sum_q J_cqk J_cql
 *   ch[c].resid[q] = r_cq
 * Everything else is plh_lsq's: the splines, the run assignment, clamping / continuation, status, the w == 0 rule (per channel: a point with w_cq == 0 is not evaluated in
 * channel c, its resid there is 0 and a NaN datum there is harmless, while the other channels still count that time), NaN containment (NaN in one channel's dcurve reaches grad and
 * JtJ of that cell only), the chunking through PLH_RESAMPLE_WS_BYTES.  The channels share tq: a channel that was measured at other times gets weight 0 where it has no datum.
 * The units of the channels differ; the weights carry 1 / sigma of each.  Within a lane the sums run queries outer, channels inner, in the order of ch[]; the bits do not depend
 * on the chunking or the pointer kind, and with n_ch == 1 they are plh_lsq's (plh_lsq is this call with one channel).
 * ch[n_ch] itself is HOST memory for every ptr_kind; the pointers in it follow ptr_kind.  y, w: [n_q] (per_cell = 0) or [n_cells][n_q] (1), for all channels alike.
 * PLH_E_ARG, nothing clamped: plh_lsq's cases, n_ch outside 1 .. PLH_LSQ_MAX_CHANNELS, a NULL ch, a NULL curve or y in a channel, a dcurve whose NULL-ness does not
 * match n_sens. */
#define PLH_LSQ_MAX_CHANNELS 3
typedef struct {
  const double* curve;   /* [n_cells][max_pts] */
  const double* dcurve;  /* [n_cells][n_sens][max_pts]; NULL iff n_sens == 0 */
  const double* y;       /* [n_q] or [n_cells][n_q]; follows per_cell */
  const double* w;       /* [n_q] or [n_cells][n_q]; may be NULL (= 1) */
  double* resid;         /* [n_cells][n_q] or NULL */
} plh_lsq_channel;
int plh_lsq_multi(plh_model_t m, int n_cells, int n_runs, int max_pts, const double* t, const int* n_pts, const plh_run_info* run_info,
                  int n_ch, const plh_lsq_channel* ch, int n_sens, int n_q, const double* tq, int per_cell, int extrapolate,
                  double* cost /* [n_cells] */, double* grad /* [n_cells][n_sens] */, double* JtJ /* [n_cells][n_sens][n_sens], full symmetric */,
                  int* status /* [n_cells] or NULL */, int ptr_kind, void* stream);

/* ---- one Levenberg-Marquardt iteration per cell on the device: judges the trial that was just integrated, updates the damping, tests convergence, solves the damped,
 * scaled, box-bounded normal equations and writes the next trial into the cell's theta row.  A fit is: integrate with sensitivities, plh_lsq / plh_lsq_multi, plh_lm_step
 * (PLH_LM_FIRST); then integrate, lsq, plh_lm_step (PLH_LM_STEP) until *n_running == 0 or the budget is spent; then integrate, lsq, plh_lm_step (PLH_LM_LAST).  One
 * sensitivity integration per iteration: an accepted trial carries its own grad / JtJ.
 *
 * Arguments.  k = n_keys (1 .. PLH_LSQ_MAX_SENS).  cols[k] (theta columns, in the order of the sens keys) and transform[k] (PLH_LM_LINEAR: u = theta, PLH_LM_LOG: u = ln theta)
 * are HOST memory for every ptr_kind, and so are shared bounds; every other array follows ptr_kind (PLH_HOST blocks; PLH_DEVICE is asynchronous on `stream`).
 *   theta[n][n_theta]   in: the point that was just integrated; out: the next trial, or the cell's best point when the cell is done.  Only columns in cols are ever written.
 *   lo, hi              bounds in theta units: [k] in HOST memory (bounds_per_cell = 0) or [n][k] following ptr_kind (1); a NULL lo is -inf, a NULL hi is +inf
 *   cost[n], grad[n][k], JtJ[n][k][k], status[n]     the fit of the point in theta, as plh_lsq_multi wrote it (status may be NULL = 0 everywhere).  Only JtJ's upper triangle
 *                                                    (row <= column) is used; JtJ_cur receives the full copy.
 *   theta_cur[n][k], cost_cur[n], grad_cur[n][k], JtJ_cur[n][k][k], lambda[n], pred[n], state[n], n_accept[n], n_reject[n]
 *                       the per-cell state, owned by the caller and carried between the calls of one fit; PLH_LM_FIRST initialises it
 *   n_running           one int: the number of cells with state == PLH_LM_RUNNING after the call
 *   o                   NULL = PLH_LM_OPTS_DEFAULT
 *
 * Per cell ("finite": neither NaN nor +-inf; "the fit": cost, grad and the upper triangle of JtJ; theta_i: the entry of column cols[i]):
 *  Done cells.  Phase STEP / LAST with state != PLH_LM_RUNNING: nothing of the cell is written -- its theta row and every state array keep their bits.  Phase FIRST ignores
 *    the incoming state.
 *  Phase FIRST.  The start is bad if status != 0, or the fit is not finite, or for some key theta_i is not finite, or not (lo_i <= theta_i <= hi_i) (so a per-cell lo_i > hi_i
 *    or a NaN bound is a bad start), or theta_i <= 0 under PLH_LM_LOG.  A bad start: state = PLH_LM_FAILED_START, and nothing else of the cell is written.  Otherwise
 *    cur <- the incoming point (theta_cur, cost_cur, grad_cur, JtJ_cur), lambda = lambda0, pred = 0, n_accept = n_reject = 0, state = PLH_LM_RUNNING; go to Propose.
 *  Phase STEP / LAST, judging the trial.  ok = (status == 0 and the fit is finite); actual = cost_cur - cost; accept iff ok and actual >= eta * pred.
 *    Accept: cur <- the trial (theta_cur, cost_cur, grad_cur, JtJ_cur), lambda = max(lambda * lambda_down, lambda_min), n_accept++; if actual <= ftol * (the old cost_cur):
 *            state = PLH_LM_CONV_F.
 *    Reject: lambda = lambda * lambda_up, n_reject++, theta_i <- theta_cur_i; if lambda > lambda_max: state = PLH_LM_STALLED.
 *    Phase LAST: a cell still RUNNING after judging gets state = PLH_LM_MAXIT, theta_i <- theta_cur_i, and nothing is proposed.
 *  Propose (FIRST and STEP, cells still RUNNING), with g, H, theta from the cur arrays:
 *    Scaling:     s_i = theta_i for a LOG key, 1 for a LINEAR key; gs_i = s_i g_i; Hs_ij = (s_i s_j) H_ij.
 *                 A gs_i or Hs_ij that is not finite (the scaling overflowed): state = PLH_LM_STALLED, theta stays at cur.
 *    Active set:  key i is held if (theta_i <= lo_i and gs_i > 0) or (theta_i >= hi_i and gs_i < 0); the others are free.
 *    Gradient test (MINPACK's cosine): no free key, or cost_cur == 0, or |gs_i| <= gtol * sqrt(Hs_ii * 2 cost_cur) for every free key (a free key with Hs_ii == 0 has
 *                 gs_i == 0 and passes): state = PLH_LM_CONV_G, theta stays at cur.
 *    Damping:     D_i = max(Hs_ii, diag_floor * max_j Hs_jj), the maximum over all k keys.
 *    Solve, at most PLH_LM_MAX_TRIES tries: A = Hs_ff + lambda diag(D_f) over the free keys; Cholesky A = L L^T, row by row (a pivot that is <= 0 or not finite fails);
 *                 d_f = -A^-1 gs_f, d = 0 for held keys; trial_i = theta_i + d_i (LINEAR) or theta_i exp(d_i) (LOG: u + d transformed back), clamped to [lo_i, hi_i];
 *                 for a key the clamp moved, d_i = trial_i - theta_i (LINEAR) or ln(trial_i / theta_i) (LOG): the step actually taken in u;
 *                 pred = -(gs.d + 1/2 d.Hs d).
 *                 A Cholesky failure, a trial that is not finite, or not (pred > 0): lambda = lambda * lambda_up; if lambda > lambda_max: state = PLH_LM_STALLED, theta stays
 *                 at cur; else try again.  After PLH_LM_MAX_TRIES failed tries the cell is PLH_LM_STALLED as well.
 *    Step test:   m_i = |d_i| (LOG) or |d_i| / max(|theta_i|, DBL_MIN) (LINEAR); if m_i <= xtol for every key: state = PLH_LM_CONV_X, theta stays at cur (the step is not taken).
 *    Otherwise    theta_i <- trial_i, and pred is stored.
 * Nothing in the arithmetic depends on the launch shape or the pointer kind: the bits of every output are the same for PLH_HOST and PLH_DEVICE.
 * PLH_E_ARG, nothing written: n_cells < 1; n_keys outside 1 .. PLH_LSQ_MAX_SENS; n_theta < 1; a column outside [0, n_theta) or given twice; an unknown transform or phase;
 * bounds_per_cell not 0 / 1; a NULL among theta, cols, transform, cost, grad, JtJ, the state arrays and n_running; lambda_up <= 1, lambda_down outside (0, 1), lambda0 <= 0,
 * lambda_min < 0, lambda_max < lambda_min, eta < 0, a negative ftol / xtol / gtol / diag_floor (or a NaN in any option); shared bounds with lo_i > hi_i or a NaN. */
#define PLH_LM_LINEAR 0
#define PLH_LM_LOG 1
#define PLH_LM_FIRST 0
#define PLH_LM_STEP 1
#define PLH_LM_LAST 2
#define PLH_LM_RUNNING 0
#define PLH_LM_CONV_F 1        /* the accepted step lowered the cost by <= ftol * cost */
#define PLH_LM_CONV_X 2        /* the proposed step is <= xtol in every key */
#define PLH_LM_CONV_G 3        /* the projected gradient test passed */
#define PLH_LM_MAXIT 4         /* still running at PLH_LM_LAST */
#define PLH_LM_STALLED 5       /* lambda passed lambda_max, or PLH_LM_MAX_TRIES failed solves */
#define PLH_LM_FAILED_START 6  /* the starting point cannot be used */
#define PLH_LM_MAX_TRIES 16
typedef struct {
  double lambda0, lambda_up, lambda_down, lambda_min, lambda_max;
  double eta, ftol, xtol, gtol, diag_floor;
} plh_lm_opts;
#define PLH_LM_OPTS_DEFAULT { 1e-3, 3.0, 1.0 / 3.0, 1e-12, 1e12, 1e-4, 1e-10, 1e-8, 1e-8, 1e-12 }
int plh_lm_step(plh_model_t m, int n_cells, int n_theta, double* theta /* [n_cells][n_theta] */,
                int n_keys, const int* cols, const int* transform, const double* lo, const double* hi, int bounds_per_cell,
                const double* cost, const double* grad, const double* JtJ, const int* status,
                double* theta_cur, double* cost_cur, double* grad_cur, double* JtJ_cur, double* lambda, double* pred,
                int* state, int* n_accept, int* n_reject,
                const plh_lm_opts* o, int phase, int* n_running, int ptr_kind, void* stream);
/* sizeof / offsetof of plh_lm_opts, in plh_abi_layout's format (sizeof, number of fields, the offsets) */
int plh_lm_abi_layout(int* out, int cap);

/* ---- parameters shared by groups of cells: consecutive cells form a group (one experiment per member), all members share the fitted keys, and one group is one
 * least-squares problem.  plh_lsq_group sums what plh_lsq_multi left per cell into one fit per group; plh_lm_step then runs with n_cells = n_groups on a matrix of one theta
 * row per group; plh_group_scatter copies the keys of every group's row into the theta rows of its members.  A grouped fit is: scatter the start; then per iteration
 * integrate with sensitivities, plh_lsq / plh_lsq_multi, plh_lsq_group, plh_lm_step (on the groups), plh_group_scatter.
 *
 * The grouping.  group_off[n_groups + 1], HOST memory for every ptr_kind (like cols): group_off[0] == 0, group_off[n_groups] == n_cells, strictly ascending (every group
 * has at least one member).  Group g owns the cells group_off[g] .. group_off[g + 1] - 1.  The device copy of the offsets is remembered per stream: a repeated call with
 * the same grouping uploads nothing and does not synchronise.
 *
 * plh_lsq_group.  For every group g with members c0 < c1 < ... :
 *   g_cost[g]         = (..((cost[c0] + cost[c1]) + cost[c2]) + ..)
 *   g_grad[g][i]      = the same sum of grad[c][i], for every i < n_sens
 *   g_JtJ[g][i][j]    = the same sum of JtJ[c][i][j], for every i, j < n_sens (the full matrix, both triangles, as plh_lsq_multi writes it)
 *   g_status[g]       = 1 if status[c] != 0 for any member, else 0 (g_status may be NULL; a NULL status is 0 everywhere)
 *  The sum is sequential, in ascending cell order, and starts from the first member's value: a group of one member has its member's bits.  Only additions occur (nothing can
 *  be contracted), so the bits of every output are a function of the inputs alone -- not of the launch shape, the pointer kind or the wave width -- and a plain loop on the
 *  host reproduces them.  A NaN or an infinity of a member flows through the sum into its group (and into no other); plh_lm_step then rejects the group's trial.  The
 *  inputs are not written.  n_sens == 0 is the cost-only call: grad, JtJ, g_grad and g_JtJ are then NULL -- and only then.
 *
 * plh_group_scatter.  theta[c][cols[i]] = g_theta[g][cols[i]] for every group g, every member c of g and every i < n_keys.  No other entry of theta is written; g_theta is
 * not written.  cols[n_keys] is HOST memory.  A PLH_HOST call stages theta whole, both ways: an entry that is not written keeps its bits.
 *
 * Both: PLH_HOST blocks, PLH_DEVICE is asynchronous on `stream`; the bits are the same for both.
 * PLH_E_ARG, nothing written: n_cells < 1; n_groups < 1 or > n_cells; a NULL group_off, or offsets that do not start at 0, do not end at n_cells or are not strictly
 * ascending; (plh_lsq_group) n_sens outside 0 .. PLH_LSQ_MAX_SENS, a NULL cost or g_cost, grad / JtJ / g_grad / g_JtJ whose NULL-ness does not match n_sens;
 * (plh_group_scatter) n_theta < 1, n_keys outside 1 .. PLH_LSQ_MAX_SENS, a NULL cols, g_theta or theta, a column outside [0, n_theta) or given twice. */
int plh_lsq_group(plh_model_t m, int n_cells, int n_groups, const int* group_off /* [n_groups + 1], HOST */,
                  int n_sens, const double* cost /* [n_cells] */, const double* grad /* [n_cells][n_sens] */, const double* JtJ /* [n_cells][n_sens][n_sens] */,
                  const int* status /* [n_cells] or NULL */,
                  double* g_cost /* [n_groups] */, double* g_grad /* [n_groups][n_sens] */, double* g_JtJ /* [n_groups][n_sens][n_sens] */,
                  int* g_status /* [n_groups] or NULL */, int ptr_kind, void* stream);
int plh_group_scatter(plh_model_t m, int n_cells, int n_groups, const int* group_off /* [n_groups + 1], HOST */,
                      int n_theta, int n_keys, const int* cols /* [n_keys], HOST */,
                      const double* g_theta /* [n_groups][n_theta] */, double* theta /* [n_cells][n_theta] */, int ptr_kind, void* stream);

/* ---- parameter covariances and identifiability of n fitted problems (a problem: a cell, or a group row of a grouped fit), from the arrays a fit left behind: the *_cur
 * state arrays of plh_lm_step, or what plh_lsq_multi / plh_lsq_group wrote together with the keys' values.  One call for all problems; nothing of the inputs is written.
 *
 * Arguments.  k = n_keys (1 .. PLH_LSQ_MAX_SENS).  transform[k] and shared bounds are HOST memory for every ptr_kind, every other array follows ptr_kind.
 *   theta_k[n][k]       the keys' values, in the order of the keys (plh_lm_step's theta_cur)
 *   lo, hi, bounds_per_cell     as plh_lm_step: [k] in HOST memory (0) or [n][k] following ptr_kind (1); a NULL lo is -inf, a NULL hi is +inf (an infinite bound is no bound)
 *   cost[n], grad[n][k], JtJ[n][k][k]     the fit at theta_k; only JtJ's upper triangle (row <= column) is used
 *   n_data[n]           the number of data of every problem (the (channel, time) pairs with a weight that is not 0), or NULL
 *   sigma2[n], cov[n][k][k], stderr_[n][k], corr[n][k][k], eval[n][k], evec[n][k][k], collinearity[n], free_mask[n], status[n]     the outputs, all required
 *
 * Per problem ("finite": neither NaN nor +-inf; g, H: grad and the upper triangle of JtJ mirrored; theta_i: theta_k[i]):
 *  Input check.  The input is bad if cost, a g_i, an H_ij or a theta_i is not finite, or not (lo_i <= theta_i <= hi_i) (so a NaN bound, or lo_i > hi_i, is bad input), or
 *    theta_i <= 0 under PLH_LM_LOG, or a scaled gs_i / Hs_ij (below) is not finite, or an Hs_ii < 0.  Bad input: status = PLH_COV_BAD_INPUT, free_mask = 0, and every double
 *    output of the problem is NaN.
 *  Scaling and active set, plh_lm_step's:  s_i = theta_i for a LOG key, 1 for a LINEAR key; gs_i = s_i g_i; Hs_ij = (s_i s_j) H_ij.  Key i is held if
 *    (theta_i <= lo_i and gs_i > 0) or (theta_i >= hi_i and gs_i < 0); the others are free.  free_mask: bit i is set for a free key; n_free = popcount(free_mask).
 *  Unseen keys.  A free key with Hs_ii == 0 is unseen (the data do not move it): it is taken out of the matrices like a held key but stays in free_mask.  The mask of the
 *    unseen keys is reported in bits 8 .. 15 of status, and PLH_COV_UNSEEN is set.  The analysed keys are the free keys that are seen; n_an is their number.
 *  Residual variance.  n_data == NULL: sigma2 = 1 (the weights are 1 / sigma of the data: scipy's absolute_sigma).  Otherwise sigma2 = (2 cost) / (n_data - n_free); with
 *    n_data - n_free <= 0: sigma2 = NaN and PLH_COV_NO_DOF is set (cov and stderr of the analysed keys are then NaN; corr and the eigen outputs stay valid).
 *  Normalised information matrix.  r_i = sqrt(Hs_ii); C_ij = Hs_ij / (r_i r_j) over the analysed keys, C_ii = 1 exactly; every other key has an identity row and column.
 *    (Marquardt's scaling, the scale plh_lm_step damps in; invariant under a change of units of a LINEAR key.)
 *  Covariance.  Cholesky C = L L^T, row by row; a pivot that is <= 0 or not finite fails: PLH_COV_SINGULAR is set and cov, stderr and corr of the analysed keys are NaN
 *    (the eigen outputs are still given).  Otherwise X = L^-1 (column by column), P = X^T X = C^-1, and for analysed i, j:
 *      corr_ij = P_ij / sqrt(P_ii P_jj), corr_ii = 1 exactly;   cov_ij = (s_i s_j) ((P_ij sigma2) / (r_i r_j))   (the covariance in u, carried to theta by the delta method);
 *      stderr_i = sqrt(cov_ii).
 *    A held key: its rows and columns of cov and corr are 0 (the diagonal too) and stderr_i = 0.  An unseen key: its rows and columns are NaN, except where they meet a held
 *    key (0), and stderr_i = +inf.  Both triangles are written.
 *  Identifiability.  The eigen-decomposition of C by cyclic Jacobi, pivots (p, q), p < q, row-wise, V = I at the start.  An entry with
 *    |a_pq| <= DBL_EPSILON sqrt(|a_pp a_qq|) is set to 0 and not rotated (so an exact 0 is never rotated, and the keys that are not analysed keep unit vectors).  Otherwise
 *    Rutishauser's rotation: theta = (a_qq - a_pp) / (2 a_pq); t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) (sign(0) = +1); c = 1 / sqrt(t^2 + 1); s = t c;
 *    tau = s / (1 + c); a_pp -= t a_pq; a_qq += t a_pq; a_pq = 0; every other pair (g, h) = (a_rp, a_rq), and every (v_rp, v_rq): g' = g - s (h + tau g), h' = h + s (g - tau h).
 *    The iteration stops after a sweep without a rotation; after PLH_COV_MAX_SWEEPS sweeps that all rotated, PLH_COV_SWEEPS is set.
 *    eval[0 .. n_an - 1]: the eigenvalues (the diagonal) of the analysed part, ascending; ties keep the order of the Jacobi columns.  evec[j][.]: eigenvector j over the k keys
 *    in key order; the component of a key that is not analysed is exactly 0; the component of largest magnitude is positive (the lowest index wins a tie).  Rows j >= n_an of
 *    eval and evec are NaN.  collinearity = 1 / sqrt(eval[0]) (Brun et al.'s collinearity index), +inf if eval[0] <= 0; with n_an == 0 it is NaN and PLH_COV_NO_FREE is set.
 * Nothing in the arithmetic depends on the launch shape or the pointer kind: the bits of every output are the same for PLH_HOST (blocks) and PLH_DEVICE (asynchronous on
 * `stream`).
 * PLH_E_ARG, nothing written: n < 1; n_keys outside 1 .. PLH_LSQ_MAX_SENS; an unknown transform; bounds_per_cell not 0 / 1; a NULL among transform, theta_k, cost, grad, JtJ
 * and the outputs; shared bounds with lo_i > hi_i or a NaN. */
#define PLH_COV_BAD_INPUT 1    /* status bits */
#define PLH_COV_NO_FREE 2      /* no analysed key */
#define PLH_COV_UNSEEN 4       /* a free key with Hs_ii == 0; which: bits 8 .. 15 */
#define PLH_COV_NO_DOF 8       /* n_data - n_free <= 0 */
#define PLH_COV_SINGULAR 16    /* the Cholesky factorisation of C failed */
#define PLH_COV_SWEEPS 32      /* Jacobi still rotated in sweep PLH_COV_MAX_SWEEPS */
#define PLH_COV_MAX_SWEEPS 16
int plh_fit_cov(plh_model_t m, int n, int n_keys, const int* transform /* [k], HOST */,
                const double* theta_k /* [n][k] */, const double* lo, const double* hi, int bounds_per_cell,
                const double* cost /* [n] */, const double* grad /* [n][k] */, const double* JtJ /* [n][k][k] */, const int* n_data /* [n] or NULL */,
                double* sigma2 /* [n] */, double* cov /* [n][k][k] */, double* stderr_ /* [n][k] */, double* corr /* [n][k][k] */,
                double* eval /* [n][k] */, double* evec /* [n][k][k] */, double* collinearity /* [n] */,
                int* free_mask /* [n] */, int* status /* [n] */, int ptr_kind, void* stream);

/* ---- prediction bands: every cell's measured curves and their sensitivities at query times of the caller's choosing, and the variance of the predicted curve under the
 * covariance of the fitted keys.  It answers "how well is the curve known?" after plh_fit_cov answered "how well are the parameters known?", from arrays that are already in
 * device memory after a fit: the per-point curves, their per-point sensitivities (plh_integrate_sens_out) and cov[n][k][k].
 * Channel c is a per-point curve and the rows of its per-point sensitivities, as in plh_lsq_multi.  S_c and S_ck are exactly plh_resample's functions of channel c's curve
 * and of row k of its dcurve: the same run-assignment rule, the same not-a-knot cubic with the same n = 3 / 2 / 1 fall-backs, the same clamping (extrapolate = 0) or
 * continuation (1).  With k = n_sens (1 .. PLH_LSQ_MAX_SENS; a call without sensitivities is plh_resample) and query times tq_q:
 *   ch[c].pred[cell][q]     = S_c(tq_q)
 *   ch[c].dpred[cell][i][q] = S_ci(tq_q)       the derivative of the resampled curve AT FIXED KNOTS, as everywhere in this library
 *   ch[c].var[cell][q]      = sum_i s_i v_i (i ascending), with s_i = S_ci(tq_q) and v_i = sum_j M_ij s_j (j ascending)
 * M is the upper triangle (row <= column) of the cell's covariance, mirrored.  This is the delta-method variance of the predicted curve, in the units of the curve squared.
 * cov is in theta units, as plh_fit_cov writes it (its delta method for PLH_LM_LOG keys is already inside).  var is stored as computed: it is not clamped and no square
 * root is taken, so a tiny negative value from cancellation stays visible.  It is the variance of the curve, not of a new observation (the caller adds sigma^2 for that).
 * Every output pointer of a channel may be NULL (not written), but not all three; a query at a saved time returns the saved bits in pred and dpred.
 * NaN flows through the arithmetic.  A held key has 0 rows and columns in cov and contributes nothing.  A problem with an unseen key (NaN rows) or a failed covariance
 * gets var = NaN and keeps pred and dpred.  A NaN in one channel's dcurve reaches that channel's dpred and var of that cell only.  A NaN tq_q gives NaN at q in every output.
 * Which covariance a cell takes.  group_off == NULL: cov[cell] (cov is [n_cells][k][k]; n_groups is ignored).  Otherwise cov[g] of the group g that owns the cell (cov is
 * [n_groups][k][k]); group_off[n_groups + 1] is HOST memory and follows plh_lsq_group's rules, and its device copy is the one plh_lsq_group remembers per stream: after a
 * grouped fit nothing is uploaded and nothing synchronises.
 * Cells that cannot be resampled (plh_resample's rule, status[cell] = 1): every output row of the cell is NaN, none of its points is read, other cells do not notice.
 * ch[n_ch] itself and tq[n_q] are HOST memory for every ptr_kind; the pointers in ch and every other array follow ptr_kind.  PLH_HOST blocks, PLH_DEVICE is asynchronous
 * on `stream`.  The slopes of the n_ch (1 + k) columns live in plh_resample's per-stream workspace, bounded the same way (PLH_RESAMPLE_WS_BYTES).  Every output is computed
 * by one lane in one order: the bits do not depend on the chunking or the pointer kind, and a channel's outputs do not depend on what else is in the call.
 * PLH_E_ARG, nothing written, nothing clamped: n_cells, n_runs, max_pts or n_q < 1; n_sens outside 1 .. PLH_LSQ_MAX_SENS; n_ch outside 1 .. PLH_LSQ_MAX_CHANNELS;
 * extrapolate not 0 / 1; a NULL among t, n_pts, run_info, ch, tq; a NULL curve or dcurve in a channel; a channel whose pred, dpred and var are all NULL; a var without cov;
 * with a group_off: plh_lsq_group's cases (n_groups < 1 or > n_cells, offsets that do not start at 0, do not end at n_cells or are not strictly ascending). */
typedef struct {
  const double* curve;   /* [n_cells][max_pts]            (V, I or T_avg as plh_integrate_sens_out wrote it) */
  const double* dcurve;  /* [n_cells][n_sens][max_pts] */
  double* pred;          /* [n_cells][n_q]          or NULL */
  double* dpred;         /* [n_cells][n_sens][n_q]  or NULL */
  double* var;           /* [n_cells][n_q]          or NULL; non-NULL needs cov */
} plh_predict_channel;
int plh_predict(plh_model_t m, int n_cells, int n_runs, int max_pts, const double* t, const int* n_pts, const plh_run_info* run_info,
                int n_ch, const plh_predict_channel* ch /* HOST */, int n_sens, int n_q, const double* tq /* HOST */, int extrapolate,
                const double* cov /* [n_prob][n_sens][n_sens] or NULL */, int n_groups, const int* group_off /* [n_groups + 1], HOST, or NULL */,
                int* status /* [n_cells] or NULL */, int ptr_kind, void* stream);

/* timing of the last plh_integrate kernel on its stream, measured with HIP events (ms); <0 if unavailable */
double plh_last_kernel_ms(plh_model_t m);

/* pinned host memory for PLH_HOST_ASYNC calls, and the completion point of everything the handle enqueued on `stream` */
int plh_host_alloc(void** p, unsigned long long bytes);
void plh_host_free(void* p);
int plh_synchronize(plh_model_t m, void* stream);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI for the ensemble scatter / gather only ----
 * A communicator joins n_ranks processes, each bound to one GPU.  Rank 0 obtains a 128-byte id with plh_comm_unique_id and hands it to the other
 * ranks by whatever means the host has (MPI, Distributed.jl, a file); every rank then calls plh_comm_create(n_ranks, rank, id, device).
 * plh_ensemble_run (collective: every rank calls it with the same protocol / options; theta, SOC0 and the output arrays are significant on rank 0
 * only and are HOST memory):
 *   1. ncclBroadcast of the ensemble shape, 2. scatter of the parameter rows from rank 0 (grouped ncclSend / ncclRecv; partition = contiguous blocks
 *   cells[r n/G, (r+1) n/G) or cyclic cell mod G, which evens out step-count variance in randomised sweeps), 3. plh_integrate of the local shard on the
 *   rank's GPU (no collective in the data path: cells are independent for the whole trajectory), 4. gather of the per-cell summaries (run_info,
 *   counters, optionally the final states) to rank 0 in the caller's cell order.  rank_ms[n_ranks] (rank 0, may be NULL) receives every rank's
 *   integrate-kernel time: the load-imbalance figure of a randomised sweep.
 * Per-cell protocol arrays (plh_run.value_cell / tf_cell) belong to the protocol: n_cells_total entries indexed by the GLOBAL cell, the same on every rank; each rank
 * integrates with its own shard of them.  An error on any rank (arguments, staging, its plh_integrate) is agreed on between the phases: every rank returns non-zero. */
typedef struct plh_comm_s* plh_comm_t;
#define PLH_PART_BLOCK 0
#define PLH_PART_CYCLIC 1
int plh_comm_unique_id(char id[128]);
int plh_comm_create(int n_ranks, int rank, const char id[128], int device, plh_comm_t* out);
void plh_comm_destroy(plh_comm_t c);
int plh_comm_rank(plh_comm_t c);
int plh_comm_size(plh_comm_t c);
int plh_ensemble_run(plh_comm_t c, plh_model_t m, int n_cells_total, const double* theta, const double* SOC0, int n_runs, const plh_run* runs,
                     const plh_opts* opts, int partition, plh_run_info* run_info, plh_counters* counters, double* Y_final, double* rank_ms);

#ifdef __cplusplus
}
#endif
#endif

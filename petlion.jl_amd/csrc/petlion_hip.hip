// petlion_hip.hip -- host side of the C ABI of include/petlion_hip.h  (libpetlion_hip.so, gfx950).
//
// The kernels live in one translation unit per model variant (variant_tu.hip, -DPL_VARIANT=<id>, table of entry points: VariantOps in plh_host.h);
// this file owns the handles, the staging of host arrays, the per-stream workspaces, the Jacobian patterns and the RCCL scatter / gather.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <cerrno>
#include <sys/mman.h>
#include <atomic>
#include <chrono>
#include <functional>
#include <vector>

#include <dlfcn.h>
#include <mutex>

#include "plh_host.h"

#ifdef PL_WAVE_EMU
// the test-only wave-emulator build is a single translation unit: every variant's kernels are compiled right here, no RCCL
// (-DPL_VARIANT=<id>: a developer's quick build with that one variant; the others are then refused by plh_model_create)
#ifndef PL_VARIANT
#define PL_VARIANT -1
#endif
#include "variant_tu.hip"
#else
#include <rccl/rccl.h>
#endif

#include "plh_resample.h"
#include "plh_lsq.h"
#include "plh_predict.h"
#include "plh_lm.h"
#include "plh_cov.h"
#include "plh_group.h"

using namespace pl;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return fail(PLH_E_HIP, std::string(#x) + ": " + hipGetErrorString(e__)); } while (0)

// names of the Key enum entries (reference Symbols, UTF-8)
static const char* const KEY_ENUM_NAMES[K_COUNT] = {
    "D_n", "D_p", "D_s", "D_sn", "D_sp", "Ea_D_sn", "Ea_D_sp", "Ea_k_n", "Ea_k_p", "M_n", "R_SEI", "Rp_n", "Rp_p", "T₀", "Uref_s",
    "brugg_n", "brugg_p", "brugg_s", "c_e₀", "c_max_n", "c_max_p", "i_0_jside", "k_n", "k_n_aging", "k_p", "l_n", "l_p", "l_s",
    "t₊", "w", "θ_max_n", "θ_max_p", "θ_min_n", "θ_min_p", "ρ_n", "σ_n", "σ_p", "ϵ_fn", "ϵ_fp", "ϵ_n", "ϵ_p", "ϵ_s",
    "Cp_a", "Cp_n", "Cp_p", "Cp_s", "Cp_z", "T_amb", "h_cell", "l_a", "l_z", "λ_a", "λ_n", "λ_p", "λ_s", "λ_z",
    "ρ_a", "ρ_p", "ρ_s", "ρ_z", "σ_a", "σ_z", "λ_MHC_n", "λ_MHC_p", "D_e"};
// per variant: the sorted theta_keys the reference's generated functions would receive (generate_functions.jl:327-363, 387) and
// the chemistry defaults (reference src/params.jl:5-117, 176-226 LCO/LiC6; 295-367, 436-452 NMC/LiC6_NMC)
static const char* const KEYS_LCO_ISO[] = {
    "D_n", "D_p", "D_s", "D_sn", "D_sp", "Ea_D_sn", "Ea_D_sp", "Ea_k_n", "Ea_k_p", "Rp_n", "Rp_p", "T₀", "brugg_n", "brugg_p", "brugg_s",
    "c_e₀", "c_max_n", "c_max_p", "k_n", "k_p", "l_n", "l_p", "l_s", "t₊", "θ_max_n", "θ_max_p", "θ_min_n", "θ_min_p", "σ_n", "σ_p",
    "ϵ_fn", "ϵ_fp", "ϵ_n", "ϵ_p", "ϵ_s"};
static const double DEFAULTS_LCO_ISO[] = {
    7.5e-10, 7.5e-10, 7.5e-10, 3.9e-14, 1e-14, 5000.0, 5000.0, 5000.0, 5000.0, 2e-6, 2e-6, 25 + 273.15, 4.0, 4.0, 4.0,
    1000.0, 30555.0, 51554.0, 5.0310e-11, 2.334e-11, 88e-6, 80e-6, 25e-6, 0.364, 0.85510, 0.49550, 0.01429, 0.99174, 100.0, 100.0,
    0.0326, 0.025, 0.485, 0.385, 0.724};
static const char* const KEYS_NMC_ISO[] = {
    "D_sn", "D_sp", "Ea_D_sn", "Ea_D_sp", "Ea_k_n", "Ea_k_p", "Rp_n", "Rp_p", "T₀", "brugg_n", "brugg_p", "brugg_s", "c_e₀", "c_max_n", "c_max_p",
    "k_n", "k_p", "l_n", "l_p", "l_s", "t₊", "θ_max_n", "θ_max_p", "θ_min_n", "θ_min_p", "σ_n", "σ_p", "ϵ_fn", "ϵ_fp", "ϵ_n", "ϵ_p", "ϵ_s"};
static const double DEFAULTS_NMC_ISO[] = {
    1.5e-14, 2e-14, 4e4, 2.5e4, 3e4, 3e4, 10e-6, 7.5e-6, 25 + 273.15, 1.5, 1.5, 1.5, 1200.0, 31080.0, 51830.0,
    6.3466e-10, 6.3066e-10, 48e-6, 41.6e-6, 25e-6, 0.38, 0.790813, 0.359749, 0.001, 0.955473, 100.0, 100.0, 0.038, 0.12, 0.3, 0.3, 0.4};
// aging = :SEI adds M_n, R_SEI, Uref_s, i_0_jside, k_n_aging, w, rho_n (reference src/params.jl:90,98-110; NMC borrows them)
static const char* const KEYS_LCO_SEI[] = {
    "D_n", "D_p", "D_s", "D_sn", "D_sp", "Ea_D_sn", "Ea_D_sp", "Ea_k_n", "Ea_k_p", "M_n", "R_SEI", "Rp_n", "Rp_p", "T₀", "Uref_s",
    "brugg_n", "brugg_p", "brugg_s", "c_e₀", "c_max_n", "c_max_p", "i_0_jside", "k_n", "k_n_aging", "k_p", "l_n", "l_p", "l_s",
    "t₊", "w", "θ_max_n", "θ_max_p", "θ_min_n", "θ_min_p", "ρ_n", "σ_n", "σ_p", "ϵ_fn", "ϵ_fp", "ϵ_n", "ϵ_p", "ϵ_s"};
static const double DEFAULTS_LCO_SEI[] = {
    7.5e-10, 7.5e-10, 7.5e-10, 3.9e-14, 1e-14, 5000.0, 5000.0, 5000.0, 5000.0, 7.3e-4, 0.01, 2e-6, 2e-6, 25 + 273.15, 0.4,
    4.0, 4.0, 4.0, 1000.0, 30555.0, 51554.0, 1.5e-6, 5.0310e-11, 1.0, 2.334e-11, 88e-6, 80e-6, 25e-6,
    0.364, 2.0, 0.85510, 0.49550, 0.01429, 0.99174, 2500.0, 100.0, 100.0, 0.0326, 0.025, 0.485, 0.385, 0.724};
static const char* const KEYS_NMC_SEI[] = {
    "D_sn", "D_sp", "Ea_D_sn", "Ea_D_sp", "Ea_k_n", "Ea_k_p", "M_n", "R_SEI", "Rp_n", "Rp_p", "T₀", "Uref_s", "brugg_n", "brugg_p", "brugg_s",
    "c_e₀", "c_max_n", "c_max_p", "i_0_jside", "k_n", "k_n_aging", "k_p", "l_n", "l_p", "l_s", "t₊", "w", "θ_max_n", "θ_max_p", "θ_min_n",
    "θ_min_p", "ρ_n", "σ_n", "σ_p", "ϵ_fn", "ϵ_fp", "ϵ_n", "ϵ_p", "ϵ_s"};
static const double DEFAULTS_NMC_SEI[] = {
    1.5e-14, 2e-14, 4e4, 2.5e4, 3e4, 3e4, 7.3e-4, 0.01, 10e-6, 7.5e-6, 25 + 273.15, 0.4, 1.5, 1.5, 1.5,
    1200.0, 31080.0, 51830.0, 1.5e-6, 6.3466e-10, 1.0, 6.3066e-10, 48e-6, 41.6e-6, 25e-6, 0.38, 2.0, 0.790813, 0.359749, 0.001,
    0.955473, 2500.0, 100.0, 100.0, 0.038, 0.12, 0.3, 0.3, 0.4};
// temperature = true adds the heat-equation parameters (reference src/params.jl:40-45, 85-96, 200-226)
static const char* const KEYS_LCO_THERMAL[] = {
    "Cp_a", "Cp_n", "Cp_p", "Cp_s", "Cp_z", "D_n", "D_p", "D_s", "D_sn", "D_sp", "Ea_D_sn", "Ea_D_sp", "Ea_k_n", "Ea_k_p", "Rp_n", "Rp_p",
    "T_amb", "T₀", "brugg_n", "brugg_p", "brugg_s", "c_e₀", "c_max_n", "c_max_p", "h_cell", "k_n", "k_p", "l_a", "l_n", "l_p", "l_s", "l_z",
    "t₊", "θ_max_n", "θ_max_p", "θ_min_n", "θ_min_p", "λ_a", "λ_n", "λ_p", "λ_s", "λ_z", "ρ_a", "ρ_n", "ρ_p", "ρ_s", "ρ_z",
    "σ_a", "σ_n", "σ_p", "σ_z", "ϵ_fn", "ϵ_fp", "ϵ_n", "ϵ_p", "ϵ_s"};
static const double DEFAULTS_LCO_THERMAL[] = {
    897.0, 700.0, 700.0, 700.0, 385.0, 7.5e-10, 7.5e-10, 7.5e-10, 3.9e-14, 1e-14, 5000.0, 5000.0, 5000.0, 5000.0, 2e-6, 2e-6,
    25 + 273.15, 25 + 273.15, 4.0, 4.0, 4.0, 1000.0, 30555.0, 51554.0, 1.0, 5.0310e-11, 2.334e-11, 10e-6, 88e-6, 80e-6, 25e-6, 10e-6,
    0.364, 0.85510, 0.49550, 0.01429, 0.99174, 237.0, 1.7, 2.1, 0.16, 401.0, 2700.0, 2500.0, 2500.0, 1100.0, 8940.0,
    3.55e7, 100.0, 100.0, 5.96e7, 0.0326, 0.025, 0.485, 0.385, 0.724};
// rxn = MHC adds the reorganisation energies λ_MHC_p, λ_MHC_n (reference src/params.jl:16,67)
static const char* const KEYS_LCO_MHC[] = {
    "D_n", "D_p", "D_s", "D_sn", "D_sp", "Ea_D_sn", "Ea_D_sp", "Ea_k_n", "Ea_k_p", "Rp_n", "Rp_p", "T₀", "brugg_n", "brugg_p", "brugg_s",
    "c_e₀", "c_max_n", "c_max_p", "k_n", "k_p", "l_n", "l_p", "l_s", "t₊", "θ_max_n", "θ_max_p", "θ_min_n", "θ_min_p", "λ_MHC_n", "λ_MHC_p", "σ_n", "σ_p",
    "ϵ_fn", "ϵ_fp", "ϵ_n", "ϵ_p", "ϵ_s"};
static const double DEFAULTS_LCO_MHC[] = {
    7.5e-10, 7.5e-10, 7.5e-10, 3.9e-14, 1e-14, 5000.0, 5000.0, 5000.0, 5000.0, 2e-6, 2e-6, 25 + 273.15, 4.0, 4.0, 4.0,
    1000.0, 30555.0, 51554.0, 5.0310e-11, 2.334e-11, 88e-6, 80e-6, 25e-6, 0.364, 0.85510, 0.49550, 0.01429, 0.99174, 6.26e-20, 6.26e-20, 100.0, 100.0,
    0.0326, 0.025, 0.485, 0.385, 0.724};
// NMC_LGM50 + LiC6_LGM50 + system_LGM50_NMC_LiC6 (Chen et al. 2020): reference src/params.jl:514-560, 576-625, 776-801
static const char* const KEYS_LGM50_ISO[] = {
    "D_e", "D_sn", "D_sp", "Ea_D_sn", "Ea_D_sp", "Ea_k_n", "Ea_k_p", "Rp_n", "Rp_p", "T₀", "brugg_n", "brugg_p", "brugg_s", "c_e₀", "c_max_n", "c_max_p",
    "k_n", "k_p", "l_n", "l_p", "l_s", "t₊", "θ_max_n", "θ_max_p", "θ_min_n", "θ_min_p", "σ_n", "σ_p", "ϵ_fn", "ϵ_fp", "ϵ_n", "ϵ_p", "ϵ_s"};
static const double DEFAULTS_LGM50_ISO[] = {
    8.794e-11, 3.3e-14, 4e-15, 3.03e4, 0.0, 35000.0, 17800.0, 5.86e-6, 5.22e-06, 25 + 273.15, 1.5, 1.5, 1.5, 1000.0, 33133.0, 63104.0,
    6.716046737258585e-12, 3.5445802224420315e-11, 85.2e-6, 75.6e-6, 12e-6, 0.2594, 29866.0 / 33133, 17038.0 / 63104.0, 0.0481727, 0.8395, 215.0, 0.18, 0.0, 0.0, 0.25, 0.335, 0.47};
// ... with temperature = true, the reference default of this chemistry (params.jl:695): + the heat-equation parameters (params.jl:531-533, 593-595, 779-800)
static const char* const KEYS_LGM50_THERMAL[] = {
    "Cp_a", "Cp_n", "Cp_p", "Cp_s", "Cp_z", "D_e", "D_sn", "D_sp", "Ea_D_sn", "Ea_D_sp", "Ea_k_n", "Ea_k_p", "Rp_n", "Rp_p", "T_amb", "T₀", "brugg_n", "brugg_p", "brugg_s", "c_e₀", "c_max_n", "c_max_p", "h_cell", "k_n", "k_p", "l_a", "l_n", "l_p", "l_s", "l_z", "t₊", "θ_max_n", "θ_max_p", "θ_min_n", "θ_min_p", "λ_a", "λ_n", "λ_p", "λ_s", "λ_z", "ρ_a", "ρ_n", "ρ_p", "ρ_s", "ρ_z", "σ_a", "σ_n", "σ_p", "σ_z", "ϵ_fn", "ϵ_fp", "ϵ_n", "ϵ_p", "ϵ_s"};
static const double DEFAULTS_LGM50_THERMAL[] = {
    897.0, 700.0, 700.0, 700.0, 385.0, 8.794e-11, 3.3e-14, 4e-15, 30300.0, 0.0, 35000.0, 17800.0, 5.86e-06, 5.22e-06, 298.15, 298.15, 1.5, 1.5, 1.5, 1000.0, 33133.0, 63104.0, 1.0, 6.716046737258585e-12, 3.5445802224420315e-11, 1.6e-05, 8.52e-05, 7.56e-05, 1.2e-05, 1.2e-05, 0.2594, 0.9013973983641687, 0.2699987322515213, 0.0481727, 0.8395, 237.0, 1.7, 2.1, 0.16, 401.0, 2700.0, 1657.0, 3262.0, 397.0, 8960.0, 36914000.0, 215.0, 0.18, 58410000.0, 0.0, 0.0, 0.25, 0.335, 0.47};
struct VariantInfo { int nkeys; const char* const* keys; const double* defaults; };
// parameter set of a variant: by (chemistry, SEI, temperature); the mixed-precision variants share their fp64 sibling's
static VariantInfo variant_keys(int chem, int sei, int thermal, int rxn) {
  if (chem == PLH_CHEM_LGM50) return thermal ? VariantInfo{54, KEYS_LGM50_THERMAL, DEFAULTS_LGM50_THERMAL} : VariantInfo{33, KEYS_LGM50_ISO, DEFAULTS_LGM50_ISO};
  if (rxn == PLH_RXN_MHC) return {37, KEYS_LCO_MHC, DEFAULTS_LCO_MHC};
  if (thermal) return {56, KEYS_LCO_THERMAL, DEFAULTS_LCO_THERMAL};
  if (chem == PLH_CHEM_LCO_LIC6) return sei ? VariantInfo{42, KEYS_LCO_SEI, DEFAULTS_LCO_SEI} : VariantInfo{35, KEYS_LCO_ISO, DEFAULTS_LCO_ISO};
  return sei ? VariantInfo{39, KEYS_NMC_SEI, DEFAULTS_NMC_SEI} : VariantInfo{32, KEYS_NMC_ISO, DEFAULTS_NMC_ISO};
}
static const VariantOps* variant_ops(int id) {
  switch (id) {
#define PL_OPS_CASE(ID, CHEM, SEI, TH, MIX, SD, TF, RXN, W2) case ID: return plh_variant_ops_##ID ? plh_variant_ops_##ID() : nullptr;
    PL_VARIANT_LIST(PL_OPS_CASE)
#undef PL_OPS_CASE
  }
  return nullptr;
}
// libraries of variants compiled for other discretisations (plh_register_grid_library): kept loaded for the life of the process
struct GridLib { std::string path; void* handle; int grid[7]; const VariantOps* (*ops)(int); };
static std::vector<GridLib> g_grid_libs;
static std::mutex g_grid_mutex;
static bool desc_matches(const plh_model_desc* d, const VariantOps* o) {
  return o->chem == d->chemistry && o->sei == (d->aging_SEI ? 1 : 0) && o->thermal == (d->temperature ? 1 : 0) && o->mixed == d->precision &&
         o->sd == d->solid_diffusion && o->tf == d->thermodynamic_factor && o->rxn == d->rxn && o->w2 == (d->waves_per_cell == 2 ? 1 : 0);
}
// N_a / N_z only exist with temperature = true, N_r only for Fickian diffusion (params.jl:119-136); an absent dimension matches anything
static bool grid_matches(const plh_model_desc* d, const int* g) {
  if (d->N_p != g[0] || d->N_s != g[1] || d->N_n != g[2]) return false;
  if (d->solid_diffusion == PLH_SD_FICKIAN && (d->N_r_p != g[3] || d->N_r_n != g[6])) return false;
  if (d->temperature && (d->N_a != g[4] || d->N_z != g[5])) return false;
  return true;
}

// ---- per-handle state ----
struct StageBlock { void* p; size_t bytes; bool busy; };
// a device buffer of one stream that only grows.  An earlier launch on the stream may still be using the old block: growing waits for the stream before it frees it
struct DevBuf {
  void* d = nullptr; size_t cap = 0;
  void free() { if (d) hipFree(d); d = nullptr; cap = 0; }
  hipError_t regrow(size_t bytes) { free(); const hipError_t e = hipMalloc(&d, bytes); if (e == hipSuccess) cap = bytes; return e; }      // (the stream is known to be idle)
  hipError_t reserve(hipStream_t st, size_t bytes) {
    if (cap >= bytes) return hipSuccess;
    if (d) { const hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) return e; }
    return regrow(bytes);
  }
};
// a host array's device copy, kept per stream: uploaded again only when the caller's array differs from what is there, and then behind a stream synchronise (an earlier
// launch may still be reading the old copy).  keep = false: the array holds pointers to staging blocks of this call only -- uploaded, never remembered
template <class T> struct Uploaded {
  DevBuf buf; std::vector<T> on_device;
  int get(hipStream_t st, const std::vector<T>& v, const T** out, bool keep = true, size_t alloc_elems = 0) {
    *out = nullptr;
    if (v.empty()) return 0;
    if (!keep || v.size() != on_device.size() || memcmp(v.data(), on_device.data(), v.size() * sizeof(T)) != 0) {
      HIPCHK(hipStreamSynchronize(st));
      on_device.clear();
      if (buf.cap < v.size() * sizeof(T)) HIPCHK(buf.regrow(std::max(v.size(), alloc_elems) * sizeof(T)));
      HIPCHK(hipMemcpy(buf.d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
      if (keep) on_device = v;
    }
    *out = (const T*)buf.d; return 0;
  }
};
// what one in-flight launch needs: kept per stream, so that launches of one handle on different streams never share workspaces
struct StreamCtx {
  hipStream_t st = nullptr;
  DevBuf scratch;                                           // [n_cells][2][N]: previous accepted point of every cell (back-interpolation)
  DevBuf genW;                                              // [n_cells][N]: border vector of the general control row (closure inputs with derivative programs)
  Uploaded<plh_run> runs;                                   // the protocol (remembered when it is plain: a repeated launch with the same protocol uploads nothing and does not synchronise)
  Uploaded<double> tdiscon, tstops;                         // opts.tdiscon / opts.tstops, sorted
  Uploaded<int> sel;                                        // packed entry -> state index of plh_outputs.sel (Y_sel); allocated at N ints, the longest selection there is
  DevBuf resample;                                          // plh_resample: elimination factors, query locations and slopes of one chunk of cells (plh_resample.h, plrs::Work)
  Uploaded<double> lm_bounds;                               // plh_lm_step: shared bounds, lo[n_keys] then hi[n_keys] (remembered: the same for every iteration of a fit)
  Uploaded<int> group_off;                                  // plh_lsq_group / plh_group_scatter: the offsets of the groups (remembered: the same for every iteration of a grouped fit)
  Uploaded<double> resample_tq;                             // plh_resample: the query times (remembered: the fields of one ensemble are resampled on the same grid, one call each)
  hipEvent_t ev0 = nullptr, ev1 = nullptr; bool timed = false;
  std::vector<hipEvent_t> ret_ev;                           // one event per output array of a synchronous host call (host_return): grown on demand, kept
  std::vector<void*> pending;                               // staging blocks of PLH_HOST_ASYNC launches: released by plh_synchronize
};
struct plh_model_s {
  plh_model_desc desc;
  const VariantOps* ops = nullptr;
  int device = 0;
  int N = 0, Nd = 0, P = 0;        // states, differential states, theta entries
  const char* const* key_names = nullptr; const double* key_defaults = nullptr;
  Tables h_tb;
  Tables* d_tb = nullptr;
  std::vector<int> colptr[PLH_N_MODES], rowval[PLH_N_MODES];
  std::vector<unsigned> code[PLH_N_MODES];
  std::vector<int> alg_colptr[PLH_N_MODES], alg_rowval[PLH_N_MODES], alg_sel[PLH_N_MODES];     // J_y_alg block: pattern + positions in the full CSC order
  std::vector<void*> d_tables;     // device copies of the pattern tables (freed with the handle)
  int* d_alg_sel[PLH_N_MODES] = {};
  bool last_compiled = false;                                                  // the last plh_integrate ran the attached library's kernels
  const VariantOps* cl_ops = nullptr; unsigned long long cl_digest = 0;      // attached closure library (plh_model_attach_closure_library): its kernels, the protocol digest it was built for
  std::vector<StreamCtx*> streams;
  StreamCtx* last = nullptr;
  StreamCtx& ctx(hipStream_t st) {
    for (StreamCtx* c : streams) if (c->st == st) return *c;
    StreamCtx* c = new StreamCtx(); c->st = st; hipEventCreate(&c->ev0); hipEventCreate(&c->ev1); streams.push_back(c); return *c;
  }
  // device staging blocks of the host-pointer paths, kept between calls: a repeated call with the same shapes does no hipMalloc / hipFree
  std::vector<StageBlock> stage_cache;
  void* grab(size_t bytes) {
    int best = -1;
    for (size_t k = 0; k < stage_cache.size(); k++)
      if (!stage_cache[k].busy && stage_cache[k].bytes >= bytes && (best < 0 || stage_cache[k].bytes < stage_cache[best].bytes)) best = (int)k;
    if (best >= 0 && stage_cache[best].bytes <= 2 * bytes + 4096) { stage_cache[best].busy = true; return stage_cache[best].p; }
    void* d = nullptr; if (hipMalloc(&d, bytes ? bytes : 8) != hipSuccess) return nullptr;
    stage_cache.push_back({d, bytes, true}); return d;
  }
  void release(void* p) { for (auto& b : stage_cache) if (b.p == p) b.busy = false; }
  // pinned host bounce buffer for the device-to-host copies of the PLH_HOST path: hipMemcpy into fresh pageable pages (a caller that allocates
  // its output arrays per call) costs ~10x the DMA time in page pinning; DMA into this buffer + memcpy does not
  void* pin = nullptr; size_t pin_bytes = 0;
  void* pinned(size_t bytes) {
    if (bytes <= pin_bytes) return pin;
    if (pin) hipHostFree(pin);
    pin = nullptr; pin_bytes = 0;
    if (hipHostMalloc(&pin, bytes, hipHostMallocDefault) != hipSuccess) { pin = nullptr; return nullptr; }
    pin_bytes = bytes; return pin;
  }
};

// every entry point runs on the handle's device and restores the caller's
struct DeviceGuard {
  int prev = -1; bool switched = false;
  explicit DeviceGuard(int dev) {
#ifndef PL_WAVE_EMU
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) { switched = hipSetDevice(dev) == hipSuccess; }
#else
    (void)dev;
#endif
  }
  ~DeviceGuard() {
#ifndef PL_WAVE_EMU
    if (switched) hipSetDevice(prev);
#endif
  }
};

// ---- staging helpers: host arrays are copied through cached device blocks; every failure is remembered and reported before the launch ----
struct Stage {
  std::vector<void*> tmp;
  plh_model_s* m; int kind; hipStream_t st; StreamCtx* cx;
  bool bad = false; std::string why;
  Stage(plh_model_s* mm, int k, void* s) : m(mm), kind(k), st((hipStream_t)s), cx(&mm->ctx((hipStream_t)s)) {}
  ~Stage() { for (void* p : tmp) m->release(p); }
  void err(const char* what, hipError_t e) { if (!bad) { bad = true; why = std::string(what) + ": " + hipGetErrorString(e); } }
  void* dev_block(size_t bytes) {
    void* d = m->grab(bytes);
    if (!d) { if (!bad) { bad = true; why = "hipMalloc failed (staging block of " + std::to_string(bytes) + " bytes)"; } return nullptr; }
    tmp.push_back(d); return d;
  }
  void h2d(void* d, const void* p, size_t bytes) {
    const hipError_t e = kind == PLH_HOST_ASYNC ? hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, st) : hipMemcpy(d, p, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) err("host-to-device copy", e);
  }
  template <class T> const T* in(const T* p, size_t n) {
    if (!p || kind == PLH_DEVICE) return p;
    void* d = dev_block(n * sizeof(T)); if (!d) return nullptr;
    h2d(d, p, n * sizeof(T)); return (const T*)d;
  }
  // always-host inputs (protocol tables, per-cell protocol values, tdiscon): synchronous copies whatever the kind of the call
  template <class T> const T* in_host(const T* p, size_t n) {
    void* d = dev_block(n * sizeof(T)); if (!d) return nullptr;
    const hipError_t e = hipMemcpy(d, p, n * sizeof(T), hipMemcpyHostToDevice); if (e != hipSuccess) err("host-to-device copy", e);
    return (const T*)d;
  }
  template <class T> T* buf(T* p, size_t n, bool copy_in) {
    if (!p || kind == PLH_DEVICE) return p;
    void* d = dev_block(n * sizeof(T)); if (!d) return nullptr;
    if (copy_in) h2d(d, p, n * sizeof(T));
    return (T*)d;
  }
  template <class T> void back(T* host, const T* dev, size_t n) {
    if (!host || kind == PLH_DEVICE || bad) return;
    hipError_t e;
    if (kind == PLH_HOST_ASYNC) e = hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st);
    else {
      void* pb = n * sizeof(T) >= (64u << 10) ? m->pinned(n * sizeof(T)) : nullptr;
      if (pb) { e = hipMemcpy(pb, dev, n * sizeof(T), hipMemcpyDeviceToHost); if (e == hipSuccess) memcpy(host, pb, n * sizeof(T)); }
      else e = hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) err("device-to-host copy", e);
  }
  // PLH_HOST_ASYNC: the staging blocks stay busy until plh_synchronize
  void defer() { cx->pending.insert(cx->pending.end(), tmp.begin(), tmp.end()); tmp.clear(); }
};
// ---- r06: the way back of a synchronous host call (PLH_HOST): HostReturn below.  The caller's output pages are touched WHILE THE KERNEL RUNS (a caller that allocates its
// outputs per call -- numpy.empty, a Julia Vector{Float64}(undef, n) -- otherwise pays the first touch in the copy: a third of the kernel rate on C2 / C4)
struct HostRet { char* host; const char* dev; size_t rows, width, pitch, pin_off; };      // rows x width bytes; both sides keep their rows `pitch` bytes apart (one row: a plain copy)
// first touch of the caller's output pages (they are overwritten afterwards: writing a zero is harmless).  Rows longer than a page: only the pages the prefix copy can reach.
// r06b: ONE parallel region over all arrays (a thread team per array cost more in thread starts than the small arrays in faults), and the whole pages inside an array are
// populated by madvise(MADV_POPULATE_WRITE) (Linux >= 5.14: the kernel fills the page tables in one call instead of one trap per page -- measured on the GPU box, 13 MB of
// fresh anonymous memory: 0.43 ms against 0.99 ms for the touch loop on four threads, 100 MB: 2.7 against 8.2 ms; more threads lose: tools/gpu/host_ubench.hip); a kernel
// that does not know the advice falls back to the touch loop.
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
static void touch_pages(char* h, size_t bytes) { for (size_t k = 0; k < bytes; k += 4096) ((volatile char*)h)[k] = 0; if (bytes) ((volatile char*)h)[bytes - 1] = 0; }
static void populate(char* h, size_t bytes) {
  static std::atomic<int> have_populate{1};
  const uintptr_t PG = 4096, lo = ((uintptr_t)h + PG - 1) & ~(PG - 1), hi = ((uintptr_t)h + bytes) & ~(PG - 1);
  if (have_populate.load(std::memory_order_relaxed) && hi > lo) {
    if (madvise((void*)lo, hi - lo, MADV_POPULATE_WRITE) == 0) {
      ((volatile char*)h)[0] = 0; ((volatile char*)h)[bytes - 1] = 0;            // the partial pages at both ends
      return;
    }
    if (errno == EINVAL) have_populate.store(0, std::memory_order_relaxed);
  }
  touch_pages(h, bytes);
}
static void prefault(const std::vector<HostRet>& rets, size_t prefix_bytes_of_wide_rows) {
  const size_t PG = 4096;
  struct Piece { char* h; size_t bytes; };
  std::vector<Piece> pieces; size_t total = 0;
  for (const HostRet& r : rets) {
    if (!r.host) continue;
    if (r.rows <= 1 || r.pitch <= PG) {
      const size_t bytes = r.rows <= 1 ? r.width : r.rows * r.pitch;
      for (size_t o = 0; o < bytes; o += (1u << 20)) { pieces.push_back({r.host + o, std::min<size_t>(1u << 20, bytes - o)}); }          // 1 MB pieces: the unit of work sharing
      total += bytes;
    } else {
      const size_t span = std::min(r.width, prefix_bytes_of_wide_rows);
      for (size_t q = 0; q < r.rows; q++) pieces.push_back({r.host + q * r.pitch, span});
      total += r.rows * span;
    }
  }
  unsigned nt = (unsigned)std::min<size_t>(4, total / (1u << 20));
#ifdef PL_WAVE_EMU
  nt = 1;
#endif
  if (nt <= 1) { for (const Piece& pc : pieces) populate(pc.h, pc.bytes); return; }
  std::atomic<size_t> next{0};
  auto work = [&] { for (size_t k; (k = next.fetch_add(1, std::memory_order_relaxed)) < pieces.size();) populate(pieces[k].h, pieces[k].bytes); };
  std::vector<std::thread> th;
  for (unsigned k = 1; k < nt; k++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}
#define CHECK_MODEL(m) do { if (!(m)) return fail(PLH_E_ARG, "null model"); } while (0)
#define CHECK_MODE(mode) do { if ((mode) != PLH_MODE_I && (mode) != PLH_MODE_V && (mode) != PLH_MODE_P && (mode) != PLH_MODE_ETA_P && !((mode) == PLH_MODE_DT && m->desc.temperature)) \
    return fail(PLH_E_UNSUPPORTED, "operating mode not available for this model (I, V, P, eta_p; dT with temperature = true)"); } while (0)
#define CHECK_KIND(kind) do { if ((kind) != PLH_HOST && (kind) != PLH_DEVICE) return fail(PLH_E_ARG, "ptr_kind must be PLH_HOST or PLH_DEVICE here"); } while (0)
#define CHECK_STAGE(stage) do { if ((stage).bad) return fail(PLH_E_HIP, (stage).why); } while (0)
#define FINISH(stage) do { if ((stage).kind == PLH_HOST) HIPCHK(hipStreamSynchronize((stage).st)); HIPCHK(hipGetLastError()); } while (0)

template <class T> static int upload(plh_model_s* m, const std::vector<T>& v, const T** out) {
  void* d = nullptr;
  if (hipMalloc(&d, (v.size() ? v.size() : 1) * sizeof(T)) != hipSuccess) return PLH_E_HIP;
  m->d_tables.push_back(d);
  if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return PLH_E_HIP;
  *out = (const T*)d; return 0;
}

// CSC pattern + decode words per mode, the same entries in CSR order (refinement mat-vec), and the J_y_alg block
static int build_patterns(plh_model_s* m) {
  Tables& tb = m->h_tb;
  const int N = m->ops->N, Nd = m->ops->Nd;
  for (int mode = 0; mode < PLH_N_MODES; mode++) {
    if (mode == PLH_MODE_DT && !m->ops->thermal) continue;
    m->colptr[mode].assign(N + 1, 0);
    std::vector<std::vector<std::pair<int, unsigned>>> rows(N);
    for (int c = 0; c < N; c++) {
      for (int r = 0; r < N; r++) { const unsigned w = m->ops->classify(tb, mode, r, c); if (w) { m->rowval[mode].push_back(r); m->code[mode].push_back(w); rows[r].push_back({c, w}); } }
      m->colptr[mode][c + 1] = (int)m->rowval[mode].size();
    }
    tb.nnz[mode] = (int)m->rowval[mode].size();
    std::vector<int> rptr(N + 1, 0); std::vector<unsigned> rcode; std::vector<unsigned short> rcol;
    for (int r = 0; r < N; r++) { for (auto& e : rows[r]) { rcol.push_back((unsigned short)e.first); rcode.push_back(e.second); } rptr[r + 1] = (int)rcode.size(); }
    if (upload(m, m->code[mode], &tb.csc_code[mode]) || upload(m, rptr, &tb.csr_ptr[mode]) || upload(m, rcode, &tb.csr_code[mode]) || upload(m, rcol, &tb.csr_col[mode])) return PLH_E_HIP;
    // J_y_alg (generate_functions.jl:318-325): rows N_diff .. N-2 (the control row is not generated), columns N_diff .. N-1
    m->alg_colptr[mode].assign(N - Nd + 1, 0);
    for (int c = Nd; c < N; c++) {
      for (int q = m->colptr[mode][c]; q < m->colptr[mode][c + 1]; q++) {
        const int r = m->rowval[mode][q];
        if (r >= Nd && r < N - 1) { m->alg_rowval[mode].push_back(r - Nd); m->alg_sel[mode].push_back(q); }
      }
      m->alg_colptr[mode][c - Nd + 1] = (int)m->alg_rowval[mode].size();
    }
    const int* dsel = nullptr; if (upload(m, m->alg_sel[mode], &dsel)) return PLH_E_HIP;
    m->d_alg_sel[mode] = const_cast<int*>(dsel);
  }
  m->N = N; m->Nd = Nd;
  return 0;
}

// The communicator and the five transport operations plh_ensemble_run is written against (x_send / x_recv / x_bcast / x_allmin, grouped between x_group_start / _end).
// Product build: RCCL on the communicator's stream, device buffers.  Test-only wave-emulator build: a file-backed LOOPBACK between processes on one machine (one file per
// message in a directory named by the 128-byte id, written whole and renamed into place; receives poll with a timeout), so that the multi-rank control flow of the SAME
// function -- shard offsets, ragged and cyclic partitions, per-cell protocol shards, the status agreements, the gather re-ordering, failures on one rank -- runs with
// 2 or 3 processes on a machine without a GPU (tests/test_ensemble_loopback.py).  `dead`: a transport failure inside a collective phase leaves the fabric in an unknown
// state; the communicator is aborted (ncclCommAbort) and refuses further use instead of letting the caller walk into a hang.
#ifndef PL_WAVE_EMU
struct plh_comm_s { ncclComm_t comm = nullptr; int n_ranks = 1, rank = 0, device = 0; hipStream_t st = nullptr; int* d_status = nullptr; bool dead = false; };
#else
#include <unistd.h>
#include <sys/stat.h>
struct plh_comm_s { int n_ranks = 1, rank = 0, device = 0; std::string dir; std::vector<long long> seq_tx, seq_rx; int* d_status = nullptr; bool dead = false; bool comm = false; };
#endif

// a postfix program of the PLH_OP_* vocabulary (closure inputs, the stop function): checked here, the device interpreter trusts it
static int check_postfix(const double* ops, const double* args, int k0, int k1, int N, int P) {
  int sp = 0;
  for (int k = k0; k < k1; k++) {
    const double opd = ops[k]; const int op = (int)opd; const double a = args[k];
    if (!(opd == (double)op) || op < 0 || op >= PLH_N_OPS) return fail(PLH_E_ARG, "PLH_VAL_EXPR: unknown opcode");
    int pop = 2, idx_max = -1;
    if (op <= PLH_OP_THETA) pop = 0; else if (op == PLH_OP_SELECT) pop = 3;
    else if (op == PLH_OP_NEG || op == PLH_OP_SIN || op == PLH_OP_COS || op == PLH_OP_EXP || op == PLH_OP_LOG || op == PLH_OP_SQRT || op == PLH_OP_ABS || op == PLH_OP_TANH) pop = 1;
    if (op == PLH_OP_Y || op == PLH_OP_YP) idx_max = N; else if (op == PLH_OP_THETA) idx_max = P;
    if (idx_max >= 0 && !(a == (double)(int)a && a >= 0 && a < idx_max)) return fail(PLH_E_ARG, "PLH_VAL_EXPR: state / theta index out of range");
    if (sp < pop) return fail(PLH_E_ARG, "PLH_VAL_EXPR: stack underflow");
    sp += 1 - pop;
    if (sp > PLH_EXPR_STACK) return fail(PLH_E_ARG, "PLH_VAL_EXPR: more than 16 values on the stack");
  }
  if (sp != 1) return fail(PLH_E_ARG, "PLH_VAL_EXPR: the program must leave exactly one value");
  return 0;
}

extern "C" {

const char* plh_last_error(void) { return g_err.c_str(); }

int plh_model_create(const plh_model_desc* d, plh_model_t* out) {
  if (!d || !out) return fail(PLH_E_ARG, "null argument");
  if (d->real_bytes != 8) return fail(PLH_E_UNSUPPORTED, "states, residuals and time are fp64 (real_bytes = 8); reduced precision is selected with precision = PLH_PREC_MIXED");
  if (d->precision != PLH_PREC_F64 && d->precision != PLH_PREC_MIXED && d->precision != PLH_PREC_F64_REFORDER) return fail(PLH_E_ARG, "precision must be PLH_PREC_F64, PLH_PREC_MIXED or PLH_PREC_F64_REFORDER");
  if (d->chemistry != PLH_CHEM_LCO_LIC6 && d->chemistry != PLH_CHEM_NMC_LIC6 && d->chemistry != PLH_CHEM_LGM50) return fail(PLH_E_UNSUPPORTED, "unknown chemistry");
  if (d->solid_diffusion < 0 || d->solid_diffusion > PLH_SD_POLYNOMIAL || d->thermodynamic_factor < 0 || d->thermodynamic_factor > 1 || d->rxn < 0 || d->rxn > 1)
    return fail(PLH_E_ARG, "solid_diffusion / thermodynamic_factor / rxn out of range");
  if (d->waves_per_cell < 0 || d->waves_per_cell > 2) return fail(PLH_E_ARG, "waves_per_cell must be 0, 1 or 2");
  const VariantOps* ops = nullptr;
  bool variant_exists = false;
  for (int v = 0; v < PL_N_VARIANTS; v++) {
    const VariantOps* o = variant_ops(v);
    if (o && desc_matches(d, o)) { variant_exists = true; if (grid_matches(d, o->grid)) ops = o; }
  }
  if (!ops) {                                            // another discretisation: a registered grid library
    std::lock_guard<std::mutex> lk(g_grid_mutex);
    // (latest registration first: a library that failed the kernel self-test is superseded by its fall-back build, registered after it -- api.petlion)
    for (auto it = g_grid_libs.rbegin(); it != g_grid_libs.rend() && !ops; ++it) {
      const GridLib& gl = *it;
      if (!grid_matches(d, gl.grid)) continue;
      for (int v = 0; v < PL_N_VARIANTS && !ops; v++) { const VariantOps* o = gl.ops(v); if (o && desc_matches(d, o)) { variant_exists = true; ops = o; } }
    }
  }
  if (!ops && variant_exists)
    return fail(PLH_E_UNSUPPORTED, "discretisation: the library's built-in kernels are compiled for N_p = N_s = N_n = N_r_p = N_r_n = N_a = N_z = 10; another grid (2 <= N_p, N_s, N_n, "
                                   "N_p + N_s + N_n <= 48, 10 <= N_r_p, N_r_n <= 16) is one more build of csrc/variant_tu.hip, registered with plh_register_grid_library() before "
                                   "plh_model_create (petlion.jl_amd/grids.py does both; INTEGRATION.md)");
  if (!ops) return fail(PLH_E_UNSUPPORTED, "this chemistry / temperature / aging / precision / model-option combination is not instantiated on the device (built in fp64: LCO and NMC "
                                           "isothermal with or without SEI aging, LGM50 isothermal and with temperature, LCO with temperature; LCO isothermal with ONE of: quadratic or polynomial solid diffusion, the nonlinear "
                                           "thermodynamic factor, MHC kinetics; mixed precision: LCO isothermal, NMC + SEI, LCO with temperature)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(PLH_E_HIP, "no HIP device visible: the product path has no CPU fallback");
  int dev = d->device;
#ifndef PL_WAVE_EMU
  if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) return fail(PLH_E_HIP, "hipGetDevice failed"); }
  if (dev >= ndev) return fail(PLH_E_ARG, "device ordinal out of range");
#else
  dev = 0;
#endif
  DeviceGuard guard(dev);
  plh_model_s* m = new plh_model_s();
  m->desc = *d; m->desc.device = dev; m->device = dev; m->ops = ops;
  Tables& tb = m->h_tb;
  memset(&tb, 0, sizeof(tb));
  // radial operators of the variant's N_r_p / N_r_n: one block per electrode at the common stride S = max(N_r_p, N_r_n) -- M, LAM, V, W back to back, the smaller operator
  // zero-padded (rows, columns and modes that do not exist contribute nothing to any sum over S entries); the variant's kernels read them through Tables::Mp / LAMp / Vp / Wp
  { const int S = ops->grid[3] > ops->grid[6] ? ops->grid[3] : ops->grid[6];
    for (int el = 0; el < 2; el++) {
      const int nr = el == 0 ? ops->grid[3] : ops->grid[6];
      double* r = el == 0 ? tb.RAD : tb.RAD_N;
      for (int i = 0; i < nr; i++) {
        r[S * S + i] = ops->rad_LAM[el][i];
        for (int j = 0; j < nr; j++) { r[i * S + j] = ops->rad_M[el][i * nr + j]; r[S * S + S + i * S + j] = ops->rad_V[el][i * nr + j]; r[2 * S * S + S + i * S + j] = ops->rad_W[el][i * nr + j]; }
      }
    } }
  tb.BJ = ops->rad_BJ[0]; tb.BJ_N = ops->rad_BJ[1]; tb.chem = d->chemistry;
  const VariantInfo vi = variant_keys(ops->chem, ops->sei, ops->thermal, ops->rxn);
  m->P = vi.nkeys; m->key_names = vi.keys; m->key_defaults = vi.defaults;
  tb.P = m->P;
  for (int k = 0; k < K_COUNT; k++) {
    tb.thidx[k] = -1;
    for (int q = 0; q < m->P; q++) if (!strcmp(KEY_ENUM_NAMES[k], m->key_names[q])) tb.thidx[k] = q;
  }
  if (build_patterns(m) != 0) { plh_model_destroy(m); return fail(PLH_E_HIP, "pattern construction failed (hipMalloc / hipMemcpy)"); }
  if (hipMalloc((void**)&m->d_tb, sizeof(Tables)) != hipSuccess || hipMemcpy(m->d_tb, &tb, sizeof(Tables), hipMemcpyHostToDevice) != hipSuccess) {
    plh_model_destroy(m); return fail(PLH_E_HIP, "hipMalloc / hipMemcpy of the model tables failed");
  }
  *out = m;
  return 0;
}

int plh_register_grid_library(const char* path) {
  if (!path) return fail(PLH_E_ARG, "null path");
  std::lock_guard<std::mutex> lk(g_grid_mutex);
  for (const GridLib& gl : g_grid_libs) if (gl.path == path) return 0;
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) return fail(PLH_E_ARG, std::string("dlopen failed: ") + dlerror());
  GridLib gl; gl.path = path; gl.handle = h;
  gl.ops = (const VariantOps* (*)(int))dlsym(h, "plh_grid_variant_ops");
  void (*dims)(int*) = (void (*)(int*))dlsym(h, "plh_grid_dims");
  void (*abi)(int*, int*, int*, int*) = (void (*)(int*, int*, int*, int*))dlsym(h, "plh_grid_abi");
  if (!gl.ops || !dims || !abi) { dlclose(h); return fail(PLH_E_ARG, "not a grid library: plh_grid_variant_ops / plh_grid_dims / plh_grid_abi missing (petlion.jl_amd/grids.py builds one)"); }
  { int v = 0, so = 0, sa = 0, st = 0; abi(&v, &so, &sa, &st);
    if (v != PLH_HOST_ABI || so != (int)sizeof(VariantOps) || sa != (int)sizeof(IntegrateArgs) || st != (int)sizeof(Tables)) {
      dlclose(h); return fail(PLH_E_ARG, "grid library was built against another version of the host interface (stale cache: rebuild it, grids.library(..., force=True))"); } }
  dims(gl.grid);
  int found = 0;
  for (int v = 0; v < PL_N_VARIANTS; v++) {
    const VariantOps* o = gl.ops(v);
    if (!o) continue;
    if (memcmp(o->grid, gl.grid, sizeof(gl.grid)) != 0 || o->id != v) { dlclose(h); return fail(PLH_E_ARG, "grid library: variant table does not match the library's own dimensions (stale build?)"); }
    found++;
  }
  if (!found) { dlclose(h); return fail(PLH_E_ARG, "grid library holds no variant"); }
  g_grid_libs.push_back(gl);
  return 0;
}

// FNV-1a (64 bit) over the closure programs of a protocol as the kernels see them; petlion.jl_amd/closure_lib.py::digest computes the same number when it builds a library
static_assert(sizeof(plh_run) == 176, "plh_run: a field added outside the padding moves the others (bindings/julia, the ctypes mirror) -- and see DESIGN.md 5a");
unsigned long long plh_closure_digest(int n_runs, const plh_run* runs) {
  unsigned long long h = 0xcbf29ce484222325ull; bool any = false;
  auto feed = [&](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t k = 0; k < n; k++) { h ^= b[k]; h *= 0x100000001b3ull; } };
  for (int r = 0; r < n_runs; r++) {
    if (!runs || runs[r].value_kind != PLH_VAL_EXPR || !runs[r].tab_t || !runs[r].tab_v) continue;
    any = true;
    const int nd = runs[r].n_dcol > 0 ? runs[r].n_dcol : 0, n_all = nd > 0 ? runs[r].dofs[nd] : runs[r].n_tab;
    feed(&runs[r].n_tab, sizeof(int)); feed(runs[r].tab_t, (size_t)n_all * sizeof(double)); feed(runs[r].tab_v, (size_t)n_all * sizeof(double));
    feed(&nd, sizeof(int));
    if (nd > 0) { feed(runs[r].dcol, (size_t)nd * sizeof(int)); feed(runs[r].dofs, (size_t)(nd + 1) * sizeof(int)); }
  }
  return any ? h : 0ull;
}

int plh_model_attach_closure_library(plh_model_t m, const char* path) {
  CHECK_MODEL(m);
  if (!path) { m->cl_ops = nullptr; m->cl_digest = 0; return 0; }      // (r06) NULL detaches: every closure runs in the interpreter again (how compile_closures verifies a library)
  void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);          // (kept loaded for the life of the process, like a grid library)
  if (!h) return fail(PLH_E_ARG, std::string("dlopen failed: ") + dlerror());
  auto ops = (const VariantOps* (*)(int))dlsym(h, "plh_grid_variant_ops");
  auto dims = (void (*)(int*))dlsym(h, "plh_grid_dims");
  auto abi = (void (*)(int*, int*, int*, int*))dlsym(h, "plh_grid_abi");
  auto dig = (unsigned long long (*)())dlsym(h, "plh_closure_library_digest");
  if (!ops || !dims || !abi || !dig) { dlclose(h); return fail(PLH_E_ARG, "not a closure library (petlion.jl_amd/closure_lib.py builds one)"); }
  { int v = 0, so = 0, sa = 0, st = 0; abi(&v, &so, &sa, &st);
    if (v != PLH_HOST_ABI || so != (int)sizeof(VariantOps) || sa != (int)sizeof(IntegrateArgs) || st != (int)sizeof(Tables)) {
      dlclose(h); return fail(PLH_E_ARG, "closure library was built against another version of the host interface (stale cache: rebuild it)"); } }
  int g[7]; dims(g);
  const VariantOps* o = ops(m->ops->id);
  if (!o || memcmp(g, m->ops->grid, sizeof(g)) != 0 || !desc_matches(&m->desc, o)) { dlclose(h); return fail(PLH_E_ARG, "closure library: built for another model variant or discretisation"); }
  m->cl_ops = o; m->cl_digest = dig();
  return 0;
}

int plh_last_integrate_compiled(plh_model_t m) { return m && m->last_compiled ? 1 : 0; }

void plh_model_destroy(plh_model_t m) {
  if (!m) return;
  DeviceGuard guard(m->device);
  for (void* p : m->d_tables) hipFree(p);
  if (m->d_tb) hipFree(m->d_tb);
  for (StreamCtx* c : m->streams) {
    for (DevBuf* b : {&c->scratch, &c->genW, &c->runs.buf, &c->tdiscon.buf, &c->tstops.buf, &c->sel.buf, &c->resample, &c->resample_tq.buf, &c->lm_bounds.buf, &c->group_off.buf}) b->free();
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);
    for (hipEvent_t e : c->ret_ev) hipEventDestroy(e);
    delete c;
  }
  for (auto& b : m->stage_cache) hipFree(b.p);
  if (m->pin) hipHostFree(m->pin);
  delete m;
}

int plh_n_states(plh_model_t m) { return m ? m->N : PLH_E_ARG; }
int plh_n_diff(plh_model_t m) { return m ? m->Nd : PLH_E_ARG; }
int plh_n_theta(plh_model_t m) { return m ? m->P : PLH_E_ARG; }
const char* plh_theta_key(plh_model_t m, int i) { return (m && i >= 0 && i < m->P) ? m->key_names[i] : nullptr; }
double plh_theta_default(plh_model_t m, int i) { return (m && i >= 0 && i < m->P) ? m->key_defaults[i] : NAN; }
int plh_lds_bytes(plh_model_t m) { return m ? (int)m->ops->lds_bytes : PLH_E_ARG; }

int plh_n_sections(plh_model_t m) { if (!m) return PLH_E_ARG; SectionInfo s[12]; return m->ops->sections(s); }
int plh_section(plh_model_t m, int i, const char** name, int* start, int* len) {
  if (!m) return fail(PLH_E_ARG, "null model");
  SectionInfo s[12]; const int n = m->ops->sections(s);
  if (i < 0 || i >= n) return fail(PLH_E_ARG, "section index out of range");
  if (name) *name = s[i].name; if (start) *start = s[i].start; if (len) *len = s[i].len;
  return 0;
}

int plh_jac_pattern(plh_model_t m, int mode, int* nnz, int* colptr, int* rowval) {
  if (!m || !nnz) return fail(PLH_E_ARG, "null argument");
  if (mode < 0 || mode >= PLH_N_MODES || m->rowval[mode].empty()) return fail(PLH_E_UNSUPPORTED, "mode not available for this model");
  *nnz = (int)m->rowval[mode].size();
  if (colptr) memcpy(colptr, m->colptr[mode].data(), (m->N + 1) * sizeof(int));
  if (rowval) memcpy(rowval, m->rowval[mode].data(), m->rowval[mode].size() * sizeof(int));
  return 0;
}
int plh_jac_alg_pattern(plh_model_t m, int mode, int* nnz, int* colptr, int* rowval) {
  if (!m || !nnz) return fail(PLH_E_ARG, "null argument");
  if (mode < 0 || mode >= PLH_N_MODES || m->rowval[mode].empty()) return fail(PLH_E_UNSUPPORTED, "mode not available for this model");
  *nnz = (int)m->alg_rowval[mode].size();
  if (colptr) memcpy(colptr, m->alg_colptr[mode].data(), (m->N - m->Nd + 1) * sizeof(int));
  if (rowval) memcpy(rowval, m->alg_rowval[mode].data(), m->alg_rowval[mode].size() * sizeof(int));
  return 0;
}

// what this binary was built with (hipcc / clang versions, a hash of the per-variant compiler flags, a hash of the device and host sources): __graft_entry__.build_hip
// passes it to this translation unit.  A kernel of this size sits at the register allocator's limits, and one build was seen to miscompile one instantiation:
// the host compares this string with the one of the binary the committed GPU test run validated (profiles/validated_build.json) and runs the kernel self-test when they differ.
#ifndef PLH_BUILD_INFO
#define PLH_BUILD_INFO "unrecorded build (no -DPLH_BUILD_INFO: not built by __graft_entry__.build_hip)"
#endif
const char* plh_build_info(void) { return PLH_BUILD_INFO; }
int plh_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

int plh_abi_layout(int* out, int cap) {
  std::vector<int> v;
#define PL_S(T, NF) v.push_back((int)sizeof(T)); v.push_back(NF);
#define PL_F(T, f) v.push_back((int)offsetof(T, f));
  PL_S(plh_model_desc, 17) PL_F(plh_model_desc, chemistry) PL_F(plh_model_desc, N_p) PL_F(plh_model_desc, N_s) PL_F(plh_model_desc, N_n) PL_F(plh_model_desc, N_a)
  PL_F(plh_model_desc, N_z) PL_F(plh_model_desc, N_r_p) PL_F(plh_model_desc, N_r_n) PL_F(plh_model_desc, temperature) PL_F(plh_model_desc, aging_SEI)
  PL_F(plh_model_desc, real_bytes) PL_F(plh_model_desc, precision) PL_F(plh_model_desc, device) PL_F(plh_model_desc, solid_diffusion)
  PL_F(plh_model_desc, thermodynamic_factor) PL_F(plh_model_desc, rxn) PL_F(plh_model_desc, waves_per_cell)
  PL_S(plh_bounds, 11) PL_F(plh_bounds, V_max) PL_F(plh_bounds, V_min) PL_F(plh_bounds, SOC_max) PL_F(plh_bounds, SOC_min) PL_F(plh_bounds, T_max) PL_F(plh_bounds, c_s_n_max)
  PL_F(plh_bounds, I_max) PL_F(plh_bounds, I_min) PL_F(plh_bounds, eta_plating_min) PL_F(plh_bounds, c_e_min) PL_F(plh_bounds, dfilm_max)
  PL_S(plh_run, 15) PL_F(plh_run, mode) PL_F(plh_run, value_kind) PL_F(plh_run, value) PL_F(plh_run, tf) PL_F(plh_run, bounds) PL_F(plh_run, n_tab) PL_F(plh_run, closure_id) PL_F(plh_run, tab_t)
  PL_F(plh_run, tab_v) PL_F(plh_run, value_cell) PL_F(plh_run, tf_cell) PL_F(plh_run, n_dcol) PL_F(plh_run, dstate) PL_F(plh_run, dcol) PL_F(plh_run, dofs)
  PL_S(plh_opts, 19) PL_F(plh_opts, abstol) PL_F(plh_opts, reltol) PL_F(plh_opts, abstol_init) PL_F(plh_opts, reltol_init) PL_F(plh_opts, maxiters) PL_F(plh_opts, check_bounds)
  PL_F(plh_opts, interp_final) PL_F(plh_opts, max_order) PL_F(plh_opts, jac_every_step) PL_F(plh_opts, init_step) PL_F(plh_opts, n_tdiscon) PL_F(plh_opts, tdiscon) PL_F(plh_opts, refine)
  PL_F(plh_opts, n_tstops) PL_F(plh_opts, tstops) PL_F(plh_opts, yp_alg_zero) PL_F(plh_opts, n_stop) PL_F(plh_opts, stop_ops) PL_F(plh_opts, stop_args)
  PL_S(plh_run_info, 7) PL_F(plh_run_info, flag) PL_F(plh_run_info, iterations) PL_F(plh_run_info, t_end) PL_F(plh_run_info, V) PL_F(plh_run_info, I) PL_F(plh_run_info, SOC)
  PL_F(plh_run_info, T_avg)
  PL_S(plh_counters, 11) PL_F(plh_counters, n_steps) PL_F(plh_counters, n_res) PL_F(plh_counters, n_jac) PL_F(plh_counters, n_fact) PL_F(plh_counters, n_solve)
  PL_F(plh_counters, n_newton) PL_F(plh_counters, n_errfail) PL_F(plh_counters, n_convfail) PL_F(plh_counters, sum_kp2) PL_F(plh_counters, n_init_iters) PL_F(plh_counters, cyc)
  PL_S(plh_outputs, 15) PL_F(plh_outputs, max_pts) PL_F(plh_outputs, t) PL_F(plh_outputs, V) PL_F(plh_outputs, I) PL_F(plh_outputs, SOC) PL_F(plh_outputs, T_avg)
  PL_F(plh_outputs, n_pts) PL_F(plh_outputs, Y_final) PL_F(plh_outputs, YP_final) PL_F(plh_outputs, run_info) PL_F(plh_outputs, counters) PL_F(plh_outputs, Y_all)
  PL_F(plh_outputs, n_sel) PL_F(plh_outputs, sel) PL_F(plh_outputs, Y_sel)
#undef PL_S
#undef PL_F
  for (int k = 0; k < (int)v.size() && k < cap; k++) if (out) out[k] = v[k];
  return (int)v.size();
}

int plh_initial_guess(plh_model_t m, int n, const double* theta, const double* SOC, double* Y, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind); if (n <= 0 || !theta || !SOC || !Y) return fail(PLH_E_ARG, "bad argument");
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  const double* th = s.in(theta, (size_t)n * m->P); const double* so = s.in(SOC, n); double* y = s.buf(Y, (size_t)n * m->N, false);
  CHECK_STAGE(s);
  m->ops->initial_guess(s.st, m->d_tb, n, th, so, y);
  FINISH(s); s.back(Y, y, (size_t)n * m->N); CHECK_STAGE(s);
  return 0;
}

static int residual_rows(plh_model_t m, int n, const double* theta, const double* Y, const double* YP, int mode, double value, double* F, int row0, int nrows, int kind, void* stream) {
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  const double* th = s.in(theta, (size_t)n * m->P); const double* y = s.in(Y, (size_t)n * m->N); const double* yp = s.in(YP, (size_t)n * m->N);
  double* f = s.buf(F, (size_t)n * nrows, false);
  CHECK_STAGE(s);
  m->ops->residual(s.st, m->d_tb, n, th, y, yp, mode, value, f, row0, nrows);
  FINISH(s); s.back(F, f, (size_t)n * nrows); CHECK_STAGE(s);
  return 0;
}
int plh_residual(plh_model_t m, int n, const double* theta, const double* Y, const double* YP, int mode, double value, double* F, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_MODE(mode); CHECK_KIND(kind); if (n <= 0 || !theta || !Y || !YP || !F) return fail(PLH_E_ARG, "bad argument");
  return residual_rows(m, n, theta, Y, YP, mode, value, F, 0, m->N, kind, stream);
}
int plh_residual_diff(plh_model_t m, int n, const double* theta, const double* Y, const double* YP, double* out, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind); if (n <= 0 || !theta || !Y || !YP || !out) return fail(PLH_E_ARG, "bad argument");
  return residual_rows(m, n, theta, Y, YP, PLH_MODE_I, 0.0, out, 0, m->Nd, kind, stream);
}
int plh_residual_alg(plh_model_t m, int n, const double* theta, const double* Y, const double* YP, double* out, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind); if (n <= 0 || !theta || !Y || !YP || !out) return fail(PLH_E_ARG, "bad argument");
  return residual_rows(m, n, theta, Y, YP, PLH_MODE_I, 0.0, out, m->Nd, m->N - m->Nd - 1, kind, stream);
}

static int jacobian_sel(plh_model_t m, int n, const double* theta, const double* Y, const double* YP, double cj, int mode, double* nzval, const int* sel, size_t nnz, int kind, void* stream) {
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  const double* th = s.in(theta, (size_t)n * m->P); const double* y = s.in(Y, (size_t)n * m->N); const double* yp = s.in(YP, (size_t)n * m->N);
  double* z = s.buf(nzval, (size_t)n * nnz, false);
  CHECK_STAGE(s);
  m->ops->jacobian(s.st, m->d_tb, n, th, y, yp, cj, mode, z, sel, (int)nnz);
  FINISH(s); s.back(nzval, z, (size_t)n * nnz); CHECK_STAGE(s);
  return 0;
}
int plh_jacobian(plh_model_t m, int n, const double* theta, const double* Y, const double* YP, double cj, int mode, double* nzval, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_MODE(mode); CHECK_KIND(kind); if (n <= 0 || !theta || !Y || !YP || !nzval) return fail(PLH_E_ARG, "bad argument");
  return jacobian_sel(m, n, theta, Y, YP, cj, mode, nzval, nullptr, m->rowval[mode].size(), kind, stream);
}
int plh_jacobian_alg(plh_model_t m, int n, const double* theta, const double* Y, const double* YP, int mode, double* nzval, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_MODE(mode); CHECK_KIND(kind); if (n <= 0 || !theta || !Y || !YP || !nzval) return fail(PLH_E_ARG, "bad argument");
  return jacobian_sel(m, n, theta, Y, YP, 0.0, mode, nzval, m->d_alg_sel[mode], m->alg_sel[mode].size(), kind, stream);
}

int plh_linear_solve_refined(plh_model_t m, int n, const double* theta, const double* Y, const double* YP, double cj, int mode, double* b, int nref, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_MODE(mode); CHECK_KIND(kind); if (n <= 0 || !theta || !Y || !YP || !b || nref < 0) return fail(PLH_E_ARG, "bad argument");
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  const double* th = s.in(theta, (size_t)n * m->P); const double* y = s.in(Y, (size_t)n * m->N); const double* yp = s.in(YP, (size_t)n * m->N);
  double* bb = s.buf(b, (size_t)n * m->N, true);
  CHECK_STAGE(s);
  m->ops->linear_solve(s.st, m->d_tb, n, th, y, yp, cj, mode, bb, nref);
  FINISH(s); s.back(b, bb, (size_t)n * m->N); CHECK_STAGE(s);
  return 0;
}
int plh_linear_solve(plh_model_t m, int n, const double* theta, const double* Y, const double* YP, double cj, int mode, double* b, int kind, void* stream) {
  return plh_linear_solve_refined(m, n, theta, Y, YP, cj, mode, b, 0, kind, stream);
}

int plh_init_consistent(plh_model_t m, int n, const double* theta, int mode, double value, double reltol_init, double* Y, double* YP, int* status,
                        int* iters, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_MODE(mode); CHECK_KIND(kind); if (n <= 0 || !theta || !Y || !YP) return fail(PLH_E_ARG, "bad argument");
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  const double* th = s.in(theta, (size_t)n * m->P);
  double* y = s.buf(Y, (size_t)n * m->N, true); double* yp = s.buf(YP, (size_t)n * m->N, false);
  int* st = s.buf(status, n, false); int* it = s.buf(iters, n, false);
  CHECK_STAGE(s);
  m->ops->init_consistent(s.st, m->d_tb, n, th, mode, value, reltol_init, y, yp, st, it, 0);
  FINISH(s);
  s.back(Y, y, (size_t)n * m->N); s.back(YP, yp, (size_t)n * m->N); s.back(status, st, n); s.back(iters, it, n); CHECK_STAGE(s);
  return 0;
}

// ---- r06b: the copy kernels of a blocking host call's way back.  The outputs travel to the pinned block by KERNELS that store into mapped host memory (54 GB/s on the GPU box,
// the rate of one large blocking hipMemcpy; a chain of hipMemcpyAsync / hipMemcpy2DAsync commands with events between them reached 30 ... 40 GB/s), and the whole chain is
// queued BEHIND the integrate kernel before it ends: no host round trip between the kernel and the first byte on the bus.  The per-point arrays are packed to the longest
// trajectory of the call (row r of an array lands at r x maxn x elem), which the device works out itself (k_max_npts).
__host__ __device__ inline void pack_word(const char* src, size_t pitch, size_t w8, size_t row0, char* dst, size_t q) {
  const size_t r = row0 + q / w8, c = q % w8;
  ((double*)(dst + r * w8 * 8))[c] = ((const double*)(src + r * pitch))[c];
}
#ifndef PL_WAVE_EMU
__global__ void k_max_npts(const int* n_pts, int n, int mp, int* maxn_dev, int* host_hdr, int* host_npts) {          // one workgroup
  __shared__ int sm[256];
  int v = 0;
  for (int i = threadIdx.x; i < n; i += 256) { const int x = n_pts[i]; host_npts[i] = x; v = x > v ? x : v; }
  sm[threadIdx.x] = v; __syncthreads();
  for (int k = 128; k > 0; k >>= 1) { if ((int)threadIdx.x < k && sm[threadIdx.x + k] > sm[threadIdx.x]) sm[threadIdx.x] = sm[threadIdx.x + k]; __syncthreads(); }
  if (threadIdx.x == 0) { const int mx = sm[0] < mp ? sm[0] : mp; *maxn_dev = mx; *host_hdr = mx; }
}
__global__ void k_pack_rows(const char* src, size_t pitch, size_t elem8, const int* maxn_dev, size_t row0, size_t rows, char* dst) {
  const size_t w8 = (size_t)(*maxn_dev) * elem8, total = rows * w8;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) pack_word(src, pitch, w8, row0, dst, q);
}
__global__ void k_copy_words(const double* src, double* dst, size_t n8) {
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n8; q += (size_t)gridDim.x * blockDim.x) dst[q] = src[q];
}
#endif
static void launch_max_npts(hipStream_t st, const int* n_pts, int n, int mp, int* maxn_dev, int* host_hdr, int* host_npts) {
#ifndef PL_WAVE_EMU
  hipLaunchKernelGGL(k_max_npts, dim3(1), dim3(256), 0, st, n_pts, n, mp, maxn_dev, host_hdr, host_npts);
#else
  (void)st; int v = 0; for (int i = 0; i < n; i++) { host_npts[i] = n_pts[i]; v = std::max(v, n_pts[i]); } *maxn_dev = *host_hdr = std::min(v, mp);
#endif
}
static void launch_pack_rows(hipStream_t st, const char* src, size_t pitch, size_t elem8, const int* maxn_dev, size_t row0, size_t rows, size_t worst_w8, char* dst) {
#ifndef PL_WAVE_EMU
  const size_t blocks = std::min<size_t>(2048, (rows * worst_w8 + 255) / 256);
  hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)std::max<size_t>(1, blocks)), dim3(256), 0, st, src, pitch, elem8, maxn_dev, row0, rows, dst);
#else
  (void)st; (void)worst_w8; const size_t w8 = (size_t)(*maxn_dev) * elem8; for (size_t q = 0; q < rows * w8; q++) pack_word(src, pitch, w8, row0, dst, q);
#endif
}
static void launch_copy_words(hipStream_t st, const void* src, void* dst, size_t bytes) {
#ifndef PL_WAVE_EMU
  const size_t n8 = (bytes + 7) / 8, blocks = std::min<size_t>(2048, (n8 + 255) / 256);
  hipLaunchKernelGGL(k_copy_words, dim3((unsigned)std::max<size_t>(1, blocks)), dim3(256), 0, st, (const double*)src, (double*)dst, n8);
#else
  (void)st; memcpy(dst, src, bytes);
#endif
}
// forward parameter sensitivities of a plh_integrate_sens call (dfn_sens.h)
struct SensReq { int n_sens; const int* cols; double* dY; double* dV; int* stat; double* dI; double* dT; mutable double* d_dI; mutable double* d_dT; };      // (dI, dT: the further per-point channels of plh_integrate_sens_out; d_*: where the kernel writes them)
// theta_pert[cell][k][:] = the cell's theta row with column cols[k] moved by a relative 1e-7 (an absolute 1e-7 where the entry is zero)
__host__ __device__ inline void theta_pert_entry(const double* theta, const int* cols, int n_sens, int P, double* out, size_t q) {
  const int col = (int)(q % P), k = (int)((q / P) % n_sens); const size_t cell = q / ((size_t)P * n_sens);
  const double v = theta[cell * P + col];
  out[q] = col == cols[k] ? (v != 0.0 ? v * (1.0 + 1e-7) : 1e-7) : v;
}
#ifndef PL_WAVE_EMU
__global__ void k_theta_pert(const double* theta, const int* cols, int n_cells, int n_sens, int P, double* out) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < (size_t)n_cells * n_sens * P) theta_pert_entry(theta, cols, n_sens, P, out, q);
}
#endif
static void launch_theta_pert(hipStream_t st, const double* theta, const int* cols, int n_cells, int n_sens, int P, double* out) {
  const size_t tot = (size_t)n_cells * n_sens * P;
#ifndef PL_WAVE_EMU
  hipLaunchKernelGGL(k_theta_pert, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, theta, cols, n_cells, n_sens, P, out);
#else
  (void)st; for (size_t q = 0; q < tot; q++) theta_pert_entry(theta, cols, n_sens, P, out, q);      // (the emulator's "device" memory is host memory)
#endif
}

// ---- plh_integrate / plh_integrate_sens: the argument rules.  Pure host code, no HIP call; each function returns the first complaint, and integrate_impl calls them in
// the order the rules were always tested in (protocol, outputs, t_init, options, sensitivities), so a call that is wrong in several ways hears about the same one ----
// entries of the general control row of a closure with derivative programs: one per lane -- the input method's own (<= 3), one per Y column, and for a YP column the
// algebraic entries of that state's row (consistent-initialisation form), counted on the exported pattern
static int control_row_entries(const plh_model_s* m, const plh_run& run) {
  int n_entries = 3, n_y = 0;
  for (int k = 0; k < run.n_dcol; k++) {
    const int c = run.dcol[k];
    if (c < m->N) { n_y++; continue; }
    int tw = 0;
    for (int cc = m->ops->Nd; cc < m->N; cc++) for (int q = m->colptr[PLH_MODE_I][cc]; q < m->colptr[PLH_MODE_I][cc + 1]; q++) tw += m->rowval[PLH_MODE_I][q] == c - m->N;
    n_entries += tw > 1 ? tw : 1;
  }
  return n_entries + n_y;
}
// a closure input as postfix programs (PLH_VAL_EXPR): checked here, the device interpreter trusts them
static int check_closure(const plh_model_s* m, const plh_run& run) {
  if (run.n_tab < 1 || !run.tab_t || !run.tab_v) return fail(PLH_E_ARG, "PLH_VAL_EXPR needs n_tab >= 1 and both program arrays");
  if (run.mode == PLH_MODE_DT) return fail(PLH_E_UNSUPPORTED, "function inputs for dT are not defined by the reference");
  if (int rc = check_postfix(run.tab_t, run.tab_v, 0, run.n_tab, m->N, m->P)) return rc;
  if (run.n_dcol < 0 || run.n_dcol > PLH_MAX_DCOL) return fail(PLH_E_ARG, "PLH_VAL_EXPR: n_dcol out of range (0 .. 60)");
  if (run.n_dcol == 0) return 0;                                      // else: derivative programs of the control row, behind the main program in the same arrays
  if (!run.dcol || !run.dofs || run.dofs[0] < run.n_tab) return fail(PLH_E_ARG, "PLH_VAL_EXPR: n_dcol > 0 needs dcol, dofs and dofs[0] >= n_tab");
  for (int k = 0; k < run.n_dcol; k++) {
    // columns 0 .. N-1: d f / d Y[c]; N + i: d f / d YP[i] of a differential state i
    if (run.dcol[k] < 0 || run.dcol[k] >= m->N + m->ops->Nd || (k > 0 && run.dcol[k] <= run.dcol[k - 1]))
      return fail(PLH_E_ARG, "PLH_VAL_EXPR: dcol must be ascending columns (0 .. N-1 for Y, N + i for YP of a differential state i)");
    if (run.dofs[k + 1] <= run.dofs[k]) return fail(PLH_E_ARG, "PLH_VAL_EXPR: dofs must be increasing");
    if (int rc = check_postfix(run.tab_t, run.tab_v, run.dofs[k], run.dofs[k + 1], m->N, m->P)) return rc;
  }
  if (control_row_entries(m, run) > 64) return fail(PLH_E_UNSUPPORTED, "PLH_VAL_EXPR: the control row of this closure has more than 64 entries (columns read + Jacobian entries of the differential states whose YP it reads)");
  return 0;
}
static int check_runs(const plh_model_s* m, int n, int n_runs, const plh_run* runs, const double* Y_init) {
  for (int r = 0; r < n_runs; r++) {
    const plh_run& run = runs[r];
    if (run.mode == PLH_MODE_RES) {                              // user-defined control residual: a closure of Y with its derivative programs
      if (run.value_kind != PLH_VAL_EXPR || run.n_dcol < 1)
        return fail(PLH_E_UNSUPPORTED, "PLH_MODE_RES needs a PLH_VAL_EXPR closure of the state with derivative programs (n_dcol >= 1; closures of YP are not supported)");
    } else if (run.mode == PLH_MODE_DSTATE) {                    // rate of one differential state held (dc_s_* / dc_e_*): continues a solution
      if (run.dstate < PLH_DSTATE_CS_P_MAX || run.dstate > PLH_DSTATE_CE_MIN) return fail(PLH_E_ARG, "PLH_MODE_DSTATE: plh_run.dstate must be a PLH_DSTATE_* constant");
      if (run.value_kind != PLH_VAL_CONST && run.value_kind != PLH_VAL_HOLD) return fail(PLH_E_ARG, "PLH_MODE_DSTATE takes a constant value or :hold");
      if (r == 0 && !Y_init) return fail(PLH_E_ARG, "PLH_MODE_DSTATE chooses its state from the end of the previous run: it cannot be the first run of a new solution");
    } else CHECK_MODE(run.mode);
    if (run.value_kind < 0 || run.value_kind > PLH_VAL_EXPR) return fail(PLH_E_ARG, "bad value_kind");
    if (run.value_kind == PLH_VAL_EXPR) { if (int rc = check_closure(m, run)) return rc; }
    if (run.value_kind == PLH_VAL_TABLE) {
      if (run.n_tab < 1 || !run.tab_t || !run.tab_v) return fail(PLH_E_ARG, "PLH_VAL_TABLE needs n_tab >= 1 and both table arrays");
      if (run.mode == PLH_MODE_DT) return fail(PLH_E_UNSUPPORTED, "time-dependent dT inputs are not defined by the reference");
      for (int k = 1; k < run.n_tab; k++) if (!(run.tab_t[k] >= run.tab_t[k - 1])) return fail(PLH_E_ARG, "table times must be non-decreasing");
    }
    if (!(run.tf > 0)) return fail(PLH_E_ARG, "run length tf must be positive");
    if (run.value_cell && run.value_kind != PLH_VAL_CONST) return fail(PLH_E_ARG, "value_cell needs PLH_VAL_CONST");
    if (run.tf_cell) for (int c = 0; c < n; c++) if (!(run.tf_cell[c] > 0)) return fail(PLH_E_ARG, "run length tf_cell must be positive");
  }
  return 0;
}
// max_pts and the selected state entries per saved point (plh_outputs.sel / Y_sel): refused, never clamped.  sel_map: packed entry -> state index, in the order the ranges were given
static int check_outputs(const plh_model_s* m, const plh_outputs* out, std::vector<int>* sel_map) {
  if (out->max_pts < 0) return fail(PLH_E_ARG, "max_pts");
  if (out->n_sel < 0 || out->n_sel > 16) return fail(PLH_E_ARG, "plh_outputs.n_sel must be 0 .. 16");
  if (out->n_sel > 0 && !out->sel) return fail(PLH_E_ARG, "plh_outputs.n_sel > 0 needs sel");
  if (out->Y_sel && out->n_sel == 0) return fail(PLH_E_ARG, "plh_outputs.Y_sel needs n_sel >= 1 ranges in sel");
  std::vector<char> taken(m->N, 0);
  for (int q = 0; q < out->n_sel; q++) {
    const long long st = out->sel[2 * q], ln = out->sel[2 * q + 1];
    if (st < 0 || ln < 1 || st + ln > m->N) return fail(PLH_E_ARG, "plh_outputs.sel: every range (start, len) must have len >= 1 and lie inside [0, n_states)");
    for (long long k = st; k < st + ln; k++) {
      if (taken[k]) return fail(PLH_E_ARG, "plh_outputs.sel: ranges may not overlap");
      taken[k] = 1; sel_map->push_back((int)k);
    }
  }
  return 0;
}
static int check_opts(const plh_model_s* m, const plh_opts* opts) {
  if (opts->n_tdiscon < 0 || (opts->n_tdiscon > 0 && !opts->tdiscon)) return fail(PLH_E_ARG, "tdiscon");
  if (opts->n_tstops < 0 || (opts->n_tstops > 0 && !opts->tstops)) return fail(PLH_E_ARG, "tstops");
  for (int k = 0; k < opts->n_tstops; k++) if (!(opts->tstops[k] == opts->tstops[k])) return fail(PLH_E_ARG, "tstops must not contain NaN");
  if (opts->refine < 0 || opts->refine > 4) return fail(PLH_E_ARG, "refine must be 0 .. 4");
  if (opts->n_stop < 0 || (opts->n_stop > 0 && (!opts->stop_ops || !opts->stop_args))) return fail(PLH_E_ARG, "stop function: n_stop > 0 needs both program arrays");
  if (opts->n_stop > 0) { if (int rc = check_postfix(opts->stop_ops, opts->stop_args, 0, opts->n_stop, m->N, m->P)) return rc; }
  if (opts->n_stop > 0 && m->ops->w2) return fail(PLH_E_UNSUPPORTED, "stop function: one wavefront per cell only");
  return 0;
}
static int check_sens(const plh_model_s* m, const SensReq* sq, int n_runs, const plh_run* runs, const plh_opts* opts, const double* Y_init) {
  if (sq->n_sens < 1 || sq->n_sens > 64 || !sq->cols || (!sq->dY && !sq->dV && !sq->dI && !sq->dT))
    return fail(PLH_E_ARG, "plh_integrate_sens: 1 <= n_sens <= 64, theta columns and at least one of dY_dtheta / dV_dtheta");      // (plh_integrate_sens_out: or dI_dtheta / dT_avg_dtheta)
  for (int k = 0; k < sq->n_sens; k++) if (sq->cols[k] < 0 || sq->cols[k] >= m->P) return fail(PLH_E_ARG, "plh_integrate_sens: theta column out of range");
  if (Y_init) return fail(PLH_E_UNSUPPORTED, "plh_integrate_sens: sensitivities of a continued solution (Y_init) are not carried across calls");
  if (m->ops->w2) return fail(PLH_E_UNSUPPORTED, "plh_integrate_sens: one wavefront per cell only");
  if (sq->dT && !m->ops->thermal) return fail(PLH_E_UNSUPPORTED, "plh_integrate_sens_out: dT_avg_dtheta needs a thermal model (T_avg does not depend on theta in an isothermal one)");
  if (opts->refine > 0 || opts->n_tdiscon > 0 || opts->n_stop > 0) return fail(PLH_E_UNSUPPORTED, "plh_integrate_sens: not with refine / tdiscon / a stop function");
  for (int r = 0; r < n_runs; r++)
    if ((runs[r].value_kind != PLH_VAL_CONST && runs[r].value_kind != PLH_VAL_REST && runs[r].value_kind != PLH_VAL_HOLD) || runs[r].mode == PLH_MODE_RES || runs[r].mode == PLH_MODE_DSTATE)
      return fail(PLH_E_UNSUPPORTED, "plh_integrate_sens: constant, :rest or :hold inputs in the modes I, V, P, eta_p, dT (a function input depends on theta through the state)");
  return 0;
}
// the kernel instantiation that has the features a call asks for.  The bits are pl::GenFlag of dfn_integrate.h, which the host's translation unit does not include: the
// same values under names of its own (the emulator build, one translation unit, sees both and compares them)
enum Feature { FEAT_STOPS = 1, FEAT_FUNC = 2, FEAT_EXPR = 4, FEAT_REFINE = 8, FEAT_GENROW = 16, FEAT_SENS = 32 };     // stop times / state dump, table inputs, closure inputs, refinement, general control row, sensitivities
#ifdef PL_WAVE_EMU
static_assert(FEAT_STOPS == +GF_STOPS && FEAT_FUNC == +GF_FUNC && FEAT_EXPR == +GF_EXPR && FEAT_REFINE == +GF_REFINE && FEAT_GENROW == +GF_GENROW && FEAT_SENS == +GF_SENS, "GenFlag");
#endif
static int select_features(const plh_opts* opts, const plh_outputs* out, int n_runs, const plh_run* runs, bool need_genW, const SensReq* sq) {
  if (sq) return FEAT_STOPS | FEAT_SENS;
  const int table = FEAT_STOPS | FEAT_FUNC, closure = table | FEAT_EXPR; int f = 0;
  if (opts->n_tdiscon > 0 || opts->n_tstops > 0 || out->Y_all || out->Y_sel || opts->yp_alg_zero != 0) f |= FEAT_STOPS;
  for (int r = 0; r < n_runs; r++) { if (runs[r].value_kind == PLH_VAL_TABLE) f |= table; if (runs[r].value_kind == PLH_VAL_EXPR) f |= closure; }
  if (opts->n_stop > 0) f |= closure;                                            // the stop function runs in the interpreter of the closure instantiations
  if (need_genW) f |= closure | FEAT_GENROW;                                     // closures with derivative programs: the general control row
  if (opts->refine > 0) f |= closure | FEAT_REFINE;
  return f;
}
// ---- the outputs of a call, listed ONCE: every array plh_outputs and a sensitivity request can name.  The staging of the host-pointer kinds, the device block and the
// copy kernels of a blocking host call and the copies back all walk this table: a new output is one row here plus its store in the kernel.  Rows in the
// order of the copies back of the calls that stage array by array; within a class, in the order of the device block of a blocking host call ----
enum OutClass { OC_NPTS, OC_FIXED, OC_POINT, OC_WIDE, OC_SENS };      // n_pts; one entry per cell; [max_pts] doubles per cell; [max_pts] rows of several doubles per cell; sensitivities
struct OutArr {
  void* host; void** dev; size_t elem, rows; OutClass cls;             // the caller's pointer; where the kernel's goes in IntegrateArgs; bytes per entry (per saved point); entries (rows of points)
  bool per_point() const { return cls == OC_POINT || cls == OC_WIDE; } size_t bytes(size_t max_pts) const { return rows * elem * (per_point() ? max_pts : 1); }
};
static std::vector<OutArr> output_table(const plh_model_s* m, size_t n, int n_runs, const plh_outputs* out, size_t n_selt, const SensReq* sq, IntegrateArgs& a) {
  const size_t W8 = sizeof(double), N = m->N; plh_outputs& o = a.out;
  std::vector<OutArr> t = {
      {out->t, (void**)&o.t, W8, n, OC_POINT}, {out->V, (void**)&o.V, W8, n, OC_POINT}, {out->I, (void**)&o.I, W8, n, OC_POINT}, {out->SOC, (void**)&o.SOC, W8, n, OC_POINT},
      {out->T_avg, (void**)&o.T_avg, W8, n, OC_POINT}, {out->n_pts, (void**)&o.n_pts, sizeof(int), n, OC_NPTS},
      {out->Y_all, (void**)&o.Y_all, W8 * N, n, OC_WIDE}, {out->Y_sel, (void**)&o.Y_sel, W8 * n_selt, n, OC_WIDE},
      {out->Y_final, (void**)&o.Y_final, W8 * N, n, OC_FIXED}, {out->YP_final, (void**)&o.YP_final, W8 * N, n, OC_FIXED},
      {out->run_info, (void**)&o.run_info, sizeof(plh_run_info) * n_runs, n, OC_FIXED}, {out->counters, (void**)&o.counters, sizeof(plh_counters), n, OC_FIXED}};
  if (sq) {
    const size_t ns = sq->n_sens;
    t.push_back({sq->dY, (void**)&a.sens.dY, W8 * ns * N, n, OC_SENS}); t.push_back({sq->dV, (void**)&a.sens.dV, W8 * ns * out->max_pts, n, OC_SENS});
    // (the two further channels: their device pointers are not kernel arguments -- stage_sens puts them behind the column list, SensArgs::chan says which)
    t.push_back({sq->dI, (void**)&sq->d_dI, W8 * ns * out->max_pts, n, OC_SENS}); t.push_back({sq->dT, (void**)&sq->d_dT, W8 * ns * out->max_pts, n, OC_SENS});
    t.push_back({sq->stat, (void**)&a.sens.stat, 3 * sizeof(int), n, OC_SENS});
  }
  return t;
}
// ---- the way back of a synchronous host call (see HostRet and the copy kernels above).  A blocking host call (r06b) keeps its outputs in ONE device block, so that they come back in three copies instead of ten (a device-to-host copy command costs 20 ... 30 us
// whatever its size): [longest trajectory] [n_pts] [the fixed-size arrays] [the requested per-point scalar arrays, one [n][max_pts] array behind the other]; Y_all / Y_sel have
// staging blocks of their own.  n_pts is needed on the device whether or not the caller asked for it: it bounds the per-point copies, which bring only the first max(n_pts) of
// the max_pts columns.  The pinned block mirrors the device block (rows packed to the longest trajectory, each array in its worst-case slot), Y_all and Y_sel behind it.
// Items: pieces of the caller's arrays in the order of their arrival.  Every item names the event after which its bytes are in the pinned block; small neighbours share one
// copy kernel, large arrays are cut into pieces of about 4 MB so that the copy into the caller's memory follows the bus piece by piece while later pieces are in flight.
struct RetItem { char* host; size_t rows, width, hpitch, pin_off, elem; int ev; };          // elem != 0: a per-point piece (width and row offsets follow from the longest trajectory)
static void copy_slice(const RetItem& r, const char* pb, unsigned j, unsigned of) {        // thread j of `of` copies its share of an item that has arrived
  if (r.width == 0) return; const char* src = pb + r.pin_off;
  if (r.rows > 1 || r.elem) {
    const size_t qa = r.rows * j / of, qb = r.rows * (j + 1) / of;
    if (r.width == r.hpitch) { if (qb > qa) memcpy(r.host + qa * r.hpitch, src + qa * r.width, (qb - qa) * r.width); }
    else for (size_t q = qa; q < qb; q++) memcpy(r.host + q * r.hpitch, src + q * r.width, r.width);
  } else {
    if (r.width < (256u << 10)) { if (j == 0) memcpy(r.host, src, r.width); return; }
    const size_t a0 = (r.width * j / of) & ~(size_t)63, a1 = j + 1 == of ? r.width : (r.width * (j + 1) / of) & ~(size_t)63;
    memcpy(r.host + a0, src + a0, a1 - a0);
  }
}
static void nap(unsigned& spins) {      // a waiting team thread spins for about a millisecond, then naps in 50 us steps
#if defined(__x86_64__) || defined(__i386__)
  if (spins++ < 20000) __builtin_ia32_pause(); else std::this_thread::sleep_for(std::chrono::microseconds(50));
#else
  if (spins++ < 20000) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(50));
#endif
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct CopyTeam {      // the threads that copy into the caller's memory: joined when the scope ends, whichever way it ends (an exit that has not joined them tells them to give up first)
  std::vector<std::thread> th; std::atomic<int> fired{0}; std::atomic<bool> listed{false}, give_up{false};      // events [0, fired) have been waited for; listed: the items are final
  void join() { for (auto& t : th) t.join(); th.clear(); }
  ~CopyTeam() { give_up.store(true); join(); }
};
struct HostReturn {
  plh_model_s* m; Stage& s; IntegrateArgs& a; std::vector<OutArr>& tab; const plh_outputs* out; size_t n, mp, np; double t_entry;      // (mp: max_pts, np = n mp)
  std::vector<size_t> off;                                            // per table row: its place in the pinned block (n_pts, fixed-size and per-point scalar arrays: in the device block too)
  size_t hdr = 0, npts = 0, fixed1 = 0, worst = 0, CH = 0; char *base = nullptr, *pb = nullptr, *pbd = nullptr;      // (hdr: the longest trajectory, worked out on the device; CH: the piece size); the device block, the pinned block as the host and as the device see it
  std::vector<RetItem> items; std::vector<HostRet> rets;              // (rets, for the prefault: the whole arrays)
  int n_ev = 0, ev_n = 0; hipError_t ev_err = hipSuccess; double tr0 = 0, tr1 = 0;
  void chk(hipError_t e) { if (e != hipSuccess && ev_err == hipSuccess) ev_err = e; }
  int record() { std::vector<hipEvent_t>& evs = s.cx->ret_ev;         // an event behind what has been queued so far
    if ((size_t)n_ev == evs.size()) { hipEvent_t e; chk(hipEventCreate(&e)); if (ev_err != hipSuccess) return n_ev; evs.push_back(e); }
    chk(hipEventRecord(evs[n_ev], s.st)); return n_ev++;
  }
  void layout() {                                                     // the device block and the kernel's pointers into it
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    bool dev_npts = false; for (const OutArr& e : tab) dev_npts = dev_npts || (e.host && (e.cls == OC_NPTS || (e.per_point() && np > 0)));
    off.assign(tab.size(), 0); size_t o = 256; npts = o; if (dev_npts) o += up(n * sizeof(int));
    for (size_t k = 0; k < tab.size(); k++) if (tab[k].cls == OC_FIXED && tab[k].host) { off[k] = o; o += up(tab[k].bytes(mp)); }
    fixed1 = o; for (size_t k = 0; k < tab.size(); k++) if (tab[k].cls == OC_POINT && tab[k].host && np > 0) { off[k] = o; o += tab[k].bytes(mp); }
    base = (char*)s.dev_block(o + 256);
    for (size_t k = 0; k < tab.size(); k++) { const OutArr& e = tab[k];
      if (e.cls == OC_NPTS) { off[k] = npts; *e.dev = base && dev_npts ? base + npts : nullptr; }
      else if (e.cls == OC_FIXED) *e.dev = base && e.host ? base + off[k] : nullptr;
      else if (e.cls == OC_POINT) *e.dev = base && e.host && np > 0 ? base + off[k] : nullptr;
      else { *e.dev = s.buf((char*)e.host, e.bytes(mp), false); o = up(o); off[k] = o; o += e.host ? e.bytes(mp) : 0; }
    }
    worst = o + 256;
  }
  int queue() {      // behind the integrate kernel, before it ends: the longest trajectory, then every array into the pinned block, an event behind each piece
    CH = std::max<size_t>(4u << 20, worst / 48);
    pb = (char*)m->pinned(worst);
    if (!pb) return fail(PLH_E_HIP, "pinned staging block of the host return path");
    pbd = pb;
#ifndef PL_WAVE_EMU
    { void* dp = nullptr; if (hipHostGetDevicePointer(&dp, pb, 0) == hipSuccess && dp) pbd = (char*)dp; }
#endif
    if (a.out.n_pts) launch_max_npts(s.st, a.out.n_pts, (int)n, (int)mp, (int*)(base + hdr), (int*)(pbd + hdr), (int*)(pbd + npts));
    ev_n = record();                                                  // the kernel is done, n_pts and the longest trajectory are here
    queue_fixed(); queue_per_point(); return 0;
  }
  void queue_fixed() {                                                // the fixed-size arrays, in the order of the device block
    size_t run0 = 0, run1 = 0, first = items.size();                  // the pending run of small arrays [run0, run1) of the block, its items from `first`
    auto flush = [&] {
      if (run1 > run0) { launch_copy_words(s.st, base + run0, pbd + run0, run1 - run0); const int e = record(); for (size_t q = first; q < items.size(); q++) items[q].ev = e; }
      run0 = run1 = 0; first = items.size();
    };
    for (size_t k = 0; k < tab.size(); k++) {
      const OutArr& f = tab[k]; const size_t bytes = f.bytes(mp), o = off[k];
      if (f.cls != OC_FIXED || !f.host || !*f.dev || !bytes) continue;
      rets.push_back({(char*)f.host, (const char*)*f.dev, 1, bytes, bytes, 0});
      if (bytes > CH) {                                               // a large array: its own kernels, piece by piece
        flush();
        for (size_t q = 0; q < bytes; q += CH) {
          const size_t b = std::min(CH, bytes - q);
          launch_copy_words(s.st, (const char*)*f.dev + q, pbd + o + q, b);
          items.push_back({(char*)f.host + q, 1, b, b, o + q, 0, record()});
        }
        first = items.size();
        continue;
      }
      if (run1 > run0 && o + bytes - run0 > CH) flush();
      if (run1 == run0) run0 = o;
      run1 = o + bytes;
      items.push_back({(char*)f.host, 1, bytes, bytes, o, 0, -1});
    }
    flush();
  }
  void queue_per_point() {                                            // the per-point arrays, scalar ones first: row pieces sized by the worst case (max_pts columns)
    for (OutClass cls : {OC_POINT, OC_WIDE}) for (size_t k = 0; k < tab.size(); k++) {
      const OutArr& q = tab[k];
      if (q.cls != cls || !q.host || !*q.dev || !mp || !a.out.n_pts) continue;
      const size_t pitch = mp * q.elem, rows_per = std::max<size_t>(std::max<size_t>(1, CH / pitch), (n + 63) / 64);          // (at most 64 pieces per array)
      rets.push_back({(char*)q.host, (const char*)*q.dev, n, pitch, pitch, 0});
      for (size_t q0 = 0; q0 < n; q0 += rows_per) {
        const size_t nr = std::min(rows_per, n - q0);
        launch_pack_rows(s.st, (const char*)*q.dev, pitch, q.elem / 8, (const int*)(base + hdr), q0, nr, mp * q.elem / 8, pbd + off[k]);
        items.push_back({(char*)q.host + q0 * pitch, nr, q0, pitch, off[k], q.elem, record()});          // (pin_off: the slot, and width: the first row, until the longest trajectory is known)
      }
    }
  }
  void prefault() { tr0 = now_ms(); if (ev_err == hipSuccess) ::prefault(rets, 4096); tr1 = now_ms(); }      // first touch of the caller's pages, while the kernel runs
  // The team that copies into the caller's memory is started while the kernel still runs (starting eight threads takes 0.15 ms): this thread waits on the events and
  // publishes how many have fired, thread j copies slice j of every item
  int collect() {
    static const bool trace = getenv("PLH_HOST_TRACE") != nullptr; std::vector<hipEvent_t>& evs = s.cx->ret_ev;     // trace: timing of the phases on stderr (tools/gpu: where a blocking call's time goes)
    unsigned nt = (unsigned)std::min<size_t>(8, worst / (512u << 10));
#ifdef PL_WAVE_EMU
    nt = 0;
#endif
    CopyTeam team;
    for (unsigned j = 0; j < nt; j++) team.th.emplace_back([this, &team, j, nt] {
      for (unsigned spins = 0; !team.listed.load(std::memory_order_acquire); nap(spins)) if (team.give_up.load(std::memory_order_relaxed)) return;
      for (const RetItem& it : items) {
        for (unsigned spins = 0; team.fired.load(std::memory_order_acquire) <= it.ev; nap(spins)) if (team.give_up.load(std::memory_order_relaxed)) return;
        copy_slice(it, pb, j, nt);
      }
    });
    if (ev_err == hipSuccess) chk(hipEventSynchronize(evs[ev_n]));
    chk(hipGetLastError());
    HIPCHK(ev_err);
    const double tr2 = now_ms();
    // the longest trajectory bounds the per-point pieces: the first max(n_pts) of the max_pts columns (entries beyond n_pts[cell] were never defined)
    size_t maxn = 0, total = fixed1;
    if (a.out.n_pts) {
      maxn = (size_t)std::max(0, *(const int*)(pb + hdr));
      if (out->n_pts) memcpy(out->n_pts, pb + npts, n * sizeof(int));
    }
    for (RetItem& it : items) if (it.elem) { const size_t row0 = it.width, w = maxn * it.elem; it.width = w; it.pin_off += row0 * w; total += it.rows * w; }
    team.listed.store(true, std::memory_order_release);
    const double tr3 = now_ms();
    double tr_wait = 0; size_t done = 0;
    for (int e = 0; e < n_ev; e++) {
      const double tw = trace ? now_ms() : 0;
      if (ev_err == hipSuccess) chk(hipEventSynchronize(evs[e]));
      if (trace) tr_wait += now_ms() - tw;
      team.fired.store(e + 1, std::memory_order_release);
      if (nt == 0) for (; done < items.size() && items[done].ev <= e; done++) copy_slice(items[done], pb, 0, 1);
    }
    team.join();
    HIPCHK(ev_err);
    if (trace) { float kms = 0; hipEventElapsedTime(&kms, s.cx->ev0, s.cx->ev1);
      fprintf(stderr, "[plh host call] kernel %.3f ms | staging + launch + fixed-size copies queued %.3f, prefault %.3f, team start + wait for kernel + n_pts %.3f, items finalised %.3f (%.1f MB in all), copy-out %.3f (of which waiting on D2H %.3f) ms\n",
              kms, tr0 - t_entry, tr1 - tr0, tr2 - tr1, tr3 - tr2, total / 1048576.0, now_ms() - tr3, tr_wait); }
    return 0;
  }
};
static std::vector<double> sorted_times(const double* t, int cnt) { std::vector<double> v(t, t + (cnt > 0 ? cnt : 0)); std::sort(v.begin(), v.end()); return v; }
// The protocol is always host memory, and so are its tables, per-cell values and the stop function's program: staged, the device copy of the descriptors patched.
// compiled: the closures run as the attached library's kernels.  *plain: no staged array behind the descriptors (the device copy may be remembered)
static int stage_protocol(Stage& s, int n, int n_runs, const plh_run* runs, const plh_opts* opts, bool compiled, IntegrateArgs& a, bool* plain) {
  std::vector<plh_run> hruns(runs, runs + n_runs);
  { int cid = 0; for (int r = 0; r < n_runs; r++) hruns[r].closure_id = (compiled && hruns[r].value_kind == PLH_VAL_EXPR) ? cid++ : -1; }
  for (int r = 0; r < n_runs; r++) {
    if (hruns[r].value_kind == PLH_VAL_TABLE || hruns[r].value_kind == PLH_VAL_EXPR) {
      const bool der = hruns[r].value_kind == PLH_VAL_EXPR && runs[r].n_dcol > 0;
      const int len = der ? runs[r].dofs[runs[r].n_dcol] : runs[r].n_tab;
      hruns[r].tab_t = s.in_host(runs[r].tab_t, len); hruns[r].tab_v = s.in_host(runs[r].tab_v, len);
      if (der) { hruns[r].dcol = s.in_host(runs[r].dcol, runs[r].n_dcol); hruns[r].dofs = s.in_host(runs[r].dofs, runs[r].n_dcol + 1); }
      else { hruns[r].n_dcol = 0; hruns[r].dcol = nullptr; hruns[r].dofs = nullptr; }
    } else { hruns[r].n_tab = 0; hruns[r].tab_t = nullptr; hruns[r].tab_v = nullptr; hruns[r].n_dcol = 0; hruns[r].dcol = nullptr; hruns[r].dofs = nullptr; }
    if (runs[r].value_cell) hruns[r].value_cell = s.in_host(runs[r].value_cell, n);       // per-cell protocol values: host arrays like the protocol
    if (runs[r].tf_cell) hruns[r].tf_cell = s.in_host(runs[r].tf_cell, n);
  }
  a.opts.stop_ops = nullptr; a.opts.stop_args = nullptr;
  if (opts->n_stop > 0) { a.opts.stop_ops = s.in_host(opts->stop_ops, opts->n_stop); a.opts.stop_args = s.in_host(opts->stop_args, opts->n_stop); }
  CHECK_STAGE(s);
  *plain = opts->n_stop == 0;
  for (int r = 0; r < n_runs; r++) *plain = *plain && !hruns[r].tab_t && !hruns[r].value_cell && !hruns[r].tf_cell;
  return s.cx->runs.get(s.st, hruns, &a.runs, *plain);
}
// the workspaces of a sensitivity request, the perturbed theta rows, and outputs that read as NaN (all-ones bytes) for cells that never get as far as writing them
static int stage_sens(const plh_model_s* m, Stage& s, size_t n, size_t max_pts, const SensReq* sq, IntegrateArgs& a) {
  const size_t ns = sq->n_sens, NPAD = m->N + (m->N & 1);
  // the column list, and behind it the pointers of the further channels (dfn_cell.h, sens_chan_offset)
  std::vector<int> cols(pl::sens_chan_offset((int)ns) + 2 * sizeof(double*) / sizeof(int), 0);
  std::copy(sq->cols, sq->cols + ns, cols.begin());
  double* const chp[2] = {sq->d_dI, sq->d_dT};
  memcpy(cols.data() + pl::sens_chan_offset((int)ns), chp, sizeof chp);
  a.sens.n_sens = (int)ns; a.sens.cols = s.in_host(cols.data(), cols.size());
  a.sens.chan = (sq->d_dI ? pl::SENS_CH_I : 0) | (sq->d_dT ? pl::SENS_CH_T : 0);
  double* tp = (double*)s.dev_block(n * ns * m->P * sizeof(double)); a.sens.hist = (double*)s.dev_block(n * ns * 6 * NPAD * sizeof(double));
  a.sens.cbak = (double*)s.dev_block(n * pl::SENS_CBAK * sizeof(double)); a.sens.aux = (double*)s.dev_block(n * ns * 4 * sizeof(double));
  a.sens.fsave_stride = m->ops->fsave_doubles;
  a.sens.fsave = (double*)s.dev_block(n * a.sens.fsave_stride * sizeof(double));
  CHECK_STAGE(s);
  a.sens.theta_pert = tp; launch_theta_pert(s.st, a.theta, a.sens.cols, (int)n, (int)ns, m->P, tp);
  if (a.sens.dY) HIPCHK(hipMemsetAsync(a.sens.dY, 0xff, n * ns * m->N * sizeof(double), s.st));
  for (double* ch : {a.sens.dV, sq->d_dI, sq->d_dT}) if (ch) HIPCHK(hipMemsetAsync(ch, 0xff, n * ns * max_pts * sizeof(double), s.st));
  if (a.sens.stat) HIPCHK(hipMemsetAsync(a.sens.stat, 0, 3 * n * sizeof(int), s.st));
  if (a.sens.aux) HIPCHK(hipMemsetAsync(a.sens.aux, 0, n * ns * 4 * sizeof(double), s.st));
  return 0;
}
// No staging block goes back to the cache under a running kernel or copy: declared after the Stage, so destroyed before it, this waits for the stream on every way out --
// the error exits included -- except the successful returns, which disarm it: there the stream is idle (PLH_HOST; staged protocol arrays) or the blocks are deferred (PLH_HOST_ASYNC)
struct SyncFirst { hipStream_t st; bool armed; ~SyncFirst() { if (armed) hipStreamSynchronize(st); } };
// validate -> workspaces -> stage inputs -> outputs -> sensitivities -> launch -> return
static int integrate_impl(plh_model_t m, int n, const double* theta, const double* SOC0, const double* Y_init, const double* t_init, int n_runs,
                          const plh_run* runs, const plh_opts* opts, const plh_outputs* out, int kind, void* stream, const SensReq* sq) {
  const double t_entry = now_ms();
  CHECK_MODEL(m);
  if (kind != PLH_HOST && kind != PLH_DEVICE && kind != PLH_HOST_ASYNC) return fail(PLH_E_ARG, "bad ptr_kind");
  if (n <= 0 || !theta || !SOC0 || n_runs <= 0 || !runs || !opts || !out || !out->run_info) return fail(PLH_E_ARG, "bad argument");
  std::vector<int> sel_map; if (int rc = check_runs(m, n, n_runs, runs, Y_init)) return rc;
  if (int rc = check_outputs(m, out, &sel_map)) return rc;
  if (t_init && !Y_init) return fail(PLH_E_ARG, "t_init without Y_init");        // (Y_init without t_init: a new solution from the caller's states -- initial_states)
  if (int rc = check_opts(m, opts)) return rc;
  if (sq) { if (int rc = check_sens(m, sq, n_runs, runs, opts, Y_init)) return rc; }
  if (!out->Y_sel) sel_map.clear();                                    // (ranges without Y_sel: checked like any others, nothing selected)
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream); StreamCtx& cx = *s.cx;
  SyncFirst sync_first{s.st, true};
  bool need_genW = false;                                            // workspaces
  for (int r = 0; r < n_runs; r++) need_genW = need_genW || (runs[r].value_kind == PLH_VAL_EXPR && runs[r].n_dcol > 0) || runs[r].mode == PLH_MODE_DSTATE;
  IntegrateArgs a;
  a.tb = m->d_tb; a.n_cells = n; a.n_runs = n_runs; a.opts = *opts;
  HIPCHK(cx.scratch.reserve(cx.st, (size_t)n * 2 * m->N * sizeof(double)));
  if (need_genW) HIPCHK(cx.genW.reserve(cx.st, (size_t)n * m->N * sizeof(double)));
  a.scratch = (double*)cx.scratch.d; a.genW = need_genW ? (double*)cx.genW.d : nullptr;
  // inputs: the caller's arrays, then what is always host memory -- time lists, selection map, protocol -- as device copies kept per stream
  a.theta = s.in(theta, (size_t)n * m->P); a.SOC0 = s.in(SOC0, n);
  a.Y_init = s.in(Y_init, (size_t)n * m->N); a.t_init = s.in(t_init, n);
  if (int rc = cx.tdiscon.get(cx.st, sorted_times(opts->tdiscon, opts->n_tdiscon), &a.opts.tdiscon)) return rc;
  if (int rc = cx.tstops.get(cx.st, sorted_times(opts->tstops, opts->n_tstops), &a.opts.tstops)) return rc;
  if (int rc = cx.sel.get(cx.st, sel_map, &a.sel_map, true, m->N)) return rc;
  a.sel_tot = (int)sel_map.size();                                    // entries per saved row of Y_sel (<= N: the ranges do not overlap)
  // compiled closures: the attached library's kernels when this protocol's programs are the ones it was built from (and nothing asks for the refinement instantiation)
  const bool compiled = m->cl_ops && opts->refine == 0 && !sq && plh_closure_digest(n_runs, runs) == m->cl_digest && m->cl_digest != 0;
  bool plain = false; if (int rc = stage_protocol(s, n, n_runs, runs, opts, compiled, a, &plain)) return rc;
  // outputs: one device block for a blocking host call (HostReturn), one staging block per array for the other host kind, the caller's own pointers for PLH_DEVICE
  a.out = *out; a.out.n_sel = 0; a.out.sel = nullptr;                         // (host memory: the kernels read a.sel_map / a.sel_tot)
  a.sens = pl::SensArgs{};
  std::vector<OutArr> tab = output_table(m, n, n_runs, out, sel_map.size(), sq, a);
  const bool host_ret = kind == PLH_HOST && !sq; HostReturn hr{m, s, a, tab, out, (size_t)n, (size_t)out->max_pts, (size_t)n * out->max_pts, t_entry};
  if (host_ret) hr.layout();
  else for (const OutArr& e : tab) *e.dev = s.buf((char*)e.host, e.bytes(out->max_pts), false);
  if (sq) { if (int rc = stage_sens(m, s, n, out->max_pts, sq, a)) return rc; }
  CHECK_STAGE(s);                                                     // a failed staging allocation must never reach the kernel as a NULL ("not requested") output
  hipEventRecord(cx.ev0, s.st);                                       // launch
  const int features = select_features(opts, out, n_runs, runs, need_genW, sq);
  m->last_compiled = compiled && (features & FEAT_EXPR);
  (m->last_compiled ? m->cl_ops : m->ops)->integrate(s.st, a, features);
  hipEventRecord(cx.ev1, s.st); cx.timed = true; m->last = &cx;
  if (host_ret) {                                                     // return
    if (int rc = hr.queue()) return rc;
    hr.prefault();
    if (int rc = hr.collect()) return rc;
    CHECK_STAGE(s);
  } else {
    FINISH(s);
    if ((!plain || sq) && kind != PLH_HOST) HIPCHK(hipStreamSynchronize(s.st));   // staged tables / per-cell values / sensitivity workspaces are released below: the kernel must be done with them
    for (const OutArr& e : tab) s.back((char*)e.host, (const char*)*e.dev, e.bytes(out->max_pts));
    CHECK_STAGE(s);
    if (kind == PLH_HOST_ASYNC) s.defer();
  }
  sync_first.armed = false;
  return 0;
}

int plh_integrate(plh_model_t m, int n, const double* theta, const double* SOC0, const double* Y_init, const double* t_init, int n_runs,
                  const plh_run* runs, const plh_opts* opts, const plh_outputs* out, int kind, void* stream) {
  return integrate_impl(m, n, theta, SOC0, Y_init, t_init, n_runs, runs, opts, out, kind, stream, nullptr);
}

int plh_integrate_sens(plh_model_t m, int n, const double* theta, const double* SOC0, int n_runs, const plh_run* runs, const plh_opts* opts, const plh_outputs* out,
                       int n_sens, const int* sens_cols, double* dY_dtheta, double* dV_dtheta, int* sens_stat, int kind, void* stream) {
  if (kind != PLH_HOST && kind != PLH_DEVICE) return fail(PLH_E_ARG, "plh_integrate_sens: ptr_kind must be PLH_HOST or PLH_DEVICE");
  const plh_sens_outputs so = {dY_dtheta, dV_dtheta, nullptr, nullptr, sens_stat};
  return plh_integrate_sens_out(m, n, theta, SOC0, n_runs, runs, opts, out, n_sens, sens_cols, &so, kind, stream);
}

int plh_integrate_sens_out(plh_model_t m, int n, const double* theta, const double* SOC0, int n_runs, const plh_run* runs, const plh_opts* opts, const plh_outputs* out,
                           int n_sens, const int* sens_cols, const plh_sens_outputs* so, int kind, void* stream) {
  if (kind != PLH_HOST && kind != PLH_DEVICE) return fail(PLH_E_ARG, "plh_integrate_sens: ptr_kind must be PLH_HOST or PLH_DEVICE");
  if (!so) return fail(PLH_E_ARG, "plh_integrate_sens_out: null plh_sens_outputs");
  const SensReq sq = {n_sens, sens_cols, so->dY_dtheta, so->dV_dtheta, so->sens_stat, so->dI_dtheta, so->dT_avg_dtheta, nullptr, nullptr};
  return integrate_impl(m, n, theta, SOC0, nullptr, nullptr, n_runs, runs, opts, out, kind, stream, &sq);
}

// ---- plh_resample: one per-point field of an ensemble on a time grid shared by all cells (kernels and algorithm: plh_resample.h) ----
// The slopes need a workspace of max_pts x width doubles per cell -- a second copy of the field.  It is kept per stream and bounded: the cells are processed in chunks
// (successive launches on the stream) of at most PLH_RESAMPLE_WS_BYTES of workspace (environment, read at every call; default 256 MiB; never less than one cell).
// (shared with plh_lsq / plh_lsq_multi, whose columns are every channel's curve and the rows of its sensitivities: cells per chunk -- `blocks_per_cell` of the widest launch bounds the grid -- and the chunk's workspace)
static int resample_work(StreamCtx& cx, int n, int n_runs, int max_pts, int n_q, int width, size_t blocks_per_cell, size_t* chunk_out, plrs::Work* w) {
  size_t budget = (size_t)256 << 20;
  if (const char* e = getenv("PLH_RESAMPLE_WS_BYTES")) { const long long v = atoll(e); if (v > 0) budget = (size_t)v; }
  const size_t per = plrs::work_bytes_per_cell(n_runs, max_pts, n_q, width);
  size_t chunk = std::min<size_t>((size_t)n, std::max<size_t>(1, budget / per));
  chunk = std::max<size_t>(1, std::min(chunk, std::min<size_t>(0x7fffffffu / blocks_per_cell, (size_t)0x7fffffffu * plrs::TILE / (size_t)n_q)));      // (grid sizes of the launches)
  HIPCHK(cx.resample.reserve(cx.st, chunk * per));
  char* b = (char*)cx.resample.d;
  w->fac = (double*)b; b += chunk * max_pts * 2 * sizeof(double);
  w->loc_t = (double*)b; b += chunk * n_q * sizeof(double);
  w->slope = (double*)b; b += chunk * max_pts * width * sizeof(double);
  w->ok = (int*)b; b += chunk * sizeof(int);
  w->run0 = (int*)b; b += chunk * n_runs * sizeof(int);
  w->loc_i = (int*)b;
  *chunk_out = chunk;
  return 0;
}
int plh_resample(plh_model_t m, int n, int n_runs, int max_pts, const double* t, const int* n_pts, const plh_run_info* run_info, int width, const double* src,
                 int n_q, const double* tq, int extrapolate, double* dst, int* status, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind);
  if (n < 1 || n_runs < 1 || max_pts < 1 || width < 1 || n_q < 1) return fail(PLH_E_ARG, "plh_resample: n_cells, n_runs, max_pts, width and n_q must be >= 1");
  if (!t || !n_pts || !run_info || !src || !tq || !dst) return fail(PLH_E_ARG, "plh_resample: null array (only status may be NULL)");
  if (extrapolate != 0 && extrapolate != 1) return fail(PLH_E_ARG, "plh_resample: extrapolate must be 0 or 1");
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  StreamCtx& cx = *s.cx;
  const size_t pts = (size_t)n * max_pts, n_dst = (size_t)n * n_q * width;
  const double* d_t = s.in(t, pts); const int* d_np = s.in(n_pts, (size_t)n); const plh_run_info* d_ri = s.in(run_info, (size_t)n * n_runs);
  const double* d_src = s.in(src, pts * width);
  double* d_dst = s.buf(dst, n_dst, false); int* d_status = s.buf(status, (size_t)n, false);
  CHECK_STAGE(s);
  const double* d_tq = nullptr;
  if (int rc = cx.resample_tq.get(cx.st, std::vector<double>(tq, tq + n_q), &d_tq)) return rc;
  size_t chunk = 0; plrs::Work w;
  if (int rc = resample_work(cx, n, n_runs, max_pts, n_q, width, ((size_t)width + plrs::TILE - 1) / plrs::TILE, &chunk, &w)) return rc;
  for (size_t c0 = 0; c0 < (size_t)n; c0 += chunk) {
    plrs::Args a;
    a.cell0 = (int)c0; a.n_chunk = (int)std::min(chunk, (size_t)n - c0);
    a.n_runs = n_runs; a.max_pts = max_pts; a.width = width; a.n_q = n_q; a.extrapolate = extrapolate;
    a.t = d_t; a.n_pts = d_np; a.run_info = d_ri; a.src = d_src; a.tq = d_tq; a.dst = d_dst; a.status = d_status; a.w = w;
    plrs::launch_chunk(s.st, a);
  }
  FINISH(s);
  s.back(dst, d_dst, n_dst); s.back(status, d_status, (size_t)n); CHECK_STAGE(s);
  return 0;
}

// ---- plh_lsq / plh_lsq_multi: misfit of the measured curves against data, gradient and Gauss-Newton matrix per cell (kernels: plh_lsq.h; the slopes of every channel's curve
// and of the rows of its sensitivities share plh_resample's workspace and its chunking).  plh_lsq is the one-channel call: one kernel, the same bits ----
int plh_lsq(plh_model_t m, int n, int n_runs, int max_pts, const double* t, const int* n_pts, const plh_run_info* run_info, const double* V, int n_sens,
            const double* dV_dtheta, int n_q, const double* tq, const double* y, const double* w, int per_cell, int extrapolate,
            double* cost, double* grad, double* JtJ, double* resid, int* status, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind);
  if (n < 1 || n_runs < 1 || max_pts < 1 || n_q < 1) return fail(PLH_E_ARG, "plh_lsq: n_cells, n_runs, max_pts and n_q must be >= 1");
  if (n_sens < 0 || n_sens > PLH_LSQ_MAX_SENS) return fail(PLH_E_ARG, "plh_lsq: n_sens must be 0 .. PLH_LSQ_MAX_SENS (8)");
  if ((per_cell != 0 && per_cell != 1) || (extrapolate != 0 && extrapolate != 1)) return fail(PLH_E_ARG, "plh_lsq: per_cell and extrapolate must be 0 or 1");
  if (!t || !n_pts || !run_info || !V || !tq || !y || !cost) return fail(PLH_E_ARG, "plh_lsq: null array (only w, resid and status may be NULL)");
  if ((n_sens > 0) != (dV_dtheta != nullptr) || (n_sens > 0) != (grad != nullptr) || (n_sens > 0) != (JtJ != nullptr))
    return fail(PLH_E_ARG, "plh_lsq: dV_dtheta, grad and JtJ are given with n_sens > 0 and NULL with n_sens == 0");
  const plh_lsq_channel ch = {V, dV_dtheta, y, w, resid};
  return plh_lsq_multi(m, n, n_runs, max_pts, t, n_pts, run_info, 1, &ch, n_sens, n_q, tq, per_cell, extrapolate, cost, grad, JtJ, status, kind, stream);
}

int plh_lsq_multi(plh_model_t m, int n, int n_runs, int max_pts, const double* t, const int* n_pts, const plh_run_info* run_info, int n_ch, const plh_lsq_channel* ch,
                  int n_sens, int n_q, const double* tq, int per_cell, int extrapolate, double* cost, double* grad, double* JtJ, int* status, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind);
  if (n < 1 || n_runs < 1 || max_pts < 1 || n_q < 1) return fail(PLH_E_ARG, "plh_lsq_multi: n_cells, n_runs, max_pts and n_q must be >= 1");
  if (n_sens < 0 || n_sens > PLH_LSQ_MAX_SENS) return fail(PLH_E_ARG, "plh_lsq_multi: n_sens must be 0 .. PLH_LSQ_MAX_SENS (8)");
  if (n_ch < 1 || n_ch > PLH_LSQ_MAX_CHANNELS || !ch) return fail(PLH_E_ARG, "plh_lsq_multi: n_ch must be 1 .. PLH_LSQ_MAX_CHANNELS (3), with the channel array");
  if ((per_cell != 0 && per_cell != 1) || (extrapolate != 0 && extrapolate != 1)) return fail(PLH_E_ARG, "plh_lsq_multi: per_cell and extrapolate must be 0 or 1");
  if (!t || !n_pts || !run_info || !tq || !cost) return fail(PLH_E_ARG, "plh_lsq_multi: null array (only w, resid and status may be NULL)");
  if ((n_sens > 0) != (grad != nullptr) || (n_sens > 0) != (JtJ != nullptr)) return fail(PLH_E_ARG, "plh_lsq_multi: grad and JtJ are given with n_sens > 0 and NULL with n_sens == 0");
  for (int c = 0; c < n_ch; c++) {
    if (!ch[c].curve || !ch[c].y) return fail(PLH_E_ARG, "plh_lsq_multi: a channel without curve or y");
    if ((n_sens > 0) != (ch[c].dcurve != nullptr)) return fail(PLH_E_ARG, "plh_lsq_multi: a channel's dcurve is given with n_sens > 0 and NULL with n_sens == 0");
  }
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  StreamCtx& cx = *s.cx;
  const size_t pts = (size_t)n * max_pts, n_data = per_cell ? (size_t)n * n_q : (size_t)n_q, ns = (size_t)n_sens;
  const int width = n_ch * (1 + n_sens);
  pllsq::Args A;
  plrs::Args& a = A.rs;
  a.t = s.in(t, pts); a.n_pts = s.in(n_pts, (size_t)n); a.run_info = s.in(run_info, (size_t)n * n_runs);
  for (int c = 0; c < PLH_LSQ_MAX_CHANNELS; c++) {
    A.ch[c] = plh_lsq_channel{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (c < n_ch) A.ch[c] = plh_lsq_channel{s.in(ch[c].curve, pts), s.in(ch[c].dcurve, pts * ns), s.in(ch[c].y, n_data), s.in(ch[c].w, n_data), s.buf(ch[c].resid, (size_t)n * n_q, false)};
  }
  A.cost = s.buf(cost, (size_t)n, false); A.grad = s.buf(grad, n * ns, false); A.JtJ = s.buf(JtJ, n * ns * ns, false);
  a.status = s.buf(status, (size_t)n, false);
  CHECK_STAGE(s);
  if (int rc = cx.resample_tq.get(cx.st, std::vector<double>(tq, tq + n_q), &a.tq)) return rc;
  size_t chunk = 0;
  if (int rc = resample_work(cx, n, n_runs, max_pts, n_q, width, 1, &chunk, &a.w)) return rc;
  a.n_runs = n_runs; a.max_pts = max_pts; a.width = width; a.n_q = n_q; a.extrapolate = extrapolate; a.src = nullptr; a.dst = nullptr;
  A.n_sens = n_sens; A.per_cell = per_cell; A.n_ch = n_ch;
  for (size_t c0 = 0; c0 < (size_t)n; c0 += chunk) {
    a.cell0 = (int)c0; a.n_chunk = (int)std::min(chunk, (size_t)n - c0);
    pllsq::launch_chunk(s.st, A);
  }
  FINISH(s);
  s.back(cost, A.cost, (size_t)n); s.back(grad, A.grad, n * ns); s.back(JtJ, A.JtJ, n * ns * ns);
  for (int c = 0; c < n_ch; c++) s.back(ch[c].resid, A.ch[c].resid, (size_t)n * n_q);
  s.back(status, a.status, (size_t)n);
  CHECK_STAGE(s);
  return 0;
}

// ---- plh_predict: every channel's curve and sensitivities at the query times, and the variance of the curve under the covariance of the keys (kernel: plh_predict.h; the
// slopes share plh_resample's workspace and its chunking like plh_lsq_multi's; the offsets' device copy is the one plh_lsq_group remembers per stream) ----
static int check_groups(const char* who, int n, int n_groups, const int* group_off);
int plh_predict(plh_model_t m, int n, int n_runs, int max_pts, const double* t, const int* n_pts, const plh_run_info* run_info, int n_ch, const plh_predict_channel* ch,
                int n_sens, int n_q, const double* tq, int extrapolate, const double* cov, int n_groups, const int* group_off, int* status, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind);
  if (n < 1 || n_runs < 1 || max_pts < 1 || n_q < 1) return fail(PLH_E_ARG, "plh_predict: n_cells, n_runs, max_pts and n_q must be >= 1");
  if (n_sens < 1 || n_sens > PLH_LSQ_MAX_SENS) return fail(PLH_E_ARG, "plh_predict: n_sens must be 1 .. PLH_LSQ_MAX_SENS (8); without sensitivities use plh_resample");
  if (n_ch < 1 || n_ch > PLH_LSQ_MAX_CHANNELS || !ch) return fail(PLH_E_ARG, "plh_predict: n_ch must be 1 .. PLH_LSQ_MAX_CHANNELS (3), with the channel array");
  if (extrapolate != 0 && extrapolate != 1) return fail(PLH_E_ARG, "plh_predict: extrapolate must be 0 or 1");
  if (!t || !n_pts || !run_info || !tq) return fail(PLH_E_ARG, "plh_predict: null array (only cov, group_off and status may be NULL)");
  for (int c = 0; c < n_ch; c++) {
    if (!ch[c].curve || !ch[c].dcurve) return fail(PLH_E_ARG, "plh_predict: a channel without curve or dcurve");
    if (!ch[c].pred && !ch[c].dpred && !ch[c].var) return fail(PLH_E_ARG, "plh_predict: a channel without any output");
    if (ch[c].var && !cov) return fail(PLH_E_ARG, "plh_predict: a var without cov");
  }
  if (group_off) { if (int rc = check_groups("plh_predict", n, n_groups, group_off)) return rc; }
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  StreamCtx& cx = *s.cx;
  const size_t pts = (size_t)n * max_pts, nq = (size_t)n * n_q, ns = (size_t)n_sens, n_prob = group_off ? (size_t)n_groups : (size_t)n;
  const int width = n_ch * (1 + n_sens);
  plpr::Args A;
  plrs::Args& a = A.rs;
  a.t = s.in(t, pts); a.n_pts = s.in(n_pts, (size_t)n); a.run_info = s.in(run_info, (size_t)n * n_runs);
  for (int c = 0; c < PLH_LSQ_MAX_CHANNELS; c++) {
    A.ch[c] = plh_predict_channel{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (c < n_ch) A.ch[c] = plh_predict_channel{s.in(ch[c].curve, pts), s.in(ch[c].dcurve, pts * ns), s.buf(ch[c].pred, nq, false), s.buf(ch[c].dpred, nq * ns, false), s.buf(ch[c].var, nq, false)};
  }
  A.cov = s.in(cov, n_prob * ns * ns);
  a.status = s.buf(status, (size_t)n, false);
  CHECK_STAGE(s);
  if (int rc = cx.resample_tq.get(cx.st, std::vector<double>(tq, tq + n_q), &a.tq)) return rc;
  A.group_off = nullptr; A.n_groups = group_off ? n_groups : 0;
  if (group_off) { if (int rc = cx.group_off.get(cx.st, std::vector<int>(group_off, group_off + n_groups + 1), &A.group_off)) return rc; }
  size_t chunk = 0;
  if (int rc = resample_work(cx, n, n_runs, max_pts, n_q, width, 1, &chunk, &a.w)) return rc;
  a.n_runs = n_runs; a.max_pts = max_pts; a.width = width; a.n_q = n_q; a.extrapolate = extrapolate; a.src = nullptr; a.dst = nullptr;
  A.n_sens = n_sens; A.n_ch = n_ch;
  for (size_t c0 = 0; c0 < (size_t)n; c0 += chunk) {
    a.cell0 = (int)c0; a.n_chunk = (int)std::min(chunk, (size_t)n - c0);
    plpr::launch_chunk(s.st, A);
  }
  FINISH(s);
  for (int c = 0; c < n_ch; c++) { s.back(ch[c].pred, A.ch[c].pred, nq); s.back(ch[c].dpred, A.ch[c].dpred, nq * ns); s.back(ch[c].var, A.ch[c].var, nq); }
  s.back(status, a.status, (size_t)n);
  CHECK_STAGE(s);
  return 0;
}

// ---- plh_lm_step: one Levenberg-Marquardt iteration per cell (kernels: plh_lm.h).  cols, transform and shared bounds are host memory and travel in the kernel argument;
// a PLH_HOST call stages every array whole, both ways: a cell the kernel does not write gets its own bits back ----
int plh_lm_abi_layout(int* out, int cap) {
  const int v[] = {(int)sizeof(plh_lm_opts), 10, (int)offsetof(plh_lm_opts, lambda0), (int)offsetof(plh_lm_opts, lambda_up), (int)offsetof(plh_lm_opts, lambda_down),
                   (int)offsetof(plh_lm_opts, lambda_min), (int)offsetof(plh_lm_opts, lambda_max), (int)offsetof(plh_lm_opts, eta), (int)offsetof(plh_lm_opts, ftol),
                   (int)offsetof(plh_lm_opts, xtol), (int)offsetof(plh_lm_opts, gtol), (int)offsetof(plh_lm_opts, diag_floor)};
  const int nv = (int)(sizeof(v) / sizeof(v[0]));
  for (int k = 0; k < nv && k < cap; k++) if (out) out[k] = v[k];
  return nv;
}
int plh_lm_step(plh_model_t m, int n, int n_theta, double* theta, int n_keys, const int* cols, const int* transform, const double* lo, const double* hi, int bounds_per_cell,
                const double* cost, const double* grad, const double* JtJ, const int* status, double* theta_cur, double* cost_cur, double* grad_cur, double* JtJ_cur,
                double* lambda, double* pred, int* state, int* n_accept, int* n_reject, const plh_lm_opts* opts, int phase, int* n_running, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind);
  if (n < 1 || n_theta < 1) return fail(PLH_E_ARG, "plh_lm_step: n_cells and n_theta must be >= 1");
  if (n_keys < 1 || n_keys > PLH_LSQ_MAX_SENS) return fail(PLH_E_ARG, "plh_lm_step: n_keys must be 1 .. PLH_LSQ_MAX_SENS (8)");
  if (phase != PLH_LM_FIRST && phase != PLH_LM_STEP && phase != PLH_LM_LAST) return fail(PLH_E_ARG, "plh_lm_step: phase must be PLH_LM_FIRST, PLH_LM_STEP or PLH_LM_LAST");
  if (bounds_per_cell != 0 && bounds_per_cell != 1) return fail(PLH_E_ARG, "plh_lm_step: bounds_per_cell must be 0 or 1");
  if (!theta || !cols || !transform || !cost || !grad || !JtJ || !theta_cur || !cost_cur || !grad_cur || !JtJ_cur || !lambda || !pred || !state || !n_accept || !n_reject || !n_running)
    return fail(PLH_E_ARG, "plh_lm_step: null array (only lo, hi, status and the options may be NULL)");
  const plh_lm_opts dflt = PLH_LM_OPTS_DEFAULT;
  const plh_lm_opts o = opts ? *opts : dflt;
  if (!(o.lambda_up > 1.0) || !(o.lambda_down > 0.0 && o.lambda_down < 1.0) || !(o.lambda0 > 0.0) || !(o.lambda_min >= 0.0) || !(o.lambda_max >= o.lambda_min) || !(o.eta >= 0.0) ||
      !(o.ftol >= 0.0) || !(o.xtol >= 0.0) || !(o.gtol >= 0.0) || !(o.diag_floor >= 0.0))
    return fail(PLH_E_ARG, "plh_lm_step: options (lambda_up > 1, 0 < lambda_down < 1, lambda0 > 0, 0 <= lambda_min <= lambda_max, eta and the tolerances >= 0)");
  pllm::Args A;
  A.logmask = 0;
  std::vector<double> shared(2 * (size_t)n_keys);                    // lo, then hi
  for (int i = 0; i < pllm::NK; i++) A.cols[i] = 0;
  for (int i = 0; i < n_keys; i++) {
    if (cols[i] < 0 || cols[i] >= n_theta) return fail(PLH_E_ARG, "plh_lm_step: a column outside [0, n_theta)");
    for (int j = 0; j < i; j++) if (cols[j] == cols[i]) return fail(PLH_E_ARG, "plh_lm_step: a column given twice");
    if (transform[i] != PLH_LM_LINEAR && transform[i] != PLH_LM_LOG) return fail(PLH_E_ARG, "plh_lm_step: transform must be PLH_LM_LINEAR or PLH_LM_LOG");
    A.cols[i] = cols[i];
    if (transform[i] == PLH_LM_LOG) A.logmask |= 1u << i;
    if (!bounds_per_cell) {
      shared[i] = lo ? lo[i] : -HUGE_VAL; shared[n_keys + i] = hi ? hi[i] : HUGE_VAL;
      if (!(shared[i] <= shared[n_keys + i])) return fail(PLH_E_ARG, "plh_lm_step: shared bounds with lo > hi (or a NaN)");
    }
  }
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  const size_t nn = (size_t)n, nk = nn * n_keys, nkk = nk * n_keys, nth = nn * n_theta;
  A.n_cells = n; A.n_theta = n_theta; A.n_keys = n_keys; A.bstride = bounds_per_cell ? n_keys : 0; A.phase = phase; A.o = o;
  A.theta = s.buf(theta, nth, true);
  A.lo = bounds_per_cell ? s.in(lo, nk) : nullptr; A.hi = bounds_per_cell ? s.in(hi, nk) : nullptr;
  if (!bounds_per_cell) {
    const double* d_shared = nullptr;
    if (int rc = s.cx->lm_bounds.get(s.cx->st, shared, &d_shared)) return rc;
    A.lo = d_shared; A.hi = d_shared + n_keys;
  }
  A.cost = s.in(cost, nn); A.grad = s.in(grad, nk); A.JtJ = s.in(JtJ, nkk); A.status = s.in(status, nn);
  A.theta_cur = s.buf(theta_cur, nk, true); A.cost_cur = s.buf(cost_cur, nn, true); A.grad_cur = s.buf(grad_cur, nk, true); A.JtJ_cur = s.buf(JtJ_cur, nkk, true);
  A.lambda = s.buf(lambda, nn, true); A.pred = s.buf(pred, nn, true);
  A.state = s.buf(state, nn, true); A.n_accept = s.buf(n_accept, nn, true); A.n_reject = s.buf(n_reject, nn, true);
  int* d_count = s.buf(n_running, 1, false);
  CHECK_STAGE(s);
  pllm::launch(s.st, A, d_count);
  FINISH(s);
  s.back(theta, A.theta, nth); s.back(theta_cur, A.theta_cur, nk); s.back(cost_cur, A.cost_cur, nn); s.back(grad_cur, A.grad_cur, nk); s.back(JtJ_cur, A.JtJ_cur, nkk);
  s.back(lambda, A.lambda, nn); s.back(pred, A.pred, nn); s.back(state, A.state, nn); s.back(n_accept, A.n_accept, nn); s.back(n_reject, A.n_reject, nn);
  s.back(n_running, d_count, 1);
  CHECK_STAGE(s);
  return 0;
}

// ---- plh_fit_cov: covariances and identifiability of the fitted problems (kernel: plh_cov.h).  transform and shared bounds are host memory; the shared bounds' device copy is
// the one plh_lm_step remembers per stream: after a fit with the same bounds nothing is uploaded and nothing synchronises.  The inputs are only read ----
int plh_fit_cov(plh_model_t m, int n, int n_keys, const int* transform, const double* theta_k, const double* lo, const double* hi, int bounds_per_cell,
                const double* cost, const double* grad, const double* JtJ, const int* n_data, double* sigma2, double* cov, double* stderr_, double* corr,
                double* eval, double* evec, double* collinearity, int* free_mask, int* status, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind);
  if (n < 1) return fail(PLH_E_ARG, "plh_fit_cov: n must be >= 1");
  if (n_keys < 1 || n_keys > PLH_LSQ_MAX_SENS) return fail(PLH_E_ARG, "plh_fit_cov: n_keys must be 1 .. PLH_LSQ_MAX_SENS (8)");
  if (bounds_per_cell != 0 && bounds_per_cell != 1) return fail(PLH_E_ARG, "plh_fit_cov: bounds_per_cell must be 0 or 1");
  if (!transform || !theta_k || !cost || !grad || !JtJ || !sigma2 || !cov || !stderr_ || !corr || !eval || !evec || !collinearity || !free_mask || !status)
    return fail(PLH_E_ARG, "plh_fit_cov: null array (only lo, hi and n_data may be NULL)");
  plcov::Args A;
  A.logmask = 0;
  std::vector<double> shared(2 * (size_t)n_keys);                    // lo, then hi
  for (int i = 0; i < n_keys; i++) {
    if (transform[i] != PLH_LM_LINEAR && transform[i] != PLH_LM_LOG) return fail(PLH_E_ARG, "plh_fit_cov: transform must be PLH_LM_LINEAR or PLH_LM_LOG");
    if (transform[i] == PLH_LM_LOG) A.logmask |= 1u << i;
    if (!bounds_per_cell) {
      shared[i] = lo ? lo[i] : -HUGE_VAL; shared[n_keys + i] = hi ? hi[i] : HUGE_VAL;
      if (!(shared[i] <= shared[n_keys + i])) return fail(PLH_E_ARG, "plh_fit_cov: shared bounds with lo > hi (or a NaN)");
    }
  }
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  const size_t nn = (size_t)n, nk = nn * n_keys, nkk = nk * n_keys;
  A.n = n; A.n_keys = n_keys; A.bstride = bounds_per_cell ? n_keys : 0;
  A.theta = s.in(theta_k, nk);
  A.lo = bounds_per_cell ? s.in(lo, nk) : nullptr; A.hi = bounds_per_cell ? s.in(hi, nk) : nullptr;
  if (!bounds_per_cell) {
    const double* d_shared = nullptr;
    if (int rc = s.cx->lm_bounds.get(s.cx->st, shared, &d_shared)) return rc;
    A.lo = d_shared; A.hi = d_shared + n_keys;
  }
  A.cost = s.in(cost, nn); A.grad = s.in(grad, nk); A.JtJ = s.in(JtJ, nkk); A.n_data = s.in(n_data, nn);
  A.sigma2 = s.buf(sigma2, nn, false); A.cov = s.buf(cov, nkk, false); A.se = s.buf(stderr_, nk, false); A.corr = s.buf(corr, nkk, false);
  A.eval = s.buf(eval, nk, false); A.evec = s.buf(evec, nkk, false); A.coll = s.buf(collinearity, nn, false);
  A.free_mask = s.buf(free_mask, nn, false); A.status = s.buf(status, nn, false);
  CHECK_STAGE(s);
  plcov::launch(s.st, A);
  FINISH(s);
  s.back(sigma2, A.sigma2, nn); s.back(cov, A.cov, nkk); s.back(stderr_, A.se, nk); s.back(corr, A.corr, nkk);
  s.back(eval, A.eval, nk); s.back(evec, A.evec, nkk); s.back(collinearity, A.coll, nn); s.back(free_mask, A.free_mask, nn); s.back(status, A.status, nn);
  CHECK_STAGE(s);
  return 0;
}

// ---- plh_lsq_group / plh_group_scatter: parameters shared by groups of consecutive cells (kernels: plh_group.h).  The offsets and cols are host memory; the offsets' device
// copy is remembered per stream like the shared LM bounds: from the second iteration of a fit on nothing is uploaded and nothing synchronises ----
static int check_groups(const char* who, int n, int n_groups, const int* group_off) {
  if (n < 1) return fail(PLH_E_ARG, std::string(who) + ": n_cells must be >= 1");
  if (n_groups < 1 || n_groups > n) return fail(PLH_E_ARG, std::string(who) + ": n_groups must be 1 .. n_cells");
  if (!group_off) return fail(PLH_E_ARG, std::string(who) + ": null group_off");
  if (group_off[0] != 0 || group_off[n_groups] != n) return fail(PLH_E_ARG, std::string(who) + ": group_off must start at 0 and end at n_cells");
  for (int g = 0; g < n_groups; g++) if (!(group_off[g] < group_off[g + 1])) return fail(PLH_E_ARG, std::string(who) + ": group_off must be strictly ascending (every group has a member)");
  return 0;
}
int plh_lsq_group(plh_model_t m, int n, int n_groups, const int* group_off, int n_sens, const double* cost, const double* grad, const double* JtJ, const int* status,
                  double* g_cost, double* g_grad, double* g_JtJ, int* g_status, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind);
  if (int rc = check_groups("plh_lsq_group", n, n_groups, group_off)) return rc;
  if (n_sens < 0 || n_sens > PLH_LSQ_MAX_SENS) return fail(PLH_E_ARG, "plh_lsq_group: n_sens must be 0 .. PLH_LSQ_MAX_SENS (8)");
  if (!cost || !g_cost) return fail(PLH_E_ARG, "plh_lsq_group: null array (only status and g_status may be NULL)");
  if ((n_sens > 0) != (grad != nullptr) || (n_sens > 0) != (JtJ != nullptr) || (n_sens > 0) != (g_grad != nullptr) || (n_sens > 0) != (g_JtJ != nullptr))
    return fail(PLH_E_ARG, "plh_lsq_group: grad, JtJ, g_grad and g_JtJ are given with n_sens > 0 and NULL with n_sens == 0");
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  const size_t nn = (size_t)n, ng = (size_t)n_groups, ns = (size_t)n_sens;
  plgr::SumArgs A;
  A.n_sens = n_sens;
  A.cost = s.in(cost, nn); A.grad = s.in(grad, nn * ns); A.JtJ = s.in(JtJ, nn * ns * ns); A.status = s.in(status, nn);
  A.g_cost = s.buf(g_cost, ng, false); A.g_grad = s.buf(g_grad, ng * ns, false); A.g_JtJ = s.buf(g_JtJ, ng * ns * ns, false); A.g_status = s.buf(g_status, ng, false);
  CHECK_STAGE(s);
  if (int rc = s.cx->group_off.get(s.cx->st, std::vector<int>(group_off, group_off + n_groups + 1), &A.group_off)) return rc;
  plgr::launch_sum(s.st, n_groups, A);
  FINISH(s);
  s.back(g_cost, A.g_cost, ng); s.back(g_grad, A.g_grad, ng * ns); s.back(g_JtJ, A.g_JtJ, ng * ns * ns); s.back(g_status, A.g_status, ng);
  CHECK_STAGE(s);
  return 0;
}
int plh_group_scatter(plh_model_t m, int n, int n_groups, const int* group_off, int n_theta, int n_keys, const int* cols, const double* g_theta, double* theta, int kind, void* stream) {
  CHECK_MODEL(m); CHECK_KIND(kind);
  if (int rc = check_groups("plh_group_scatter", n, n_groups, group_off)) return rc;
  if (n_theta < 1) return fail(PLH_E_ARG, "plh_group_scatter: n_theta must be >= 1");
  if (n_keys < 1 || n_keys > PLH_LSQ_MAX_SENS) return fail(PLH_E_ARG, "plh_group_scatter: n_keys must be 1 .. PLH_LSQ_MAX_SENS (8)");
  if (!cols || !g_theta || !theta) return fail(PLH_E_ARG, "plh_group_scatter: null array");
  plgr::ScatterArgs A;
  for (int i = 0; i < plgr::NK; i++) A.cols[i] = 0;
  for (int i = 0; i < n_keys; i++) {
    if (cols[i] < 0 || cols[i] >= n_theta) return fail(PLH_E_ARG, "plh_group_scatter: a column outside [0, n_theta)");
    for (int j = 0; j < i; j++) if (cols[j] == cols[i]) return fail(PLH_E_ARG, "plh_group_scatter: a column given twice");
    A.cols[i] = cols[i];
  }
  DeviceGuard guard(m->device);
  Stage s(m, kind, stream);
  const size_t nth = (size_t)n * n_theta;
  A.n_theta = n_theta; A.n_keys = n_keys;
  A.g_theta = s.in(g_theta, (size_t)n_groups * n_theta);
  A.theta = s.buf(theta, nth, true);                                   // (whole, both ways: an entry that is not written keeps its bits)
  CHECK_STAGE(s);
  if (int rc = s.cx->group_off.get(s.cx->st, std::vector<int>(group_off, group_off + n_groups + 1), &A.group_off)) return rc;
  plgr::launch_scatter(s.st, n_groups, A);
  FINISH(s);
  s.back(theta, A.theta, nth);
  CHECK_STAGE(s);
  return 0;
}

double plh_last_kernel_ms(plh_model_t m) {
  if (!m || !m->last || !m->last->timed) return -1.0;
  DeviceGuard guard(m->device);
  if (hipEventSynchronize(m->last->ev1) != hipSuccess) return -1.0;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, m->last->ev0, m->last->ev1) != hipSuccess) return -1.0;
  return (double)ms;
}

int plh_host_alloc(void** p, unsigned long long bytes) {
  if (!p) return fail(PLH_E_ARG, "null argument");
  HIPCHK(hipHostMalloc(p, bytes ? bytes : 8, hipHostMallocDefault));
  return 0;
}
void plh_host_free(void* p) { if (p) hipHostFree(p); }

int plh_synchronize(plh_model_t m, void* stream) {
  CHECK_MODEL(m);
  DeviceGuard guard(m->device);
  StreamCtx& cx = m->ctx((hipStream_t)stream);
  HIPCHK(hipStreamSynchronize(cx.st));
  for (void* p : cx.pending) m->release(p);
  cx.pending.clear();
  HIPCHK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// multi-GPU: RCCL scatter -> local integrate -> RCCL gather.  n_ranks == 1 makes no RCCL call at all.
// ---------------------------------------------------------------------------------------------------------------------
}  // extern "C" (the transport helpers below are internal)

#ifndef PL_WAVE_EMU
#define NCCLCHK(x) do { ncclResult_t r__ = (x); if (r__ != ncclSuccess) return fail(PLH_E_HIP, std::string(#x) + ": " + ncclGetErrorString(r__)); } while (0)
static int x_group_start(plh_comm_s*) { NCCLCHK(ncclGroupStart()); return 0; }
static int x_group_end(plh_comm_s*) { NCCLCHK(ncclGroupEnd()); return 0; }
static int x_send(plh_comm_s* c, const void* dev, size_t bytes, int peer) { NCCLCHK(ncclSend(dev, bytes, ncclChar, peer, c->comm, c->st)); return 0; }
static int x_recv(plh_comm_s* c, void* dev, size_t bytes, int peer) { NCCLCHK(ncclRecv(dev, bytes, ncclChar, peer, c->comm, c->st)); return 0; }
static int x_bcast(plh_comm_s* c, void* dev, size_t bytes, int root) { NCCLCHK(ncclBroadcast(dev, dev, bytes, ncclChar, root, c->comm, c->st)); HIPCHK(hipStreamSynchronize(c->st)); return 0; }
// min over the ranks of a host int, through the communicator's own status word (allocated with the communicator: it does not depend on any staging block of the call)
static int x_allmin(plh_comm_s* c, int* v) {
  HIPCHK(hipMemcpy(c->d_status, v, sizeof(int), hipMemcpyHostToDevice));
  NCCLCHK(ncclAllReduce(c->d_status, c->d_status, 1, ncclInt, ncclMin, c->comm, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipMemcpy(v, c->d_status, sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}
static void x_abort(plh_comm_s* c) { if (c->comm) { ncclCommAbort(c->comm); c->comm = nullptr; } c->dead = true; }
static bool x_multi(const plh_comm_s* c) { return c->comm != nullptr; }
#else
// ---- loopback transport of the emulator build (test infrastructure; never in libpetlion_hip.so) ----
static double x_timeout_s() { const char* e = getenv("PLH_LOOPBACK_TIMEOUT_S"); return e ? atof(e) : 120.0; }
static std::string x_name(const plh_comm_s* c, int src, int dst, long long seq) { return c->dir + "/m_" + std::to_string(src) + "_" + std::to_string(dst) + "_" + std::to_string(seq); }
static int x_group_start(plh_comm_s*) { return 0; }
static int x_group_end(plh_comm_s*) { return 0; }
static int x_send(plh_comm_s* c, const void* buf, size_t bytes, int peer) {
  const std::string nm = x_name(c, c->rank, peer, c->seq_tx[peer]++), tmp = nm + ".part";
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f || (bytes && fwrite(buf, 1, bytes, f) != bytes)) { if (f) fclose(f); return fail(PLH_E_HIP, "loopback send: cannot write " + tmp); }
  fclose(f);
  if (rename(tmp.c_str(), nm.c_str()) != 0) return fail(PLH_E_HIP, "loopback send: rename failed for " + nm);
  return 0;
}
static int x_recv(plh_comm_s* c, void* buf, size_t bytes, int peer) {
  const std::string nm = x_name(c, peer, c->rank, c->seq_rx[peer]++);
  const double limit = x_timeout_s();
  for (double waited = 0.0;; waited += 0.002) {
    struct stat sb;
    if (stat(nm.c_str(), &sb) == 0) {
      if ((size_t)sb.st_size != bytes) return fail(PLH_E_HIP, "loopback recv: " + nm + " has " + std::to_string((long long)sb.st_size) + " bytes, expected " + std::to_string(bytes));
      FILE* f = fopen(nm.c_str(), "rb");
      const bool ok = f && (bytes == 0 || fread(buf, 1, bytes, f) == bytes);
      if (f) fclose(f);
      unlink(nm.c_str());
      return ok ? 0 : fail(PLH_E_HIP, "loopback recv: cannot read " + nm);
    }
    if (waited > limit) return fail(PLH_E_HIP, "loopback recv: timed out waiting for rank " + std::to_string(peer) + " (" + nm + ")");
    usleep(2000);
  }
}
static int x_bcast(plh_comm_s* c, void* buf, size_t bytes, int root) {
  if (c->rank == root) { for (int r = 0; r < c->n_ranks; r++) if (r != root) if (int rc = x_send(c, buf, bytes, r)) return rc; return 0; }
  return x_recv(c, buf, bytes, root);
}
static int x_allmin(plh_comm_s* c, int* v) {
  if (c->rank != 0) { if (int rc = x_send(c, v, sizeof(int), 0)) return rc; return x_recv(c, v, sizeof(int), 0); }
  for (int r = 1; r < c->n_ranks; r++) { int o = 0; if (int rc = x_recv(c, &o, sizeof(int), r)) return rc; if (o < *v) *v = o; }
  for (int r = 1; r < c->n_ranks; r++) if (int rc = x_send(c, v, sizeof(int), r)) return rc;
  return 0;
}
static void x_abort(plh_comm_s* c) { c->dead = true; }
static bool x_multi(const plh_comm_s* c) { return c->comm; }
// fault injection for the tests: PLH_TEST_FAIL = "<rank>:<phase>" makes that rank fail locally at that phase of plh_ensemble_run (0 arguments, 1 shape, 2 scatter
// preparation, 3 integrate, 4 inside the gather -- a failure INSIDE a collective phase, which the others can only time out on)
static bool x_inject(const plh_comm_s* c, int phase) {
  const char* e = getenv("PLH_TEST_FAIL"); int r = -1, ph = -1;
  return e && sscanf(e, "%d:%d", &r, &ph) == 2 && r == c->rank && ph == phase;
}
#endif
#ifndef PL_WAVE_EMU
static bool x_inject(const plh_comm_s*, int) { return false; }
#endif

extern "C" {

int plh_comm_unique_id(char id[128]) {
  if (!id) return fail(PLH_E_ARG, "null argument");
#ifndef PL_WAVE_EMU
  static_assert(sizeof(ncclUniqueId) == 128, "the 128-byte id of the header is ncclUniqueId");
  ncclUniqueId u; NCCLCHK(ncclGetUniqueId(&u)); memcpy(id, &u, 128);
#else
  // the id of the loopback transport is the name of a fresh directory (the ranks exchange their messages through it)
  memset(id, 0, 128);
  const char* base = getenv("TMPDIR"); std::string t = std::string(base && *base ? base : "/tmp") + "/plh_loopback_XXXXXX";
  if (t.size() >= 127 || !mkdtemp(&t[0])) return fail(PLH_E_HIP, "loopback: cannot create a message directory");
  memcpy(id, t.c_str(), t.size());
#endif
  return 0;
}

int plh_comm_create(int n_ranks, int rank, const char id[128], int device, plh_comm_t* out) {
  if (!out || n_ranks < 1 || rank < 0 || rank >= n_ranks || (n_ranks > 1 && !id)) return fail(PLH_E_ARG, "bad argument");
  plh_comm_s* c = new plh_comm_s();
  c->n_ranks = n_ranks; c->rank = rank;
#ifndef PL_WAVE_EMU
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { delete c; return fail(PLH_E_HIP, "no HIP device visible"); }
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) { delete c; return fail(PLH_E_HIP, "hipGetDevice failed"); } }
  if (device >= ndev) { delete c; return fail(PLH_E_ARG, "device ordinal out of range"); }
  c->device = device;
  DeviceGuard guard(device);
  if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess) { delete c; return fail(PLH_E_HIP, "hipStreamCreate failed"); }
  // the status word of the agreements between the phases of plh_ensemble_run: owned by the communicator, checked HERE, so that a staging failure of a later call can still be
  // agreed on (the word used to live in a staging block of the call itself)
  if (hipMalloc((void**)&c->d_status, 2 * sizeof(int)) != hipSuccess) { hipStreamDestroy(c->st); delete c; return fail(PLH_E_HIP, "hipMalloc failed (communicator status word)"); }
  if (id) {        // (a one-rank communicator with an id still initialises RCCL: the collective path then runs end to end on a single GPU)
    ncclUniqueId u; memcpy(&u, id, 128);
    const ncclResult_t r = ncclCommInitRank(&c->comm, n_ranks, u, rank);
    if (r != ncclSuccess) { hipFree(c->d_status); hipStreamDestroy(c->st); delete c; return fail(PLH_E_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r)); }
  }
#else
  c->device = 0; (void)device;
  if (id && id[0]) {
    c->dir.assign(id, strnlen(id, 127));
    struct stat sb;
    if (stat(c->dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) { delete c; return fail(PLH_E_ARG, "loopback: the id does not name a message directory (plh_comm_unique_id)"); }
    c->comm = true;
  } else if (n_ranks > 1) { delete c; return fail(PLH_E_ARG, "a communicator of several ranks needs the id of plh_comm_unique_id"); }
  c->seq_tx.assign(n_ranks, 0); c->seq_rx.assign(n_ranks, 0);
#endif
  *out = c;
  return 0;
}

void plh_comm_destroy(plh_comm_t c) {
  if (!c) return;
#ifndef PL_WAVE_EMU
  DeviceGuard guard(c->device);
  if (c->comm) ncclCommDestroy(c->comm);
  if (c->d_status) hipFree(c->d_status);
  if (c->st) hipStreamDestroy(c->st);
#endif
  delete c;
}
int plh_comm_rank(plh_comm_t c) { return c ? c->rank : PLH_E_ARG; }
int plh_comm_size(plh_comm_t c) { return c ? c->n_ranks : PLH_E_ARG; }

// shard of rank r: count, and the global cell index of its k-th cell
static inline long long shard_count(long long n, int G, int r) { return n / G + (r < n % G ? 1 : 0); }
static inline long long shard_cell(long long n, int G, int r, long long k, int partition) {
  if (partition == PLH_PART_CYCLIC) return r + k * G;
  const long long base = n / G, rem = n % G;
  return r * base + (r < rem ? r : rem) + k;
}

int plh_ensemble_run(plh_comm_t c, plh_model_t m, int n_total, const double* theta, const double* SOC0, int n_runs, const plh_run* runs,
                     const plh_opts* opts, int partition, plh_run_info* run_info, plh_counters* counters, double* Y_final, double* rank_ms) {
  CHECK_MODEL(m);
  // (misuse that every rank sees alike -- all ranks pass the same shape, protocol and options -- returns at once; everything that can differ between ranks is agreed on below)
  if (!c || n_total <= 0 || n_runs <= 0 || !runs || !opts) return fail(PLH_E_ARG, "bad argument");
  if (partition != PLH_PART_BLOCK && partition != PLH_PART_CYCLIC) return fail(PLH_E_ARG, "partition must be PLH_PART_BLOCK or PLH_PART_CYCLIC");
  if (c->dead) return fail(PLH_E_HIP, "plh_ensemble_run: this communicator was aborted by an earlier transport failure; destroy it and create a new one");
  const int G = c->n_ranks, me = c->rank; const bool root = me == 0;
  const bool multi = x_multi(c) && G > 1;
  DeviceGuard guard(m->device);
  const int P = m->P, N = m->N;
  const long long cnt = shard_count(n_total, G, me);
  std::vector<long long> off(G + 1, 0);
  for (int r = 0; r < G; r++) off[r + 1] = off[r] + shard_count(n_total, G, r);
#ifndef PL_WAVE_EMU
  hipStream_t st = c->st;
#else
  hipStream_t st = nullptr;
#endif
  // device blocks (cached in the handle): root holds the whole permuted ensemble, the others their shard
  Stage s(m, PLH_DEVICE, st);
  SyncFirst sync_first{st, true};     // (destroyed before `s`: no staging block is released while a collective that targets it is still enqueued)
  const size_t rows = root ? (size_t)n_total : (size_t)(cnt > 0 ? cnt : 1);
  double* d_th = (double*)s.dev_block(rows * P * sizeof(double));
  double* d_soc = (double*)s.dev_block(rows * sizeof(double));
  plh_run_info* d_info = (plh_run_info*)s.dev_block(rows * n_runs * sizeof(plh_run_info));
  plh_counters* d_cnt = (plh_counters*)s.dev_block(rows * sizeof(plh_counters));
  double* d_Y = (double*)s.dev_block(rows * N * sizeof(double));
  long long* d_meta = (long long*)s.dev_block(8 * sizeof(long long));
  double* d_ms = (double*)s.dev_block((size_t)G * sizeof(double));
  // A return that only ONE rank takes would leave the others blocked in the next send / receive: before every collective phase the ranks agree on a status (all-reduce of
  // the most negative return code, through the communicator's own status word) and leave together.  Local failures BETWEEN the collectives -- arguments, staging, host /
  // device copies, the rank's plh_integrate -- only set `rc0`; a transport failure INSIDE a collective phase cannot be agreed on any more: the communicator is aborted.
  auto agree = [&](int rc, const char* where) -> int {
    if (multi) {
      int all = rc;
      if (x_allmin(c, &all) != 0) { x_abort(c); return rc != 0 ? rc : fail(PLH_E_HIP, std::string("plh_ensemble_run: status exchange failed (") + where + "): " + g_err); }
      if (rc == 0 && all != 0) return fail(all, std::string("plh_ensemble_run: another rank failed (") + where + "); see its plh_last_error()");
    }
    return rc;
  };
  auto broken = [&](const char* where) -> int { const std::string why = g_err; x_abort(c); return fail(PLH_E_HIP, std::string("plh_ensemble_run: transport failure in ") + where + " (communicator aborted): " + why); };
#define PL_LOCAL(x) do { if (rc0 == 0) { hipError_t e__ = (x); if (e__ != hipSuccess) rc0 = fail(PLH_E_HIP, std::string(#x) + ": " + hipGetErrorString(e__)); } } while (0)
  int rc0 = 0;
  if (s.bad) rc0 = fail(PLH_E_HIP, s.why);
  else if (root && (!theta || !SOC0 || !run_info)) rc0 = fail(PLH_E_ARG, "rank 0 needs theta, SOC0 and run_info");
  else if (m->device != c->device) rc0 = fail(PLH_E_ARG, "the model handle and the communicator must be bound to the same device");
  if (x_inject(c, 0)) rc0 = fail(PLH_E_ARG, "injected failure (arguments)");
  if (int rc = agree(rc0, "arguments / staging")) return rc;
  // 1. shape check: everybody must describe the same ensemble (broadcast from rank 0)
  long long meta[4] = {n_total, n_runs, partition, P};
  if (x_multi(c)) {
    long long root_meta[4] = {0, 0, 0, 0};
    if (root) PL_LOCAL(hipMemcpy(d_meta, meta, sizeof(meta), hipMemcpyHostToDevice));
    if (int rc = agree(rc0, "ensemble shape upload")) return rc;
    if (x_bcast(c, d_meta, sizeof(meta), 0) != 0) return broken("the shape broadcast");
    PL_LOCAL(hipMemcpy(root_meta, d_meta, sizeof(meta), hipMemcpyDeviceToHost));
    if (rc0 == 0 && memcmp(root_meta, meta, sizeof(meta)) != 0) rc0 = fail(PLH_E_ARG, "plh_ensemble_run: this rank's (n_cells_total, n_runs, partition, model) differ from rank 0's");
    if (x_inject(c, 1)) rc0 = fail(PLH_E_ARG, "injected failure (shape)");
  }
  // per-cell protocol arrays (plh_run.value_cell / tf_cell) are indexed by the GLOBAL cell: n_cells_total entries, the same on every rank like the rest of the protocol.
  // plh_integrate indexes them by the LOCAL cell, so each rank hands it its own shard of them, in shard order.
  std::vector<plh_run> lruns(runs, runs + n_runs);
  std::vector<std::vector<double>> shard_vals;
  for (int r = 0; r < n_runs; r++) {
    for (int which = 0; which < 2; which++) {
      const double* src = which == 0 ? runs[r].value_cell : runs[r].tf_cell;
      if (!src) continue;
      std::vector<double> v((size_t)(cnt > 0 ? cnt : 1));
      for (long long k = 0; k < cnt; k++) v[k] = src[shard_cell(n_total, G, me, k, partition)];
      shard_vals.push_back(std::move(v));
      (which == 0 ? lruns[r].value_cell : lruns[r].tf_cell) = shard_vals.back().data();
    }
  }
  // 2. scatter of the parameter rows (rank 0 permutes them into rank-contiguous order first)
  if (root && rc0 == 0) {
    std::vector<double> th((size_t)n_total * P), soc(n_total);
    for (int r = 0; r < G; r++) for (long long k = 0; k < off[r + 1] - off[r]; k++) {
      const long long cell = shard_cell(n_total, G, r, k, partition);
      memcpy(&th[(size_t)(off[r] + k) * P], theta + (size_t)cell * P, P * sizeof(double)); soc[off[r] + k] = SOC0[cell];
    }
    PL_LOCAL(hipMemcpy(d_th, th.data(), th.size() * sizeof(double), hipMemcpyHostToDevice));
    PL_LOCAL(hipMemcpy(d_soc, soc.data(), soc.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (x_inject(c, 2)) rc0 = fail(PLH_E_HIP, "injected failure (scatter preparation)");
  if (int rc = agree(rc0, "ensemble shape / scatter preparation")) return rc;
  if (multi) {
    bool ok = x_group_start(c) == 0;
    if (root) { for (int r = 1; ok && r < G; r++) if (off[r + 1] > off[r]) ok = x_send(c, d_th + (size_t)off[r] * P, (size_t)(off[r + 1] - off[r]) * P * sizeof(double), r) == 0 &&
                                                                                x_send(c, d_soc + off[r], (size_t)(off[r + 1] - off[r]) * sizeof(double), r) == 0; }
    else if (cnt > 0) ok = ok && x_recv(c, d_th, (size_t)cnt * P * sizeof(double), 0) == 0 && x_recv(c, d_soc, (size_t)cnt * sizeof(double), 0) == 0;
    ok = ok && x_group_end(c) == 0;
    if (!ok) return broken("the scatter");
  }
  // 3. the local shard: one plh_integrate launch, device pointers, on the communicator's stream -- no collective in the data path
  double ms = 0.0;
  if (cnt > 0) {
    plh_outputs o; memset(&o, 0, sizeof(o));
    o.max_pts = 0; o.run_info = d_info; o.counters = d_cnt; o.Y_final = d_Y;
    rc0 = plh_integrate(m, (int)cnt, d_th, d_soc, nullptr, nullptr, n_runs, lruns.data(), opts, &o, PLH_DEVICE, st);
    if (rc0 == 0) ms = plh_last_kernel_ms(m);
  }
  if (x_inject(c, 3)) rc0 = fail(PLH_E_HIP, "injected failure (integrate)");
  PL_LOCAL(hipMemcpy(d_ms + me, &ms, sizeof(double), hipMemcpyHostToDevice));
  if (int rc = agree(rc0, "plh_integrate")) return rc;
  // 4. gather of the per-cell summaries to rank 0 (rank-contiguous order), then back to the caller's cell order
  if (multi) {
    if (x_inject(c, 4)) return broken("the gather (injected)");
    const size_t bi = (size_t)n_runs * sizeof(plh_run_info), bc = sizeof(plh_counters);
    bool ok = x_group_start(c) == 0;
    if (root) for (int r = 1; ok && r < G; r++) {
      const size_t k = (size_t)(off[r + 1] - off[r]);
      if (k) ok = x_recv(c, (char*)d_info + (size_t)off[r] * bi, k * bi, r) == 0 && x_recv(c, (char*)d_cnt + (size_t)off[r] * bc, k * bc, r) == 0 &&
                  x_recv(c, d_Y + (size_t)off[r] * N, k * N * sizeof(double), r) == 0;
      ok = ok && x_recv(c, d_ms + r, sizeof(double), r) == 0;
    } else {
      if (cnt > 0) ok = ok && x_send(c, d_info, (size_t)cnt * bi, 0) == 0 && x_send(c, d_cnt, (size_t)cnt * bc, 0) == 0 && x_send(c, d_Y, (size_t)cnt * N * sizeof(double), 0) == 0;
      ok = ok && x_send(c, d_ms + me, sizeof(double), 0) == 0;
    }
    ok = ok && x_group_end(c) == 0;
    if (!ok) return broken("the gather");
  }
  // (no collective after this point: a local failure is this rank's alone)
  HIPCHK(hipStreamSynchronize(st));
  if (root) {
    std::vector<plh_run_info> hi((size_t)n_total * n_runs); std::vector<plh_counters> hc(counters ? n_total : 0); std::vector<double> hy(Y_final ? (size_t)n_total * N : 0);
    HIPCHK(hipMemcpy(hi.data(), d_info, hi.size() * sizeof(plh_run_info), hipMemcpyDeviceToHost));
    if (counters) HIPCHK(hipMemcpy(hc.data(), d_cnt, hc.size() * sizeof(plh_counters), hipMemcpyDeviceToHost));
    if (Y_final) HIPCHK(hipMemcpy(hy.data(), d_Y, hy.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (rank_ms) HIPCHK(hipMemcpy(rank_ms, d_ms, (size_t)G * sizeof(double), hipMemcpyDeviceToHost));
    for (int r = 0; r < G; r++) for (long long k = 0; k < off[r + 1] - off[r]; k++) {
      const long long cell = shard_cell(n_total, G, r, k, partition), q = off[r] + k;
      memcpy(run_info + (size_t)cell * n_runs, &hi[(size_t)q * n_runs], (size_t)n_runs * sizeof(plh_run_info));
      if (counters) counters[cell] = hc[q];
      if (Y_final) memcpy(Y_final + (size_t)cell * N, &hy[(size_t)q * N], N * sizeof(double));
    }
  }
  return 0;
#undef PL_LOCAL
}

}  // extern "C"

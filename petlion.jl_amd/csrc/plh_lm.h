// plh_lm.h -- plh_lm_step: one Levenberg-Marquardt iteration of every cell's fit (include/petlion_hip.h states the definition, sentence by sentence what k_lm_step does).
// Like plh_resample.h / plh_lsq.h: no model variant, host translation unit.
//
//   k_lm_step    one block = one wave = 64 consecutive cells, lanes = cells.  The work of a cell is a k <= 8 Cholesky (a few hundred flops): the kernel is bound by its loads.
//                Per-cell scalars (cost, lambda, state, ...) are coalesced as they are.  The k x k matrices are cell-major, so the block's 64 matrices are ONE contiguous
//                segment: lanes run along it (load and store) and the matrix lives in LDS as M[entry][cell] (rows padded to 65: lanes = cells read without a bank conflict).
//                  phase A   lanes = segment: JtJ -> M.                      lanes = cells: judge the trial (needs every number of the fit), decide
//                  phase B   lanes = segment: accepting cells  M -> JtJ_cur, rejecting cells  JtJ_cur -> M, done cells: nothing
//                  phase C   lanes = cells: scale, active set, tests, the damped solves, the outputs
//                One instantiation per k = 1 .. 8: every loop over keys is unrolled to it, so the vectors of a cell stay in registers and every LDS address of phase C is
//                lane + a constant (a matrix entry (i, j) sits in row 8 i + j of M whatever k is).  A held key is an identity row of A, through a factor, not a branch.
//                After phase B the strict upper triangle of a cell's M column holds Hs, the lower triangle and the diagonal hold the Cholesky factor of the current try;
//                Hs's diagonal is in registers; bounds, damping diagonal and the factors of the held keys are in LDS too (W), the options as well.  50 kB of LDS per block,
//                no scratch and no register spills in any of the eight instantiations.
//   k_lm_count   one block: the number of running cells, lanes stride the states, one butterfly (integers in doubles: exact, any order gives the same sum).
#pragma once

#include <cfloat>

#include "plh_resample.h"

namespace pllm {

constexpr int NK = PLH_LSQ_MAX_SENS;      // keys at most
constexpr int TILE = 64;                  // cells per block = lanes
constexpr int LD = TILE + 1;              // M's row: 64 cells and one of padding

struct Args {
  int n_cells, n_theta, n_keys, phase;
  int bstride;                              // lo / hi of cell c, key i: [c bstride + i] (per-cell bounds: n_keys; shared bounds: 0, the device copy of the host's [n_keys])
  unsigned logmask;                         // bit i: key i is PLH_LM_LOG
  int cols[NK];
  plh_lm_opts o;
  double* theta; const double* lo; const double* hi;      // either may be NULL (no bound on that side)
  const double* cost; const double* grad; const double* JtJ; const int* status;
  double* theta_cur; double* cost_cur; double* grad_cur; double* JtJ_cur; double* lambda; double* pred;
  int* state; int* n_accept; int* n_reject;
};

__device__ inline bool lm_finite(double x) { return fabs(x) <= DBL_MAX; }      // (false for NaN)

// what phase A decides for a cell
enum { LM_SKIP = 0,       // done before the call, or a bad start: none of its arrays is touched in phases B and C
       LM_TAKE = 1,       // FIRST on a good start, or an accepted trial: cur <- the incoming fit
       LM_KEEP = 2 };     // a rejected trial: the fit of cur is loaded

template <int K>                          // = n_keys: the loops over keys are unrolled to it, so the vectors of a cell stay in registers and nothing is predicated on k
__global__ void __launch_bounds__(TILE) k_lm_step(Args a) {
  __shared__ double M[NK * NK][LD];
  __shared__ double W[4 * NK][LD];
  __shared__ int what[TILE];
  constexpr int k = K, kk = K * K;
  const int lane = (int)threadIdx.x;
  const size_t cell0 = (size_t)blockIdx.x * TILE, cell = cell0 + lane;
  const int nb = (int)((size_t)a.n_cells - cell0 < (size_t)TILE ? (size_t)a.n_cells - cell0 : (size_t)TILE);      // cells of this block
  const bool live = lane < nb;
  // the options go through LDS: ten doubles that stay live to the end of the kernel are twenty scalar registers the kernel does not have
  __shared__ plh_lm_opts so;
  if (lane == 0) so = a.o;
  const plh_lm_opts& o = so;
  auto ent = [](int e) { return e / K * NK + e % K; };             // entry e of a k x k matrix -> its row of M: (i, j) sits at i NK + j whatever k is

  // ---- phase A: the incoming JtJ, lanes along the block's segment
  for (int x = lane; x < nb * kk; x += TILE) M[ent(x % kk)][x / kk] = a.JtJ[cell0 * kk + x];
  __syncthreads();

  int st = PLH_LM_RUNNING, act = LM_SKIP, nacc = 0, nrej = 0;
  double lam = 0.0, ccur = 0.0, prd = 0.0;
  double th[NK], g[NK];                                              // cur: theta among cols, gradient
  if (live) {
    const int st_in = a.phase == PLH_LM_FIRST ? PLH_LM_RUNNING : a.state[cell];
    if (st_in == PLH_LM_RUNNING) {
      const double cost = a.cost[cell];
      bool ok = (a.status ? a.status[cell] : 0) == 0 && lm_finite(cost);
      double gin[NK], tin[NK];
#pragma unroll
      for (int i = 0; i < NK; i++) {
        gin[i] = 0.0; tin[i] = 1.0;
        if (i < k) {
          gin[i] = a.grad[cell * k + i]; tin[i] = a.theta[cell * a.n_theta + a.cols[i]];
          ok = ok && lm_finite(gin[i]);
#pragma unroll
          for (int j = i; j < NK; j++) if (j < k) ok = ok && lm_finite(M[i * NK + j][lane]);
        }
      }
      if (a.phase == PLH_LM_FIRST) {
#pragma unroll
        for (int i = 0; i < NK; i++) if (i < k) {
          const double l = a.lo ? a.lo[cell * a.bstride + i] : -HUGE_VAL, h = a.hi ? a.hi[cell * a.bstride + i] : HUGE_VAL;
          ok = ok && lm_finite(tin[i]) && l <= tin[i] && tin[i] <= h && !((a.logmask >> i & 1) && tin[i] <= 0.0);
        }
        if (!ok) a.state[cell] = PLH_LM_FAILED_START;
        else { act = LM_TAKE; lam = o.lambda0; ccur = cost; }
      } else {
        lam = a.lambda[cell]; prd = a.pred[cell]; nacc = a.n_accept[cell]; nrej = a.n_reject[cell];
        const double cold = a.cost_cur[cell], actual = cold - cost;
        if (ok && actual >= o.eta * prd) {
          act = LM_TAKE; ccur = cost; nacc++;
          lam = fmax(lam * o.lambda_down, o.lambda_min);
          if (actual <= o.ftol * cold) st = PLH_LM_CONV_F;
        } else {
          act = LM_KEEP; ccur = cold; nrej++;
          lam = lam * o.lambda_up;
          if (lam > o.lambda_max) st = PLH_LM_STALLED;
        }
        if (a.phase == PLH_LM_LAST && st == PLH_LM_RUNNING) st = PLH_LM_MAXIT;
      }
      if (act != LM_SKIP) { a.n_accept[cell] = nacc; a.n_reject[cell] = nrej; }      // (final here)
      if (act == LM_TAKE) {
        a.cost_cur[cell] = ccur;
#pragma unroll
        for (int i = 0; i < NK; i++) { th[i] = tin[i]; g[i] = gin[i]; if (i < k) { a.theta_cur[cell * k + i] = th[i]; a.grad_cur[cell * k + i] = g[i]; } }
      } else if (act == LM_KEEP) {
#pragma unroll
        for (int i = 0; i < NK; i++) { th[i] = 1.0; g[i] = 0.0; if (i < k) { th[i] = a.theta_cur[cell * k + i]; g[i] = a.grad_cur[cell * k + i]; } }
      }
    }
  }
  what[lane] = act;
  __syncthreads();

  // ---- phase B: the fit of cur, lanes along the segment again
  for (int x = lane; x < nb * kk; x += TILE) {
    const int w = what[x / kk];
    if (w == LM_TAKE) a.JtJ_cur[cell0 * kk + x] = M[ent(x % kk)][x / kk];
    else if (w == LM_KEEP) M[ent(x % kk)][x / kk] = a.JtJ_cur[cell0 * kk + x];
  }
  __syncthreads();
  if (act == LM_SKIP) return;

  // ---- phase C: lanes = cells
  double tr[NK];                                                     // what the theta row receives: cur, or the trial
#pragma unroll
  for (int i = 0; i < NK; i++) tr[i] = th[i];
  // per-key vectors of a cell that the tries only read go to LDS as well (W[vector][key][cell]): in registers they are 64 more per lane than there are
#define LO(i) W[0 * NK + (i)][lane]
#define HI(i) W[1 * NK + (i)][lane]
#define DD(i) W[2 * NK + (i)][lane]
#define FF(i) W[3 * NK + (i)][lane]
  if (st == PLH_LM_RUNNING) {
    // keys >= k and held keys are identity rows of A.  That is done with factors, f_i = 1 for a key that is solved for and 0 otherwise, not with per-lane conditions: a
    // condition that does not change from try to try is hoisted out of the loop over the tries, and 28 of them are 56 scalar registers
    double s[NK], Hd[NK], d[NK];
    double hmax = -HUGE_VAL;
    bool fin = true;
#pragma unroll
    for (int i = 0; i < NK; i++) {
      s[i] = 1.0; Hd[i] = 0.0; d[i] = 0.0;
      if (i < k) {
        LO(i) = a.lo ? a.lo[cell * a.bstride + i] : -HUGE_VAL;
        HI(i) = a.hi ? a.hi[cell * a.bstride + i] : HUGE_VAL;
        if (a.logmask >> i & 1) s[i] = th[i];
      }
    }
#pragma unroll
    for (int i = 0; i < NK; i++) if (i < k) {
      g[i] = s[i] * g[i];
      Hd[i] = (s[i] * s[i]) * M[i * NK + i][lane];
      hmax = fmax(hmax, Hd[i]);
      fin = fin && lm_finite(g[i]) && lm_finite(Hd[i]);
#pragma unroll
      for (int j = i + 1; j < NK; j++) if (j < k) { const double v = (s[i] * s[j]) * M[i * NK + j][lane]; M[i * NK + j][lane] = v; fin = fin && lm_finite(v); }
    }
    bool gsmall = true;
#pragma unroll
    for (int i = 0; i < NK; i++) if (i < k) {
      const bool held = (th[i] <= LO(i) && g[i] > 0.0) || (th[i] >= HI(i) && g[i] < 0.0);
      FF(i) = held ? 0.0 : 1.0;
      gsmall = gsmall && (held || fabs(g[i]) <= o.gtol * sqrt(Hd[i] * (2.0 * ccur)));
      DD(i) = fmax(Hd[i], o.diag_floor * hmax);
    }
    if (!fin) st = PLH_LM_STALLED;
    else if (ccur == 0.0 || gsmall) st = PLH_LM_CONV_G;              // (no free key: gsmall is true)
    for (int t = 0; st == PLH_LM_RUNNING; t++) {
      if (t == PLH_LM_MAX_TRIES) { st = PLH_LM_STALLED; break; }
      // A = L L^T row by row.  L_ij (i > j) -> M[8 i + j], L_ii -> M[8 i + i]; Hs_ij (i < j) stays in M[8 i + j]
      bool fail = false;
#pragma unroll
      for (int i = 0; i < NK; i++) if (i < k) {
#pragma unroll
        for (int j = 0; j < i; j++) {
          double v = M[j * NK + i][lane];
#pragma unroll
          for (int p = 0; p < j; p++) v -= M[i * NK + p][lane] * M[j * NK + p][lane];
          M[i * NK + j][lane] = (FF(i) * FF(j)) * (v / M[j * NK + j][lane]);
        }
        double v = FF(i) * (Hd[i] + lam * DD(i)) + (1.0 - FF(i));
#pragma unroll
        for (int p = 0; p < i; p++) v -= M[i * NK + p][lane] * M[i * NK + p][lane];
        if (!(v > 0.0) || !lm_finite(v)) { fail = true; v = 1.0; }
        M[i * NK + i][lane] = sqrt(v);
      }
      // L y = -gs, then L^T d = y
#pragma unroll
      for (int i = 0; i < NK; i++) if (i < k) {
        double v = -(FF(i) * g[i]);
#pragma unroll
        for (int p = 0; p < i; p++) v -= M[i * NK + p][lane] * d[p];
        d[i] = v / M[i * NK + i][lane];
      }
#pragma unroll
      for (int i = NK - 1; i >= 0; i--) if (i < k) {
        double v = d[i];
#pragma unroll
        for (int p = i + 1; p < NK; p++) if (p < k) v -= M[p * NK + i][lane] * d[p];
        d[i] = v / M[i * NK + i][lane];
      }
      // the trial, clamped; d becomes the step taken (a held key has d = 0: its trial is theta itself, inside its bounds)
#pragma unroll
      for (int i = 0; i < NK; i++) if (i < k) {
        const bool lg = a.logmask >> i & 1;
        double v = lg ? th[i] * exp(d[i]) : th[i] + d[i];
        if (v < LO(i) || v > HI(i)) {
          v = v < LO(i) ? LO(i) : HI(i);
          d[i] = lg ? log(v / th[i]) : v - th[i];
        }
        tr[i] = v;
        fail = fail || !lm_finite(v) || !lm_finite(d[i]);
      }
      // pred = -(gs.d + 1/2 d.Hs d)
      double gd = 0.0, dHd = 0.0;
#pragma unroll
      for (int i = 0; i < NK; i++) if (i < k) {
        gd += g[i] * d[i];
        double r = Hd[i] * d[i];
#pragma unroll
        for (int j = 0; j < NK; j++) if (j < k && j != i) r += (j > i ? M[i * NK + j][lane] : M[j * NK + i][lane]) * d[j];
        dHd += d[i] * r;
      }
      const double pr = -(gd + 0.5 * dHd);
      fail = fail || !(pr > 0.0) || !lm_finite(pr);
      if (fail) {
        lam = lam * o.lambda_up;
        if (lam > o.lambda_max) st = PLH_LM_STALLED;
        continue;
      }
      bool xsmall = true;
#pragma unroll
      for (int i = 0; i < NK; i++) if (i < k) {
        const double mi = (a.logmask >> i & 1) ? fabs(d[i]) : fabs(d[i]) / fmax(fabs(th[i]), DBL_MIN);
        xsmall = xsmall && mi <= o.xtol;
      }
      if (xsmall) st = PLH_LM_CONV_X;
      else prd = pr;
      break;
    }
  }
#undef LO
#undef HI
#undef DD
#undef FF
  const bool step = st == PLH_LM_RUNNING;                            // else theta is (or returns to) cur
#pragma unroll
  for (int i = 0; i < NK; i++) if (i < k) a.theta[cell * a.n_theta + a.cols[i]] = step ? tr[i] : th[i];
  a.lambda[cell] = lam; a.pred[cell] = prd; a.state[cell] = st;
}

// the number of running cells (one block)
__global__ void __launch_bounds__(TILE) k_lm_count(const int* state, int n, int* out) {
  const int lane = (int)threadIdx.x;
  double c = 0.0;
  for (int x = lane; x < n; x += TILE) c += state[x] == PLH_LM_RUNNING ? 1.0 : 0.0;
  for (int m = TILE / 2; m >= 1; m >>= 1) c += __shfl_xor(c, m);
  if (lane == 0) *out = (int)c;
}

inline void launch(hipStream_t st, const Args& a, int* d_count) {
  const unsigned grid = (unsigned)((a.n_cells + TILE - 1) / TILE);
  switch (a.n_keys) {
    case 1: PL_LAUNCH(k_lm_step<1>, grid, TILE, st, a); break;
    case 2: PL_LAUNCH(k_lm_step<2>, grid, TILE, st, a); break;
    case 3: PL_LAUNCH(k_lm_step<3>, grid, TILE, st, a); break;
    case 4: PL_LAUNCH(k_lm_step<4>, grid, TILE, st, a); break;
    case 5: PL_LAUNCH(k_lm_step<5>, grid, TILE, st, a); break;
    case 6: PL_LAUNCH(k_lm_step<6>, grid, TILE, st, a); break;
    case 7: PL_LAUNCH(k_lm_step<7>, grid, TILE, st, a); break;
    default: PL_LAUNCH(k_lm_step<8>, grid, TILE, st, a); break;
  }
  PL_LAUNCH(k_lm_count, 1u, TILE, st, (const int*)a.state, a.n_cells, d_count);
}

}  // namespace pllm

// plh_predict.h -- plh_predict: every cell's measured curves (V, I, T_avg) and their per-point sensitivities resampled at query times, and the delta-method variance of the
// resampled curve under the covariance of the fitted keys (include/petlion_hip.h states the definition).  Like plh_lsq.h: kernels over the saved points
// plh_integrate_sens_out wrote, no model variant, host translation unit.
//
// The functions S_c and S_ck are plh_resample's, so k_resample_prep and k_resample_locate run unchanged.  Then one kernel:
//   k_predict_cell   one wave per cell over its n_ch (1 + n_sens) columns, in k_lsq_cell's three phases.  Phases 1 and 2 (lanes = points load / store an LDS tile of 64 points
//                    + 2 of look-ahead per column, lanes = columns sweep it, forwards then backwards, the slopes go to the workspace) are k_lsq_cell's text: the sweep is
//                    duplicated here on purpose (DESIGN.md 3 names the fold), so that k_lsq_cell's code object stays what the validated build describes.
//                    Phase 3, after the barrier, lanes = queries (q = lane, lane + 64, ...): the Hermite evaluation of every column of a channel (k_lsq_cell's expression: a
//                    query at a saved time returns the saved bits), pred and dpred stored -- both contiguous along q: every store is one row segment of <= 512 B --, and
//                    var = s^T M s with the cell's (or its group's) covariance M: the upper triangle mirrored into 64 doubles of LDS once per cell, read at addresses that are
//                    the same for every lane (a broadcast, no bank conflict) and compile-time constants (the loops over the keys are unrolled over PLH_LSQ_MAX_SENS: no
//                    dynamically indexed register array).  Every output is computed by the lane that stores it, in one order: no atomics, no cross-lane reduction, and the bits
//                    do not depend on the chunking or the pointer kind.
#pragma once

#include "plh_resample.h"

// (PL_SYNC, dfn_cell.h: the intra-wave phase separator between an LDS store and another lane's load of it)

namespace plpr {

constexpr int NS = PLH_LSQ_MAX_SENS;      // sensitivity columns at most
constexpr int NCH = PLH_LSQ_MAX_CHANNELS; // channels at most
constexpr int NCOL = NCH * (1 + NS);      // columns of a cell at most
constexpr int TILE = plrs::TILE;          // points per tile = lanes
constexpr int LD = TILE + 3;              // tile row: 64 points, 2 of look-ahead, 1 of padding (an odd stride in 8-byte words)

struct Args {
  plrs::Args rs;                            // as k_resample_prep / k_resample_locate take it (width = n_ch (1 + n_sens); src and dst unused)
  int n_sens, n_ch, n_groups;
  plh_predict_channel ch[NCH];              // (device pointers) curve [n_cells][max_pts], dcurve [n_cells][n_sens][max_pts]; pred, var [n_cells][n_q], dpred [n_cells][n_sens][n_q]: each may be NULL
  const double* cov;                        // [n_prob][n_sens][n_sens] or NULL
  const int* group_off;                     // [n_groups + 1] (device) or NULL: the cell's own matrix
};
// channel c's members without a dynamically indexed copy of the kernel argument (c is wave-uniform: scalar selects)
#define PLPR_CH(A, c, member) ((c) == 0 ? (A).ch[0].member : (c) == 1 ? (A).ch[1].member : (A).ch[2].member)

__global__ void __launch_bounds__(TILE) k_predict_cell(Args A) {
  __shared__ double T[NCOL][LD];
  __shared__ double M[NS][NS];
  const plrs::Args& a = A.rs;
  const int lc = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (lc >= a.n_chunk) return;
  const size_t cell = (size_t)a.cell0 + lc;
  const int ns = A.n_sens, nch = A.n_ch, cw = 1 + ns, ncol = nch * cw, nq = a.n_q;       // (cw: columns per channel)
  if (!a.w.ok[lc]) {                                                 // (none of its points is read)
    for (int c = 0; c < nch; c++) {
      double* pc = PLPR_CH(A, c, pred); double* dc = PLPR_CH(A, c, dpred); double* vc = PLPR_CH(A, c, var);
      for (int q = lane; q < nq; q += TILE) {
        if (pc) pc[cell * nq + q] = plrs::rs_nan();
        if (vc) vc[cell * nq + q] = plrs::rs_nan();
        if (dc) for (int k = 0; k < ns; k++) dc[(cell * ns + k) * nq + q] = plrs::rs_nan();
      }
    }
    return;
  }
  // the covariance of the cell's problem: the upper triangle, mirrored; rows and columns past n_sens are 0 and never read.  The group is found once per wave
  // (cell is wave-uniform: a scalar binary search for the last offset <= cell)
  if (A.cov) {
    size_t prob = cell;
    if (A.group_off) {
      int lo = 0, hi = A.n_groups - 1;
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((size_t)A.group_off[mid] <= cell) lo = mid; else hi = mid - 1; }
      prob = (size_t)lo;
    }
    const int i = lane >> 3, j = lane & 7, r = i < j ? i : j, cc = i < j ? j : i;
    M[i][j] = i < ns && j < ns ? A.cov[(prob * ns + r) * ns + cc] : 0.0;
  }
  const plh_run_info* ri = a.run_info + cell * a.n_runs;
  const double* x = a.t + cell * a.max_pts;
  const double* fac = a.w.fac + (size_t)lc * a.max_pts * 2;
  double* sl = a.w.slope + (size_t)lc * ncol * a.max_pts;
  // column j = channel j / cw, its curve (k = 0) or row k - 1 of its dcurve
  auto chcol = [&](int c, int k) { return k == 0 ? PLPR_CH(A, c, curve) + cell * a.max_pts : PLPR_CH(A, c, dcurve) + (cell * ns + (k - 1)) * a.max_pts; };
  auto ycol = [&](int j) { return chcol(j / cw, j % cw); };
  // lanes = points: rows [p0, p0 + cnt) of every column <-> the tile (cnt <= TILE + 2; the look-ahead points ride on lanes 0 and 1)
  auto load = [&](bool slopes, int p0, int cnt) {
    for (int c = 0; c < ncol; c++) {
      const double* src = (slopes ? sl + (size_t)c * a.max_pts : ycol(c)) + p0;
      if (lane < cnt) T[c][lane] = src[lane];
      if (TILE + lane < cnt) T[c][TILE + lane] = src[TILE + lane];
    }
  };
  auto store = [&](int p0, int cnt) {
    for (int c = 0; c < ncol; c++) if (lane < cnt) sl[(size_t)c * a.max_pts + p0 + lane] = T[c][lane];
  };
  const bool act = lane < ncol;                                      // lanes = columns
  double* Tc = T[act ? lane : 0];
  for (int r = 0; r < a.n_runs; r++) {
    const int n = ri[r].iterations, s0 = a.w.run0[(size_t)lc * a.n_runs + r];
    if (n < 2) continue;
    const double* xr = x + s0; const double* f = fac + (size_t)s0 * 2;
    // forward sweep: g_i = rhs_i - w_i g_{i-1} over the run's tiles (n = 2, 3: the slopes themselves, one tile)
    double hm = 0, h = 0, dm = 0, d = 0, g = 0, y2 = 0, s = 0;
    for (int b = 0; b < n; b += TILE) {
      const int e = n - b < TILE ? n : b + TILE;
      load(false, s0 + b, n - b < TILE + 2 ? n - b : TILE + 2);
      PL_SYNC();
      if (act) {
        if (n == 2) { const double dd = (Tc[1] - Tc[0]) / (xr[1] - xr[0]); Tc[0] = dd; Tc[1] = dd; }
        else if (n == 3) {                                           // the parabola's slopes at its three points
          const double h0 = xr[1] - xr[0], h1 = xr[2] - xr[1], d0 = (Tc[1] - Tc[0]) / h0, d1 = (Tc[2] - Tc[1]) / h1, c = (d1 - d0) / (h0 + h1);
          Tc[0] = d0 - h0 * c; Tc[1] = d0 + h0 * c; Tc[2] = d1 + h1 * c;
        } else for (int i = b; i < e; i++) {
          if (i == 0) {
            hm = xr[1] - xr[0]; h = xr[2] - xr[1];
            const double y0 = Tc[0], y1 = Tc[1]; y2 = Tc[2];
            dm = (y1 - y0) / hm; d = (y2 - y1) / h;                  // d_{i-1}, d_i
            g = ((3.0 * hm + 2.0 * h) * h * dm + hm * hm * d) / (hm + h);
            Tc[0] = g;
          } else if (i < n - 1) {
            g = 3.0 * (h * dm + hm * d) - f[2 * i] * g;
            Tc[i - b] = g;
            if (i < n - 2) { const double yn = Tc[i + 2 - b]; hm = h; h = xr[i + 2] - xr[i + 1]; dm = d; d = (yn - y2) / h; y2 = yn; }
          } else {                                                   // (here hm = h_{n-3}, h = h_{n-2}, dm = d_{n-3}, d = d_{n-2})
            g = ((3.0 * h + 2.0 * hm) * hm * d + h * h * dm) / (hm + h) - f[2 * (n - 1)] * g;
            s = g / f[2 * (n - 1) + 1];
            Tc[i - b] = s;
          }
        }
      }
      PL_SYNC();
      store(s0 + b, e - b);
      PL_SYNC();
    }
    if (n < 4) continue;
    // back substitution: s_i = (g_i - c_i s_{i+1}) / p_i with c_0 = h_0 + h_1, c_i = h_{i-1}; the last tile is still in LDS
    for (int b = (n - 1) / TILE * TILE; b >= 0; b -= TILE) {
      const int e = n - b < TILE ? n : b + TILE;
      if (e < n) { load(true, s0 + b, TILE); PL_SYNC(); }
      if (act) for (int i = e - 1; i >= b; i--) {
        if (i == n - 1) continue;
        if (i >= 1) s = (Tc[i - b] - (xr[i] - xr[i - 1]) * s) / f[2 * i + 1];
        else s = (Tc[0] - (xr[2] - xr[0]) * s) / f[1];
        Tc[i - b] = s;
      }
      PL_SYNC();
      store(s0 + b, e - b);
      PL_SYNC();
    }
  }
  // lanes = queries: they read slopes that other lanes stored to the workspace, and M
  __syncthreads();
  const int* loc_i = a.w.loc_i + (size_t)lc * nq; const double* loc_t = a.w.loc_t + (size_t)lc * nq;
  for (int q = lane; q < nq; q += TILE) {
    const double tv = loc_t[q]; const int i = loc_i[q];
    const bool bad = !(tv == tv), one = i < 0;
    const int i0 = bad ? 0 : one ? ~i : i;
    double x0 = 0, x1 = 0, hh = 1, u = 0, ee = 0;
    if (!bad && !one) { x0 = x[i0]; x1 = x[i0 + 1]; hh = x1 - x0; u = tv - x0; ee = tv - x1; }
    auto eval = [&](int c, int k) {
      if (bad) return plrs::rs_nan();
      const double* y = chcol(c, k);
      if (one) return y[i0];
      const double* sc = sl + (size_t)(c * cw + k) * a.max_pts;
      const double y0 = y[i0], y1 = y[i0 + 1], s0 = sc[i0], s1 = sc[i0 + 1];
      const double d = (y1 - y0) / hh, c3 = (s0 + s1 - 2.0 * d) / (hh * hh);
      if (u <= -ee) return y0 + u * (s0 + u * ((3.0 * d - 2.0 * s0 - s1) / hh + u * c3));          // about the left node
      return y1 + ee * (s1 + ee * ((s0 + 2.0 * s1 - 3.0 * d) / hh + ee * c3));                     // about the right node
    };
    for (int c = 0; c < nch; c++) {
      double* pc = PLPR_CH(A, c, pred); double* dc = PLPR_CH(A, c, dpred); double* vc = PLPR_CH(A, c, var);
      if (pc) pc[cell * nq + q] = eval(c, 0);
      if (!dc && !vc) continue;
      double S[NS];
#pragma unroll
      for (int k = 0; k < NS; k++) S[k] = k < ns ? eval(c, 1 + k) : 0.0;
      if (dc) {
#pragma unroll
        for (int k = 0; k < NS; k++) if (k < ns) dc[(cell * ns + k) * nq + q] = S[k];
      }
      if (vc) {                                                      // v_i = sum_j M_ij s_j (j ascending), var = sum_i s_i v_i (i ascending)
        double var = 0.0;
#pragma unroll
        for (int k = 0; k < NS; k++) if (k < ns) {
          double v = 0.0;
#pragma unroll
          for (int l = 0; l < NS; l++) if (l < ns) v += M[k][l] * S[l];
          var += S[k] * v;
        }
        vc[cell * nq + q] = var;
      }
    }
  }
}

// the launches of one chunk
inline void launch_chunk(hipStream_t st, const Args& A) {
  const plrs::Args& a = A.rs;
  PL_LAUNCH(plrs::k_resample_prep, (unsigned)((a.n_chunk + TILE - 1) / TILE), TILE, st, a);
  PL_LAUNCH(plrs::k_resample_locate, (unsigned)(((size_t)a.n_chunk * a.n_q + TILE - 1) / TILE), TILE, st, a);
  PL_LAUNCH(k_predict_cell, (unsigned)a.n_chunk, TILE, st, A);
}

}  // namespace plpr

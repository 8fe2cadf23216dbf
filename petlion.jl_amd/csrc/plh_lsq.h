// plh_lsq.h -- plh_lsq / plh_lsq_multi: the weighted least-squares misfit of every cell's measured curves (V; with plh_lsq_multi up to three channels: V, I, T_avg) against data,
// its gradient and its Gauss-Newton matrix (include/petlion_hip.h states the definition).  Like plh_resample.h: kernels over the saved points plh_integrate / plh_integrate_sens wrote, no model variant, host translation unit.
//
// The curve S_V and the sensitivity rows S_k are plh_resample's functions, so k_resample_prep (status, run starts, elimination factors) and k_resample_locate (run, clamped
// time and interval of every query) run unchanged; they read t, run_info and tq only.  Then one kernel:
//   k_lsq_cell   one wave per cell over its n_ch (1 + n_sens) columns, the channels side by side (channel c: its curve, then the rows of its dcurve[cell]; <= 27 columns, so the
//                sweeps -- the serial part, lanes = columns -- of three channels take the time of one).  Every column is contiguous ALONG POINTS here (k_resample_field's columns
//                are contiguous across columns), so the slopes are computed through an LDS tile of 64 consecutive points per column:
//                  lanes = points    load a tile (one contiguous segment of <= 512 B per column, plus the two points the forward sweep looks ahead),
//                  lanes = columns   sweep it in place (k_resample_field's arithmetic, operation for operation; the rows are padded to an odd stride: no two columns on a bank),
//                  lanes = points    store it to the slope workspace [chunk][1 + n_sens][max_pts];
//                forwards over a run's tiles (right-hand sides), then backwards (slopes).  A lane reloads from the workspace only what it stored itself; one
//                workgroup barrier then hands the slopes to the lanes of the next phase.
//                Then lanes = queries (q = lane, lane + 64, ...): the Hermite evaluation of every column, cost / grad / upper triangle of JtJ summed in registers in that
//                order (queries outer, channels inner: the 45 running sums are shared by the channels), a fixed-order butterfly over the wave, and lane 0 stores the cell's results: the bits do not depend on the chunking or the pointer kind.
#pragma once

#include "plh_resample.h"

// (PL_SYNC, dfn_cell.h: the intra-wave phase separator between an LDS store and another lane's load of it)

namespace pllsq {

constexpr int NS = PLH_LSQ_MAX_SENS;      // sensitivity columns at most: a lane keeps 1 + NS + NS (NS + 1) / 2 sums
constexpr int NCH = PLH_LSQ_MAX_CHANNELS; // channels at most
constexpr int NCOL = NCH * (1 + NS);      // columns of a cell at most
constexpr int TILE = plrs::TILE;          // points per tile = lanes
constexpr int LD = TILE + 3;              // tile row: 64 points, 2 of look-ahead, 1 of padding (an odd stride in 8-byte words)

struct Args {
  plrs::Args rs;                            // as k_resample_prep / k_resample_locate take it (width = n_ch (1 + n_sens); src and dst unused)
  int n_sens, per_cell, n_ch;
  plh_lsq_channel ch[NCH];                  // (device pointers) curve [n_cells][max_pts], dcurve [n_cells][n_sens][max_pts]; y, w: [n_q] or [n_cells][n_q], w may be NULL; resid
  double* cost; double* grad; double* JtJ;
};
// channel c's members without a dynamically indexed copy of the kernel argument (c is wave-uniform: scalar selects)
#define PLLSQ_CH(A, c, member) ((c) == 0 ? (A).ch[0].member : (c) == 1 ? (A).ch[1].member : (A).ch[2].member)

__global__ void __launch_bounds__(TILE) k_lsq_cell(Args A) {
  __shared__ double T[NCOL][LD];
  const plrs::Args& a = A.rs;
  const int lc = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (lc >= a.n_chunk) return;
  const size_t cell = (size_t)a.cell0 + lc;
  const int ns = A.n_sens, nch = A.n_ch, cw = 1 + ns, ncol = nch * cw, nq = a.n_q;       // (cw: columns per channel)
  if (!a.w.ok[lc]) {                                                 // (none of its points is read)
    for (int c = 0; c < nch; c++) { double* rc = PLLSQ_CH(A, c, resid); if (rc) for (int q = lane; q < nq; q += TILE) rc[cell * nq + q] = plrs::rs_nan(); }
    for (int k = lane; k < ns; k += TILE) A.grad[cell * ns + k] = plrs::rs_nan();
    for (int k = lane; k < ns * ns; k += TILE) A.JtJ[cell * ns * ns + k] = plrs::rs_nan();
    if (lane == 0) A.cost[cell] = plrs::rs_nan();
    return;
  }
  const plh_run_info* ri = a.run_info + cell * a.n_runs;
  const double* x = a.t + cell * a.max_pts;
  const double* fac = a.w.fac + (size_t)lc * a.max_pts * 2;
  double* sl = a.w.slope + (size_t)lc * ncol * a.max_pts;
  // column j = channel j / cw, its curve (k = 0) or row k - 1 of its dcurve
  auto chcol = [&](int c, int k) { return k == 0 ? PLLSQ_CH(A, c, curve) + cell * a.max_pts : PLLSQ_CH(A, c, dcurve) + (cell * ns + (k - 1)) * a.max_pts; };
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
  // lanes = queries: they read slopes that other lanes stored to the workspace
  __syncthreads();
  const int* loc_i = a.w.loc_i + (size_t)lc * nq; const double* loc_t = a.w.loc_t + (size_t)lc * nq;
  const size_t d0 = A.per_cell ? cell * nq : 0;                      // the cell's row of y / w
  double cost = 0.0, G[NS], H[NS][NS];                               // H: the upper triangle
#pragma unroll
  for (int k = 0; k < NS; k++) {
    G[k] = 0.0;
#pragma unroll
    for (int l = k; l < NS; l++) H[k][l] = 0.0;
  }
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
    for (int c = 0; c < nch; c++) {                                  // channels inner: one fixed order of the sums
      const double* wd = PLLSQ_CH(A, c, w); double* resid = PLLSQ_CH(A, c, resid);
      const double wq = wd ? wd[d0 + q] : 1.0;
      if (wq == 0.0) { if (resid) resid[cell * nq + q] = 0.0; continue; }      // left out of this channel: not evaluated
      const double rq = wq * (eval(c, 0) - PLLSQ_CH(A, c, y)[d0 + q]);
      if (resid) resid[cell * nq + q] = rq;
      cost += rq * rq;
      double J[NS];
#pragma unroll
      for (int k = 0; k < NS; k++) J[k] = k < ns ? wq * eval(c, 1 + k) : 0.0;
#pragma unroll
      for (int k = 0; k < NS; k++) if (k < ns) {
        G[k] += J[k] * rq;
#pragma unroll
        for (int l = k; l < NS; l++) if (l < ns) H[k][l] += J[k] * J[l];
      }
    }
  }
  // the wave's sums, in one order: every lane ends with the same bits
  auto wave_sum = [](double v) { for (int m = TILE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m); return v; };
  cost = wave_sum(cost);
#pragma unroll
  for (int k = 0; k < NS; k++) if (k < ns) {
    G[k] = wave_sum(G[k]);
#pragma unroll
    for (int l = k; l < NS; l++) if (l < ns) H[k][l] = wave_sum(H[k][l]);
  }
  if (lane == 0) {
    A.cost[cell] = 0.5 * cost;
#pragma unroll
    for (int k = 0; k < NS; k++) if (k < ns) {
      A.grad[cell * ns + k] = G[k];
#pragma unroll
      for (int l = k; l < NS; l++) if (l < ns) { A.JtJ[(cell * ns + k) * ns + l] = H[k][l]; A.JtJ[(cell * ns + l) * ns + k] = H[k][l]; }
    }
  }
}

// the launches of one chunk
inline void launch_chunk(hipStream_t st, const Args& A) {
  const plrs::Args& a = A.rs;
  PL_LAUNCH(plrs::k_resample_prep, (unsigned)((a.n_chunk + TILE - 1) / TILE), TILE, st, a);
  PL_LAUNCH(plrs::k_resample_locate, (unsigned)(((size_t)a.n_chunk * a.n_q + TILE - 1) / TILE), TILE, st, a);
  PL_LAUNCH(k_lsq_cell, (unsigned)a.n_chunk, TILE, st, A);
}

}  // namespace pllsq
